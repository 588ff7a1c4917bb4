// orb_kernels.hip - ORB on the GPU: `cv2.ORB_create(...).detectAndCompute(img, None)` for 8-bit images.
//
// Replaces the detector of the reference's default configuration (`--detector orb --matcher bf`, `_get_opencv_detector` at
// slam/core/features_utils.py:33-55) and produces what sslam_bf_match_dev consumes: uint8 rows of 32 bytes and a device
// count.  Semantics: tests/orb_ref.py restates OpenCV's ORB_Impl::detectAndCompute stage by stage and lists what could not be
// confirmed without cv2; the kernels equal it bit for bit.  THE STATED DEVIATION: the default sampling pattern is OpenCV's
// makeRandomPattern at patch size 31 (cv::RNG(0x34985739)), not its learned table, which is not available here - descriptors
// are self-consistent, not interchangeable with cv2's; a user pattern can be given at creation.
//
// Everything the host decides is in orb_plan.hpp (sizes, offsets, quotas, tables, tile tables, refusals).  A frame is
//   1 memset of the control block (counts and cuts, 256 bytes)
//   L orb_level_kernel      the level chain: level 0 = grey of the input, level l = INTER_LINEAR_EXACT of level l - 1's interior.
//                           A stored pixel (border included) per lane, a wavefront along a row: the border is the reflect-101 image of the interior, so a
//                           lane reflects its coordinate and computes that interior pixel - interior and border in one launch.
//   1 orb_fast_kernel       all levels, a 32 x 32 tile per workgroup (four strips of 32 x 8) through the plan's per-level tile
//                           table: FAST-9/16 scores of a strip and a one-pixel halo in LDS, strict 8-neighbour NMS, the border filter; appends candidates
//                           (one integer atomic per workgroup reserves the tile's range of its level's list).
//   1 orb_blur_kernel       all levels, a stored pixel per lane: 7 x 7 fixed-point Gaussian at the reflected coordinate.
//   1 orb_response_kernel   all levels: the first cut read off the level's 256-bin score histogram, built in LDS (exact, ties
//                           kept by construction), then the Harris
//                           response (exact integer sums, float32 tail one operation at a time) or the FAST score of every
//                           candidate that passed, stored as the monotone uint32 image of the float32; 0 = cut.
//   1 orb_select_kernel     a workgroup per level: exact radix select (4 x 8 bits) of the quota-th largest key, compaction of the
//                           survivors' output keys (quota plus ties).
//   1 orb_describe_kernel   all levels, a keypoint per wavefront, four per workgroup: its rank under the output key (level,
//                           response descending, y, x - unique, so the atomic append order never reaches the output), the
//                           intensity-centroid moments over the disc, fastAtan2, cos / sin once, the 512 rotated taps shared by the
//                           lanes and the 32 bytes assembled from 4 ballots.
// = 6 + L launches, no host synchronisation and no copy of a count in between: grids come from the plan's worst case (tiles)
// or are fixed and stride over a device-written count.
// MEMORY SAFETY: every level is stored with a reflect-101 border of max(edgeThreshold, 22, 4) + 1 >= 23 pixels.  A candidate
// passed the border filter, so it is at least edgeThreshold >= 3 inside its level; every read around it - the Harris block
// with its derivative (reach 4), the disc of the orientation (reach 15), a rotated tap (|x|, |y| <= 15 is checked at creation,
// so the rounded rotation stays within 22) - is inside the stored border.  The blur and the resize read at reflected (interior)
// coordinates with reach 3 and 1.  After the border filter only integer coordinates exist.  A candidate index is checked against
// the level's capacity ceil(w / 2) ceil(h / 2) before the store although strict NMS cannot exceed it.  All loops are bounded by
// plan constants or by device counts clamped to those capacities.
// PARITY UNPINNED: cv2 is absent here; tests/orb_ref.py names what could not be confirmed.
#include "common.hpp"
#include "feat_device.hpp"
#include "feat_host.hpp"
#include "geom_common.hpp"
#include "orb_plan.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace {

using namespace sslam;

constexpr int ORB_T = 256;
constexpr int ORB_FAST_SUB = ORB_FAST_H / ORB_TILE_H;          // a FAST tile is 4 strips of 32 x 8 under one another
constexpr int ORB_HALO_W = ORB_TILE_W + 2, ORB_HALO_H = ORB_TILE_H + 2;
static_assert(ORB_FAST_W == ORB_TILE_W && ORB_FAST_H % ORB_TILE_H == 0, "strips of the FAST tile");

struct OrbCtl {                                  // zeroed at the head of every call (counts, cuts)
    int32_t ncand[ORB_MAX_LEVELS], nsurv[ORB_MAX_LEVELS], cut1[ORB_MAX_LEVELS];
    uint32_t cut2[ORB_MAX_LEVELS];               // float32 bits
};

struct OrbLevelDev {
    int w, h, stride, rows;
    int quota, cut1_n;
    int fast_tx, fast_base, pad_tx, pad_base;
    int cand_cap;
    uint32_t cand_off;
    long long off;
    float scale;
};

struct OrbArgs {
    int nactive, border, edge, score_type, fast_t;
    int fast_tiles, blur_tiles;
    OrbLevelDev lv[ORB_MAX_LEVELS];
    unsigned long long umax4;                    // umax[v] in bits 4 v .. 4 v + 3
    int gauss[7];
    float harris_k, harris_scale4;
    FastAtan atan;
    float patch_size;
    uint8_t* img; uint8_t* blur;                 // the two slabs
    uint32_t* cand_xy; uint32_t* cand_score; uint32_t* cand_key;      // [cand_total]
    unsigned long long* skey;                    // [cand_total] the survivors' output keys: ~response key << 32 | y << 16 | x
    OrbCtl* ctl;
    const int8_t* pattern;                       // [512][2]
    float* xy_out; float* aux_out; uint8_t* desc_out; int32_t* n_out;
};

// the source tap and its 8-bit weight of INTER_LINEAR_EXACT along one axis: the exact rational ((2 d + 1) sn - dn) / (2 dn)
__device__ __forceinline__ void orb_tap(int d, int sn, int dn, int& s0, int& s1, int& c) {
    const int num = (2 * d + 1) * sn - dn, den = 2 * dn;         // sn >= dn: num >= 0
    int s = num / den;
    c = ((num - s * den) * 512 + den) / (2 * den);
    if (s >= sn - 1) { s = sn - 1; c = 0; }
    s0 = s; s1 = min(s + 1, sn - 1);
}

// ---- the level chain ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORB_T) void orb_level_kernel(OrbArgs a, int l, const uint8_t* __restrict__ src, int C) {
    const OrbLevelDev L = a.lv[l];
    const int px = blockIdx.x * 64 + (threadIdx.x & 63), py = blockIdx.y * (ORB_T / 64) + (threadIdx.x >> 6);
    if (px >= L.stride || py >= L.rows) return;
    const int p = py * L.stride + px;
    const int x = reflect101(px - a.border, L.w), y = reflect101(py - a.border, L.h);
    int v;
    if (l == 0) {
        const uint8_t* s = src + ((size_t)y * L.w + x) * C;
        v = bgr_to_grey(s, C);
    } else {
        const OrbLevelDev S = a.lv[l - 1];
        const uint8_t* s = a.img + S.off + (size_t)a.border * S.stride + a.border;
        int x0, x1, cx, y0, y1, cy;
        orb_tap(x, S.w, L.w, x0, x1, cx);
        orb_tap(y, S.h, L.h, y0, y1, cy);
        const uint8_t* r0 = s + (size_t)y0 * S.stride;
        const uint8_t* r1 = s + (size_t)y1 * S.stride;
        const int h0 = (256 - cx) * r0[x0] + cx * r0[x1], h1 = (256 - cx) * r1[x0] + cx * r1[x1];
        v = ((256 - cy) * h0 + cy * h1 + (1 << 15)) >> 16;
    }
    a.img[L.off + p] = (uint8_t)v;
}

// the level of a tile of an all-level launch: `base_of(level)` is the level's first tile
template <class Base>
__device__ __forceinline__ int orb_level_of(const OrbArgs& a, int tile, Base base_of) {
    int l = 0;
    for (int i = 1; i < ORB_MAX_LEVELS; ++i)
        if (i < a.nactive && tile >= base_of(a.lv[i])) l = i;
    return l;
}

// ---- FAST-9/16 ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool orb_arc9(unsigned m) {
    m |= m << 16;
    const unsigned a2 = m & (m >> 1), a4 = a2 & (a2 >> 2), a8 = a4 & (a4 >> 4);
    return (a8 & (m >> 8) & 0xffffu) != 0;
}

// the score of an interior pixel at least 3 from the edge: the largest threshold at which it is still a corner, 0 if it is none
__device__ __forceinline__ int orb_fast_score(const uint8_t* __restrict__ p, int stride, int t) {
    constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int v = p[0];
    int d[16];
    unsigned hi = 0, lo = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        d[k] = v - (int)p[DY[k] * stride + DX[k]];
        hi |= (unsigned)(d[k] > t) << k;
        lo |= (unsigned)(d[k] < -t) << k;
    }
    const bool up = orb_arc9(hi);
    if (!up && !orb_arc9(lo)) return 0;
    // 9 of 16 brighter and 9 of 16 darker exclude each other, and the side without an arc at t cannot reach t + 1: the score is
    // max_k min_9 of the differences of the side that has the arc.  Sliding minimum over 9 by doubling: 2, 4, 8, then one more.
    int e[16], m2[16], m4[16], best = -255;
#pragma unroll
    for (int k = 0; k < 16; ++k) e[k] = up ? d[k] : -d[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) m2[k] = min(e[k], e[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m4[k] = min(m2[k], m2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) best = max(best, min(min(m4[k], m4[(k + 4) & 15]), e[(k + 8) & 15]));
    return best - 1;                                           // >= t: it is a corner at t
}

__global__ __launch_bounds__(ORB_T) void orb_fast_kernel(OrbArgs a) {
    __shared__ int s_score[ORB_HALO_H][ORB_HALO_W];
    __shared__ int s_wcnt[ORB_FAST_SUB][ORB_T / 64], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l = orb_level_of(a, blockIdx.x, [](const OrbLevelDev& L) { return L.fast_base; });
    const OrbLevelDev L = a.lv[l];
    const int tile = blockIdx.x - L.fast_base;
    const int x0 = (tile % L.fast_tx) * ORB_FAST_W, y0 = (tile / L.fast_tx) * ORB_FAST_H;
    const uint8_t* im = a.img + L.off + (size_t)a.border * L.stride + a.border;
    const int tx = tid & (ORB_TILE_W - 1), ty = tid / ORB_TILE_W, x = x0 + tx;
    int sc[ORB_FAST_SUB];
    bool kp[ORB_FAST_SUB];
    unsigned long long bal[ORB_FAST_SUB];
#pragma unroll
    for (int sub = 0; sub < ORB_FAST_SUB; ++sub) {
        const int ys = y0 + sub * ORB_TILE_H, y = ys + ty;
        if (sub) __syncthreads();                              // (the strip before has been read)
        for (int i = tid; i < ORB_HALO_W * ORB_HALO_H; i += ORB_T) {
            const int hy = i / ORB_HALO_W, hx = i - hy * ORB_HALO_W;
            const int px = x0 - 1 + hx, py = ys - 1 + hy;
            int s = 0;
            if (px >= 3 && px < L.w - 3 && py >= 3 && py < L.h - 3) s = orb_fast_score(im + (size_t)py * L.stride + px, L.stride, a.fast_t);
            s_score[hy][hx] = s;
        }
        __syncthreads();
        const int s = s_score[ty + 1][tx + 1];
        bool keep = s > 0 && x >= a.edge && x < L.w - a.edge && y >= a.edge && y < L.h - a.edge;
        if (keep) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
                    if (dy != 1 || dx != 1) keep = keep && s > s_score[ty + dy][tx + dx];
        }
        sc[sub] = s; kp[sub] = keep; bal[sub] = __ballot(keep);
        if (lane == 0) s_wcnt[sub][wave] = __popcll(bal[sub]);
    }
    // one append per workgroup: the wavefronts' counts meet in LDS, one lane reserves the tile's range of the level's list
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int i = 0; i < ORB_FAST_SUB * (ORB_T / 64); ++i) total += s_wcnt[0][i];
        s_base = total ? atomicAdd(&a.ctl->ncand[l], total) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < ORB_FAST_SUB; ++sub)
        if (kp[sub]) {
            int i = s_base + __popcll(bal[sub] & ((1ull << lane) - 1));
            for (int j = 0; j < sub * (ORB_T / 64) + wave; ++j) i += s_wcnt[0][j];
            if (i < L.cand_cap) {
                a.cand_xy[L.cand_off + i] = (uint32_t)(y0 + sub * ORB_TILE_H + ty) << 16 | (uint32_t)x;
                a.cand_score[L.cand_off + i] = (uint32_t)sc[sub];
            }
        }
}

// ---- the blurred levels ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ORB_T) void orb_blur_kernel(OrbArgs a) {
    const int tid = threadIdx.x;
    const int l = orb_level_of(a, blockIdx.x, [](const OrbLevelDev& L) { return L.pad_base; });
    const OrbLevelDev L = a.lv[l];
    const int tile = blockIdx.x - L.pad_base;
    const int px = (tile % L.pad_tx) * ORB_TILE_W + (tid & (ORB_TILE_W - 1)), py = (tile / L.pad_tx) * ORB_TILE_H + tid / ORB_TILE_W;
    if (px >= L.stride || py >= L.rows) return;
    const int x = reflect101(px - a.border, L.w), y = reflect101(py - a.border, L.h);
    const uint8_t* c = a.img + L.off + (size_t)(y + a.border) * L.stride + (x + a.border);
    int v = 0;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const uint8_t* r = c + (j - 3) * L.stride;
        int hz = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) hz += a.gauss[i] * (int)r[i - 3];
        v += a.gauss[j] * hz;
    }
    a.blur[L.off + (size_t)py * L.stride + px] = (uint8_t)((v + (1 << 15)) >> 16);
}

// ---- the first cut and the response --------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t orb_float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t orb_key_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }

// The bin of the `rem`-th largest entry of a 256-bin histogram in LDS (the bins' total is >= rem >= 1), and its rank inside
// that bin: suffix sums over the bins by wavefront shuffles, the four wavefronts' totals through LDS.  Every thread of the
// workgroup (>= 256 threads) calls it; the answer is in *digit / *rank after the call.
__device__ __forceinline__ void orb_pick_bin(const uint32_t* hist, int rem, int* tot4, int* digit, int* rank) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int v = 0, sfx = 0;
    if (tid < 256) {
        v = (int)hist[tid];
        sfx = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(sfx, o);
            if (lane + o < 64) sfx += t;
        }
        if (lane == 0) tot4[wave] = sfx;
    }
    __syncthreads();
    if (tid < 256) {
        for (int w = wave + 1; w < 4; ++w) sfx += tot4[w];      // entries in this bin or above
        if (sfx >= rem && sfx - v < rem) { *digit = tid; *rank = rem - (sfx - v); }
    }
    __syncthreads();
}

__global__ __launch_bounds__(ORB_T) void orb_response_kernel(OrbArgs a) {
    __shared__ int s_cut, s_rank, s_tot[4];
    __shared__ uint32_t s_hist[256];
    const int l = blockIdx.y;
    const OrbLevelDev L = a.lv[l];
    const int n = min(a.ctl->ncand[l], L.cand_cap);
    // retainBest(cut1_n) on the FAST scores: keep everything when no more than that, nothing for 0, else the n-th largest, read
    // off the level's 256-bin score histogram, which every workgroup builds for itself in LDS (8 scores per thread and turn)
    if (threadIdx.x == 0) s_cut = n > L.cut1_n ? 256 : 0;
    if (n > L.cut1_n && L.cut1_n > 0) {                        // (uniform)
        s_hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += ORB_T * 8) {
            int sc[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int i = i0 + u * ORB_T + (int)threadIdx.x; sc[u] = i < n ? (int)a.cand_score[L.cand_off + i] : -1; }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (sc[u] >= 0) atomicAdd(&s_hist[sc[u] & 255], 1u);
        }
        __syncthreads();
        orb_pick_bin(s_hist, L.cut1_n, s_tot, &s_cut, &s_rank);
    } else {
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl->cut1[l] = s_cut;
    const int cut = s_cut;
    for (int i = blockIdx.x * ORB_T + threadIdx.x; i < n; i += gridDim.x * ORB_T) {
        const int s = (int)a.cand_score[L.cand_off + i];
        uint32_t key = 0;
        if (s >= cut) {
            float r;
            if (a.score_type == 0) {
                const uint32_t xy = a.cand_xy[L.cand_off + i];
                const uint8_t* c = a.img + L.off + (size_t)((int)(xy >> 16) + a.border) * L.stride + ((int)(xy & 0xffffu) + a.border);
                int A = 0, B = 0, Cc = 0;
                for (int dy = -3; dy <= 3; ++dy) {
                    const uint8_t* r0 = c + (dy - 1) * L.stride;
                    const uint8_t* r1 = c + dy * L.stride;
                    const uint8_t* r2 = c + (dy + 1) * L.stride;
#pragma unroll
                    for (int dx = -3; dx <= 3; ++dx) {
                        const int ix = ((int)r1[dx + 1] - (int)r1[dx - 1]) * 2 + ((int)r0[dx + 1] - (int)r0[dx - 1]) + ((int)r2[dx + 1] - (int)r2[dx - 1]);
                        const int iy = ((int)r2[dx] - (int)r0[dx]) * 2 + ((int)r2[dx - 1] - (int)r0[dx - 1]) + ((int)r2[dx + 1] - (int)r0[dx + 1]);
                        A += ix * ix; B += ix * iy; Cc += iy * iy;
                    }
                }
                const float fa = (float)A, fb = (float)B, fc = (float)Cc;
                const float t1 = fa * fc, t2 = fb * fb, sm = fa + fc;
                float t3 = a.harris_k * sm;
                t3 = t3 * sm;
                r = t1 - t2;
                r = r - t3;
                r = r * a.harris_scale4;
            } else {
                r = (float)s;
            }
            key = orb_float_key(r);
        }
        a.cand_key[L.cand_off + i] = key;
    }
}

// ---- the second cut: exact select of the quota-th largest key, compaction -----------------------------------------------
__global__ __launch_bounds__(ORB_SEL_T) void orb_select_kernel(OrbArgs a) {
    __shared__ uint32_t s_hist[256];
    __shared__ int s_live, s_remaining, s_digit, s_tot[4], wsum[ORB_SEL_T / 64], base;
    const int l = blockIdx.x, tid = threadIdx.x;
    const OrbLevelDev L = a.lv[l];
    const int n = min(a.ctl->ncand[l], L.cand_cap);
    const uint32_t* key = a.cand_key + L.cand_off;
    if (tid == 0) { s_live = 0; s_remaining = L.quota; base = 0; }
    __syncthreads();
    // a turn of the loops below covers 8 x 1024 keys, loaded together: the passes are bound by the latency of a dependent
    // load per turn, not by their arithmetic
    int live = 0;
    for (int i0 = 0; i0 < n; i0 += ORB_SEL_T * ORB_SEL_K) {
        uint32_t k[ORB_SEL_K];
#pragma unroll
        for (int u = 0; u < ORB_SEL_K; ++u) { const int i = i0 + u * ORB_SEL_T + tid; k[u] = i < n ? key[i] : 0u; }
#pragma unroll
        for (int u = 0; u < ORB_SEL_K; ++u) live += k[u] != 0;
    }
    if (live) atomicAdd(&s_live, live);
    __syncthreads();
    uint32_t kcut = 1;                                          // everything that passed the first cut
    if (s_live > L.quota) {                                     // (uniform)
        uint32_t mask = 0, prefix = 0;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            // (only what passed the first cut takes part; a wavefront whose digits agree - the top byte of responses of one
            //  magnitude - adds its count once instead of queueing 64 atomics on one bin)
            for (int i0 = 0; i0 < n; i0 += ORB_SEL_T * ORB_SEL_K) {
                uint32_t kk[ORB_SEL_K];
#pragma unroll
                for (int u = 0; u < ORB_SEL_K; ++u) { const int i = i0 + u * ORB_SEL_T + tid; kk[u] = i < n ? key[i] : 0u; }
#pragma unroll
                for (int u = 0; u < ORB_SEL_K; ++u) {
                    const uint32_t k = kk[u];
                    const bool act = k != 0 && (k & mask) == prefix;
                    const uint32_t d = (k >> shift) & 255u;
                    const unsigned long long am = __ballot(act);
                    if (am) {
                        const int lead = __ffsll((long long)am) - 1;
                        const uint32_t d0 = __shfl(d, lead);
                        if (__ballot(act && d == d0) == am) {
                            if ((tid & 63) == lead) atomicAdd(&s_hist[d0], (uint32_t)__popcll(am));
                        } else if (act) {
                            atomicAdd(&s_hist[d], 1u);
                        }
                    }
                }
            }
            __syncthreads();
            orb_pick_bin(s_hist, s_remaining, s_tot, &s_digit, &s_remaining);
            prefix |= (uint32_t)s_digit << shift;
            mask |= 255u << shift;
            __syncthreads();                                    // (s_digit and s_remaining have been read)
        }
        kcut = prefix;
    }
    if (tid == 0) a.ctl->cut2[l] = kcut == 1 ? 0xff800000u : orb_key_bits(kcut);
    for (int i0 = 0; i0 < n; i0 += ORB_SEL_T * ORB_SEL_K) {
        uint32_t kk[ORB_SEL_K], xy[ORB_SEL_K];
#pragma unroll
        for (int u = 0; u < ORB_SEL_K; ++u) {
            const int i = i0 + u * ORB_SEL_T + tid;
            kk[u] = i < n ? key[i] : 0u;
            xy[u] = i < n ? a.cand_xy[L.cand_off + i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < ORB_SEL_K; ++u)
            sslam::block_compact<ORB_SEL_T>(kk[u] >= kcut, wsum, base, [&](int o) {
                a.skey[L.cand_off + o] = (unsigned long long)(~kk[u]) << 32 | xy[u];
            });
    }
    if (tid == 0) a.ctl->nsurv[l] = base;
}

// ---- rank, orientation, descriptor, output: a keypoint per wavefront ---------------------------------------------------
__global__ __launch_bounds__(ORB_T) void orb_describe_kernel(OrbArgs a) {
    const int l = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const OrbLevelDev L = a.lv[l];
    int first = 0, total = 0;
    for (int i = 0; i < ORB_MAX_LEVELS; ++i)
        if (i < a.nactive) {
            const int c = min(a.ctl->nsurv[i], a.lv[i].cand_cap);
            if (i < l) first += c;
            total += c;
        }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.n_out[0] = total;
    const int n = min(a.ctl->nsurv[l], L.cand_cap);
    const unsigned long long* skey = a.skey + L.cand_off;
    for (int j = blockIdx.x * (ORB_T / 64) + wave; j < n; j += gridDim.x * (ORB_T / 64)) {
        const unsigned long long mine = skey[j];
        const uint32_t rk = ~(uint32_t)(mine >> 32), xy = (uint32_t)mine;
        int less = 0;
#pragma unroll 4
        for (int jj = lane; jj < n; jj += 64) less += skey[jj] < mine;
        const int pos = first + wave_sum(less);
        const int x = (int)(xy & 0xffffu), y = (int)(xy >> 16);
        const size_t centre = (size_t)(y + a.border) * L.stride + (x + a.border);
        // the intensity centroid over the disc: rows v = -15 .. 15 of half width umax[|v|]
        const uint8_t* c = a.img + L.off + centre;
        int m01 = 0, m10 = 0;
        for (int e = lane; e < ORB_PATCH * ORB_PATCH; e += 64) {
            const int v = e / ORB_PATCH - ORB_HALF, u = e % ORB_PATCH - ORB_HALF;
            if (abs(u) <= (int)(a.umax4 >> (4 * abs(v)) & 15)) {
                const int val = c[v * L.stride + u];
                m10 += u * val; m01 += v * val;
            }
        }
        m01 = wave_sum(m01); m10 = wave_sum(m10);
        const float ang = fast_atan2_deg(a.atan, (float)m01, (float)m10);
        const float rad = ang * a.atan.deg2rad;
        const float ca = (float)cos((double)rad), sa = (float)sin((double)rad);
        const uint8_t* bl = a.blur + L.off + centre;
        for (int k = 0; k < 4; ++k) {
            const int8_t* pt = a.pattern + 4 * (k * 64 + lane);         // points 2 p and 2 p + 1 of pair p = 64 k + lane
            int t[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float px = (float)pt[2 * e], py = (float)pt[2 * e + 1];
                const float xa = px * ca, yb = py * sa, xb = px * sa, ya = py * ca;
                const int ix = (int)rintf(xa - yb), iy = (int)rintf(xb + ya);
                t[e] = bl[iy * L.stride + ix];
            }
            const unsigned long long bits = __ballot(t[0] < t[1]);
            if (lane < 8) a.desc_out[(size_t)pos * 32 + k * 8 + lane] = (uint8_t)(bits >> (8 * lane));
        }
        if (lane == 0) {
            a.xy_out[2 * (size_t)pos] = (float)x * L.scale;
            a.xy_out[2 * (size_t)pos + 1] = (float)y * L.scale;
            a.aux_out[4 * (size_t)pos] = a.patch_size * L.scale;
            a.aux_out[4 * (size_t)pos + 1] = ang;
            a.aux_out[4 * (size_t)pos + 2] = __uint_as_float(orb_key_bits(rk));
            a.aux_out[4 * (size_t)pos + 3] = (float)l;
        }
    }
}

}  // namespace

struct sslam_orb {
    sslam_ctx* ctx = nullptr;
    OrbParams p;
    int max_w = 0, max_h = 0;
    long long cap = 0;                           // output rows any call can produce
    OrbPlan plan{};                              // of the last call (stage_read reads it)
    bool have_plan = false;
    sslam::OwnedSlab slab;
    uint8_t *img = nullptr, *blur = nullptr;
    uint32_t *cand_xy = nullptr, *cand_score = nullptr, *cand_key = nullptr;
    unsigned long long* skey = nullptr;
    OrbCtl* ctl = nullptr;
    int8_t* pattern = nullptr;
    float *xy = nullptr, *aux = nullptr;         // outputs of the host entry
    uint8_t* desc = nullptr;
    int32_t* n = nullptr;
};

namespace {

// the slab-backed pointers of the instance, in slab order; P: the plan of the largest frame
void orb_bind(sslam_orb* o, const OrbPlan& P, sslam::Slab& S) {
    const size_t nc = (size_t)o->cap, sb = (size_t)std::max(P.slab_bytes, 256LL);
    o->img = S.take<uint8_t>(sb);
    o->blur = S.take<uint8_t>(sb);
    o->cand_xy = S.take<uint32_t>(nc);
    o->cand_score = S.take<uint32_t>(nc);
    o->cand_key = S.take<uint32_t>(nc);
    o->skey = S.take<unsigned long long>(nc);
    o->ctl = S.take<OrbCtl>(1);
    o->pattern = S.take<int8_t>(2 * ORB_PATTERN_POINTS);
    o->xy = S.take<float>(2 * nc);
    o->aux = S.take<float>(4 * nc);
    o->desc = S.take<uint8_t>(32 * nc);
    o->n = S.take<int32_t>(1);
}

int orb_enqueue(sslam_orb* o, const uint8_t* img_dev, int h, int w, int c, float* xy, float* aux, uint8_t* desc, int32_t* n_out) {
    const OrbPlan P = orb_plan(o->p, w, h);
    o->plan = P; o->have_plan = true;
    hipStream_t s = o->ctx->stream;
    (void)hipGetLastError();
    SSLAM_HIP_CHECK(hipMemsetAsync(o->ctl, 0, sizeof(OrbCtl), s));
    if (P.nactive == 0) {                                      // no level can hold a keypoint
        SSLAM_HIP_CHECK(hipMemsetAsync(n_out, 0, sizeof(int32_t), s));
        return 0;
    }
    OrbArgs a{};
    a.nactive = P.nactive; a.border = P.border; a.edge = o->p.edge_threshold; a.score_type = o->p.score_type;
    a.fast_t = o->p.fast_threshold; a.fast_tiles = P.fast_tiles; a.blur_tiles = P.blur_tiles;
    for (int l = 0; l < P.nactive; ++l) {
        const OrbLevel& L = P.lv[l];
        a.lv[l] = OrbLevelDev{L.w, L.h, L.stride, L.rows, L.quota, L.cut1_n, L.fast_tx, L.fast_base, L.pad_tx, L.pad_base,
                              L.cand_cap, (uint32_t)L.cand_off, L.off, L.scale};
    }
    for (int v = 0; v <= ORB_HALF; ++v) a.umax4 |= (unsigned long long)P.umax[v] << (4 * v);
    for (int i = 0; i < 7; ++i) a.gauss[i] = P.gauss[i];
    a.harris_k = P.harris_k; a.harris_scale4 = P.harris_scale4; a.atan = P.atan; a.patch_size = P.patch_size;
    a.img = o->img; a.blur = o->blur; a.cand_xy = o->cand_xy; a.cand_score = o->cand_score; a.cand_key = o->cand_key; a.skey = o->skey;
    a.ctl = o->ctl; a.pattern = o->pattern; a.xy_out = xy; a.aux_out = aux; a.desc_out = desc; a.n_out = n_out;
    for (int l = 0; l < P.nactive; ++l)
        hipLaunchKernelGGL(orb_level_kernel, dim3(cdiv(P.lv[l].stride, 64), cdiv(P.lv[l].rows, ORB_T / 64)), dim3(ORB_T), 0, s, a, l, img_dev, c);
    hipLaunchKernelGGL(orb_fast_kernel, dim3(P.fast_tiles), dim3(ORB_T), 0, s, a);
    hipLaunchKernelGGL(orb_blur_kernel, dim3(P.blur_tiles), dim3(ORB_T), 0, s, a);
    hipLaunchKernelGGL(orb_response_kernel, dim3(ORB_RESP_GX, P.nactive), dim3(ORB_T), 0, s, a);
    hipLaunchKernelGGL(orb_select_kernel, dim3(P.nactive), dim3(ORB_SEL_T), 0, s, a);
    hipLaunchKernelGGL(orb_describe_kernel, dim3(ORB_DESC_GX, P.nactive), dim3(ORB_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int sslam_orb_create(sslam_ctx* ctx, int max_w, int max_h, int nfeatures, double scale_factor, int nlevels,
                                int edge_threshold, int score_type, int fast_threshold, const int8_t* pattern_or_null,
                                sslam_orb** out) {
    const char* who = "sslam_orb_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    OrbParams p;
    p.nfeatures = nfeatures; p.scale_factor = scale_factor; p.nlevels = nlevels; p.edge_threshold = edge_threshold;
    p.score_type = score_type; p.fast_threshold = fast_threshold;
    char msg[160];
    if (orb_check_params(p, max_w, max_h, msg, sizeof msg)) { sslam::set_error("%s: %s", who, msg); return 2; }
    int8_t pat[2 * ORB_PATTERN_POINTS];
    if (pattern_or_null) {
        if (orb_check_pattern(pattern_or_null, msg, sizeof msg)) { sslam::set_error("%s: %s", who, msg); return 2; }
        std::memcpy(pat, pattern_or_null, sizeof pat);
    } else {
        orb_default_pattern(pat);
    }
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_orb> o(new sslam_orb);
    o->ctx = ctx; o->p = p; o->max_w = max_w; o->max_h = max_h;
    const OrbPlan P = orb_plan(p, max_w, max_h);
    o->cap = orb_capacity(p, max_w, max_h);
    if (int rc = o->slab.alloc(who, false, [&](sslam::Slab& S) { orb_bind(o.get(), P, S); })) return rc;
    if (const hipError_t e = hipMemcpy(o->pattern, pat, sizeof pat, hipMemcpyHostToDevice); e != hipSuccess) {
        sslam::set_error("%s: pattern upload: %s", who, hipGetErrorString(e));
        return 1;
    }
    sslam::ctx_retain(ctx);
    *out = o.release();
    return 0;
}

extern "C" int sslam_orb_destroy(sslam_orb* o) {
    return sslam::destroy_instance(o);
}

extern "C" int sslam_orb_capacity(sslam_orb* o, int* cap) {
    const char* who = "sslam_orb_capacity";
    SSLAM_REQUIRE(o != nullptr && cap != nullptr, "%s: NULL argument", who);
    *cap = (int)o->cap;
    return 0;
}

extern "C" int sslam_orb_default_pattern(int8_t* pattern_out) {
    SSLAM_REQUIRE(pattern_out != nullptr, "sslam_orb_default_pattern: pattern_out is NULL");
    orb_default_pattern(pattern_out);
    return 0;
}

extern "C" int sslam_orb_detect_dev(sslam_orb* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev,
                                    float* aux_out_dev, uint8_t* desc_out_dev, int32_t* n_out_dev) {
    const char* who = "sslam_orb_detect_dev";
    if (int rc = feat_check_call(who, o, img_dev, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out_dev && aux_out_dev && desc_out_dev && n_out_dev, "%s: an output pointer is NULL", who);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    return orb_enqueue(o, img_dev, h, w, c, xy_out_dev, aux_out_dev, desc_out_dev, n_out_dev);
}

extern "C" int sslam_orb_detect_host(sslam_orb* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out,
                                     uint8_t* desc_out, int32_t* n_out) {
    const char* who = "sslam_orb_detect_host";
    if (int rc = feat_check_call(who, o, img, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out && aux_out && desc_out && n_out, "%s: an output pointer is NULL", who);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    const uint8_t* img_dev;
    if (int rc = feat_stage_image(o->ctx, img, h, w, c, &img_dev)) return rc;
    if (int rc = orb_enqueue(o, img_dev, h, w, c, o->xy, o->aux, o->desc, o->n)) return rc;
    hipStream_t s = o->ctx->stream;
    // the count and the rows a call without ties can fill come down behind the kernels: one synchronisation.  Only a call
    // whose ties exceed that fetches the rest.  (ORB has no capacities to void a frame on and knows its likely count in advance:
    // this is why its tail is not feat_host.hpp's feat_detect_host, which reads the count first and fetches the rows after.)
    const size_t first = (size_t)std::min<long long>(o->cap, (long long)o->p.nfeatures + 64);
    int32_t n = 0;
    SSLAM_HIP_CHECK(sslam::copy_down(s, &n, o->n, 1));
    SSLAM_HIP_CHECK(sslam::copy_down(s, xy_out, o->xy, first * 2));
    SSLAM_HIP_CHECK(sslam::copy_down(s, aux_out, o->aux, first * 4));
    SSLAM_HIP_CHECK(sslam::copy_down(s, desc_out, o->desc, first * 32));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if ((size_t)n > first) {
        const size_t more = (size_t)n - first;
        SSLAM_HIP_CHECK(sslam::copy_down(s, xy_out + first * 2, o->xy + first * 2, more * 2));
        SSLAM_HIP_CHECK(sslam::copy_down(s, aux_out + first * 4, o->aux + first * 4, more * 4));
        SSLAM_HIP_CHECK(sslam::copy_down(s, desc_out + first * 32, o->desc + first * 32, more * 32));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    *n_out = n;
    return 0;
}

extern "C" int sslam_orb_level_info(sslam_orb* o, int level, int* info8) {
    const char* who = "sslam_orb_level_info";
    SSLAM_REQUIRE(o != nullptr && info8 != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(o->have_plan, "%s: no frame has been processed", who);
    SSLAM_REQUIRE(level >= 0 && level < o->plan.nlevels, "%s: level %d outside 0..%d", who, level, o->plan.nlevels - 1);
    const OrbLevel& L = o->plan.lv[level];
    const int v[8] = {L.w, L.h, L.active ? L.stride : 0, L.active ? L.rows : 0, L.active, L.quota, L.active ? L.cand_cap : 0, o->plan.border};
    for (int i = 0; i < 8; ++i) info8[i] = v[i];
    return 0;
}

extern "C" int sslam_orb_stage_read(sslam_orb* o, int level, uint8_t* img, uint8_t* blur, int32_t* cand, int32_t* ncand,
                                    int32_t* cuts) {
    const char* who = "sslam_orb_stage_read";
    SSLAM_REQUIRE(o != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(o->have_plan, "%s: no frame has been processed", who);
    SSLAM_REQUIRE(level >= 0 && level < o->plan.nactive, "%s: level %d is not among the %d stored levels", who, level, o->plan.nactive);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    const OrbLevel& L = o->plan.lv[level];
    hipStream_t s = o->ctx->stream;
    const size_t np = (size_t)L.stride * L.rows;
    if (img) SSLAM_HIP_CHECK(hipMemcpyAsync(img, o->img + L.off, np, hipMemcpyDeviceToHost, s));
    if (blur) SSLAM_HIP_CHECK(hipMemcpyAsync(blur, o->blur + L.off, np, hipMemcpyDeviceToHost, s));
    OrbCtl ctl;
    SSLAM_HIP_CHECK(hipMemcpyAsync(&ctl, o->ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const int n = std::min(ctl.ncand[level], L.cand_cap);
    if (ncand) *ncand = n;
    if (cuts) { cuts[0] = ctl.cut1[level]; cuts[1] = (int32_t)ctl.cut2[level]; }
    if (cand && n > 0) {
        std::vector<uint32_t> xy(n), sc(n), key(n);
        SSLAM_HIP_CHECK(hipMemcpyAsync(xy.data(), o->cand_xy + L.cand_off, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipMemcpyAsync(sc.data(), o->cand_score + L.cand_off, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipMemcpyAsync(key.data(), o->cand_key + L.cand_off, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
        for (int i = 0; i < n; ++i) {
            cand[4 * i] = (int32_t)(xy[i] & 0xffffu); cand[4 * i + 1] = (int32_t)(xy[i] >> 16); cand[4 * i + 2] = (int32_t)sc[i];
            const uint32_t k = key[i];
            cand[4 * i + 3] = (int32_t)(k == 0 ? 0x7fc00000u : ((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k));
        }
    }
    return 0;
}
