// klt_kernels.hip - pyramidal Lucas-Kanade: the per-frame pyramid and the per-point tracker.
//
// Replaces `cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)` and `cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize, maxLevel,
// criteria, flags, minEigThreshold)` for 8-bit images as the KLT front end calls them (slam/monocular/main4.py:396-433), and the
// forward-backward gate between its two calls.  Kernels:
//   * klt_gray_kernel        per frame, a pixel per lane: fixed-point B 3735 + G 19235 + R 9798, + 2^14, >> 15 (one channel: a
//                            copy) into the interior of padded level 0.
//   * klt_down_kernel        per level, an output pixel per lane: pyrDown's [1 4 6 4 1] x [1 4 6 4 1], (sum + 128) >> 8,
//                            reflect-101 by index arithmetic on the level below's INTERIOR.
//   * klt_ring_deriv_kernel  per level, a pixel of the padded level per lane.  Interior: the unscaled Scharr pair (dx, dy) as one
//                            int16x2 record, reflect-101 at the edge.  Ring (winSize wide on each side): the reflect-101 copy of
//                            the interior into the level, zeros into the derivative record (OpenCV pads it BORDER_CONSTANT).  It
//                            reads interior pixels only and writes ring pixels and records only, so one launch does both.
//   * klt_track_kernel       a point per wavefront, four per block, all levels inside.  Lanes stride over the window; the I / Ix /
//                            Iy patch of the level sits in LDS as int16 (a lane reads back only what it wrote: no barrier); the
//                            integer sums are per-lane int64, reduced over the 64 lanes by xor shuffles (every lane ends with the
//                            same exact total) and converted to float32 once, through float64, which holds them exactly.  The
//                            float tail is computed by every lane alike, one IEEE operation at a time (contraction is off for
//                            the whole file; sqrt and the divisions go through float64, which rounds to the correctly rounded
//                            float32 result whatever the compiler's division mode), in the order of tests/klt_ref.py.
//   * klt_gate_kernel        one block: status / err / forward-backward masks, the five counters, and the kept pairs compacted in
//                            point order (ballot + a running base).
// MEMORY SAFETY: a patch load at integer origin i touches i .. i + win inclusive; every level is stored padded by win on each
// side, so any i in [-win, size - 1] stays inside it.  `klt_inside` is that test, written on the float so that NaN, inf and
// values outside int range fail it, and it precedes every load; the float -> int conversion happens only after it passed.
// All loops are bounded: levels <= KLT_MAX_LEVELS, iterations <= 100, window elements <= 31 x 31.
// PARITY UNPINNED: cv2 is absent here; tests/klt_ref.py restates the functions and names what could not be confirmed.
#include "common.hpp"
#include "feat_device.hpp"
#include "feat_host.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int KLT_MAX_SIDE = sslam::FEAT_MAX_SIDE;
constexpr int KLT_MAX_POINTS = 1 << 20;
constexpr int KLT_MIN_WIN = 3, KLT_MAX_WIN = 31;         // odd sides; 31 x 31 x 3 int16 per wave is the LDS patch
constexpr int KLT_MAX_ELEMS = KLT_MAX_WIN * KLT_MAX_WIN;
constexpr int KLT_MAX_LEVELS = 11;                       // maxLevel 0..10
constexpr int KLT_T = 256, KLT_WAVES = KLT_T / 64;
constexpr int KLT_USE_INITIAL_FLOW = 4, KLT_GET_MIN_EIGENVALS = 8;
constexpr int KLT_W_BITS = 14;

struct KltLevel {
    uint8_t* img = nullptr;      // [(h + 2 ph)][(w + 2 pw)], the image at (ph, pw)
    uint32_t* der = nullptr;     // same layout, one record per pixel: dx in the low half, dy in the high half (int16 each)
    int w = 0, h = 0;
};

struct KltFrame {
    KltLevel lv[KLT_MAX_LEVELS];
    int top = -1;                // the last level built (the effective maxLevel); -1: no frame yet
};

}  // namespace

struct sslam_klt {
    sslam_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0, max_points = 0, ww = 0, wh = 0, max_level = 0;
    KltFrame fr[2];
    int cur = 0;                 // fr[cur] is the current frame, fr[cur ^ 1] the previous one
    sslam::OwnedSlab slab;
    // workspace of the host entries and of the fused stage, each [max_points]
    float *prev = nullptr, *init = nullptr, *next = nullptr, *back = nullptr, *err = nullptr, *err_back = nullptr;
    float *pts0 = nullptr, *pts1 = nullptr;
    uint8_t *status = nullptr, *st_back = nullptr, *mask = nullptr;
    int* counts = nullptr;       // [5]
};

namespace {

__global__ __launch_bounds__(KLT_T)
void klt_gray_kernel(const uint8_t* __restrict__ src, int h, int w, int C, uint8_t* __restrict__ dst, int stride) {
    const size_t p = (size_t)blockIdx.x * KLT_T + threadIdx.x;
    if (p >= (size_t)h * w) return;
    const int y = (int)(p / (size_t)w), x = (int)(p % (size_t)w);
    dst[(size_t)y * stride + x] = (uint8_t)sslam::bgr_to_grey(src + p * (size_t)C, C);
}

// src / dst: the interiors (pointer to pixel (0, 0)) of two padded levels
__global__ __launch_bounds__(KLT_T)
void klt_down_kernel(const uint8_t* __restrict__ src, int sh, int sw, int sstride, uint8_t* __restrict__ dst, int dh, int dw,
                     int dstride) {
    const size_t p = (size_t)blockIdx.x * KLT_T + threadIdx.x;
    if (p >= (size_t)dh * dw) return;
    const int y = (int)(p / (size_t)dw), x = (int)(p % (size_t)dw);
    const int k[5] = {1, 4, 6, 4, 1};
    int cx[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) cx[i] = sslam::reflect101(2 * x - 2 + i, sw);
    int sum = 128;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* r = src + (size_t)sslam::reflect101(2 * y - 2 + j, sh) * sstride;
        int row = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) row += k[i] * (int)r[cx[i]];
        sum += k[j] * row;
    }
    dst[(size_t)y * dstride + x] = (uint8_t)(sum >> 8);
}

__global__ __launch_bounds__(KLT_T)
void klt_ring_deriv_kernel(uint8_t* __restrict__ img, uint32_t* __restrict__ der, int h, int w, int pw, int ph) {
    const int stride = w + 2 * pw;
    const size_t p = (size_t)blockIdx.x * KLT_T + threadIdx.x;
    if (p >= (size_t)stride * (h + 2 * ph)) return;
    const int y = (int)(p / (size_t)stride) - ph, x = (int)(p % (size_t)stride) - pw;
    const uint8_t* in = img + (size_t)ph * stride + pw;                      // pixel (0, 0)
    if (y >= 0 && y < h && x >= 0 && x < w) {
        const int ym = sslam::reflect101(y - 1, h), yp = sslam::reflect101(y + 1, h);
        const int xm = sslam::reflect101(x - 1, w), xp = sslam::reflect101(x + 1, w);
        const uint8_t* r0 = in + (size_t)ym * stride;
        const uint8_t* r1 = in + (size_t)y * stride;
        const uint8_t* r2 = in + (size_t)yp * stride;
        const int a = r0[xm], b = r0[x], c = r0[xp], d = r1[xm], f = r1[xp], g = r2[xm], hh = r2[x], i = r2[xp];
        const int dx = 3 * (c - a) + 10 * (f - d) + 3 * (i - g);
        const int dy = 3 * (g - a) + 10 * (hh - b) + 3 * (i - c);
        der[p] = (uint32_t)(uint16_t)(int16_t)dx | ((uint32_t)(uint16_t)(int16_t)dy << 16);
    } else {
        img[p] = in[(size_t)sslam::reflect101(y, h) * stride + sslam::reflect101(x, w)];
        der[p] = 0u;
    }
}

struct KltTrackArgs {
    KltLevel I[KLT_MAX_LEVELS], J[KLT_MAX_LEVELS];
    int top, n, ww, wh, flags, max_count;
    double eps2, min_eig;
    const float* prev;           // [n][2]
    const float* init;           // [n][2], read under KLT_USE_INITIAL_FLOW
    float* next;                 // [n][2]
    uint8_t* status;             // [n]
    float* err;                  // [n]
};

struct KltTap { int ix, iy, w00, w01, w10, w11; };

// the bounds test on floor(f): not (< -win or >= size).  NaN, +-inf and anything outside int range fail it.
__device__ __forceinline__ bool klt_inside(float fx, float fy, int w, int h, int ww, int wh) {
    return fx >= -(float)ww && fx < (float)w && fy >= -(float)wh && fy < (float)h;
}

// of a position that passed klt_inside
__device__ __forceinline__ KltTap klt_tap(float fx, float fy) {
    const float flx = floorf(fx), fly = floorf(fy);
    const float a = fx - flx, b = fy - fly;
    const float sc = (float)(1 << KLT_W_BITS);
    KltTap t;
    t.ix = (int)flx; t.iy = (int)fly;
    t.w00 = (int)rintf((1.0f - a) * (1.0f - b) * sc);
    t.w01 = (int)rintf(a * (1.0f - b) * sc);
    t.w10 = (int)rintf((1.0f - a) * b * sc);
    t.w11 = (1 << KLT_W_BITS) - t.w00 - t.w01 - t.w10;
    return t;
}

// (x, y) += 64 window elements, in row-major order of a window ww wide (step_x < ww: one carry at most)
__device__ __forceinline__ void klt_next(int& x, int& y, int step_x, int step_y, int ww) {
    x += step_x; y += step_y;
    if (x >= ww) { x -= ww; ++y; }
}

__device__ __forceinline__ int klt_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// an exact integer below 2^53 -> float32, one rounding
__device__ __forceinline__ float klt_to_float(long long s) { return (float)(double)s; }
// correctly rounded float32 quotient and square root (float64 carries enough bits for the second rounding to be harmless)
__device__ __forceinline__ float klt_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float klt_sqrt(float a) { return (float)sqrt((double)a); }

// the J sample of window element (x, y) at tap t, CV_DESCALE(.., W_BITS - 5)
__device__ __forceinline__ int klt_sample_img(const KltLevel& L, int pw, int ph, const KltTap& t, int x, int y) {
    const int stride = L.w + 2 * pw;
    const uint8_t* r0 = L.img + (size_t)(t.iy + ph + y) * stride + (t.ix + pw + x);
    const uint8_t* r1 = r0 + stride;
    return klt_descale((int)r0[0] * t.w00 + (int)r0[1] * t.w01 + (int)r1[0] * t.w10 + (int)r1[1] * t.w11, KLT_W_BITS - 5);
}

// (no packed fp32: the build's ISA guard named this kernel - the vectoriser paired the x / y halves of the float tail into the
//  op_sel form that isa_guard.py bars; see al_aggregate_kernel in aliked_kernels.hip)
__attribute__((target("no-packed-fp32-ops")))
__global__ __launch_bounds__(KLT_T) void klt_track_kernel(KltTrackArgs a) {
    __shared__ int16_t s_pat[KLT_WAVES][3][KLT_MAX_ELEMS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * KLT_WAVES + wave;
    if (p >= a.n) return;                                // (per wave: the kernel has no block barrier)
    int16_t* sI = s_pat[wave][0];
    int16_t* sIx = s_pat[wave][1];
    int16_t* sIy = s_pat[wave][2];
    const int ww = a.ww, wh = a.wh, ne = ww * wh;
    // window element e = y ww + x of this lane: e = lane, lane + 64, ...; the step of 64 elements as (step_y rows, step_x columns)
    const int step_y = 64 / ww, step_x = 64 - step_y * ww;
    const int y0 = lane / ww, x0 = lane - y0 * ww;
    const float halfx = (float)(ww - 1) * 0.5f, halfy = (float)(wh - 1) * 0.5f;
    const float FLT_SCALE = 1.0f / (float)(1 << 20), EPS = 1.1920929e-07f;
    const float den_eig = (float)(2 * ww * wh), den_err = (float)(32 * ww * wh);
    const float ptx = a.prev[2 * (size_t)p], pty = a.prev[2 * (size_t)p + 1];
    float nx = 0.0f, ny = 0.0f, err = 0.0f;
    int status = 1;
    for (int level = a.top; level >= 0; --level) {
        const KltLevel LI = a.I[level], LJ = a.J[level];
        const float scale = ldexpf(1.0f, -level);
        const float px = ptx * scale, py = pty * scale;
        if (level == a.top) {
            if (a.flags & KLT_USE_INITIAL_FLOW) {
                nx = a.init[2 * (size_t)p] * scale; ny = a.init[2 * (size_t)p + 1] * scale;
            } else {
                nx = px; ny = py;
            }
        } else {
            nx = nx * 2.0f; ny = ny * 2.0f;
        }
        const float fx = px - halfx, fy = py - halfy;
        if (!klt_inside(fx, fy, LI.w, LI.h, ww, wh)) {
            if (level == 0) { status = 0; err = 0.0f; }
            continue;
        }
        {   // the I / Ix / Iy patch and the three sums of the gradient matrix
            const KltTap t = klt_tap(fx, fy);
            const int stride = LI.w + 2 * ww;
            long long s11 = 0, s12 = 0, s22 = 0;
            for (int e = lane, x = x0, y = y0; e < ne; e += 64, klt_next(x, y, step_x, step_y, ww)) {
                const size_t o = (size_t)(t.iy + wh + y) * stride + (t.ix + ww + x);
                const uint8_t* r0 = LI.img + o;
                const uint8_t* r1 = r0 + stride;
                const int iv = klt_descale((int)r0[0] * t.w00 + (int)r0[1] * t.w01 + (int)r1[0] * t.w10 + (int)r1[1] * t.w11,
                                           KLT_W_BITS - 5);
                const uint32_t d00 = LI.der[o], d01 = LI.der[o + 1], d10 = LI.der[o + stride], d11 = LI.der[o + stride + 1];
                const int ixv = klt_descale((int)(int16_t)(d00 & 0xffffu) * t.w00 + (int)(int16_t)(d01 & 0xffffu) * t.w01
                                            + (int)(int16_t)(d10 & 0xffffu) * t.w10 + (int)(int16_t)(d11 & 0xffffu) * t.w11, KLT_W_BITS);
                const int iyv = klt_descale((int)(int16_t)(d00 >> 16) * t.w00 + (int)(int16_t)(d01 >> 16) * t.w01
                                            + (int)(int16_t)(d10 >> 16) * t.w10 + (int)(int16_t)(d11 >> 16) * t.w11, KLT_W_BITS);
                sI[e] = (int16_t)iv; sIx[e] = (int16_t)ixv; sIy[e] = (int16_t)iyv;
                s11 += (long long)(ixv * ixv); s12 += (long long)(ixv * iyv); s22 += (long long)(iyv * iyv);
            }
            s11 = sslam::wave_sum(s11); s12 = sslam::wave_sum(s12); s22 = sslam::wave_sum(s22);
            const float A11 = klt_to_float(s11) * FLT_SCALE, A12 = klt_to_float(s12) * FLT_SCALE, A22 = klt_to_float(s22) * FLT_SCALE;
            const float D = A11 * A22 - A12 * A12;
            const float dif = A11 - A22;
            const float root = klt_sqrt(dif * dif + 4.0f * A12 * A12);
            const float min_eig = klt_div(A22 + A11 - root, den_eig);
            if (a.flags & KLT_GET_MIN_EIGENVALS) err = min_eig;
            if ((double)min_eig < a.min_eig || D < EPS) {
                if (level == 0) status = 0;
                continue;
            }
            const float Dinv = klt_div(1.0f, D);
            float cx = nx - halfx, cy = ny - halfy;      // nextPt in window-corner form
            float pdx = 0.0f, pdy = 0.0f;
            for (int j = 0; j < a.max_count; ++j) {
                if (!klt_inside(cx, cy, LJ.w, LJ.h, ww, wh)) {
                    if (level == 0) status = 0;
                    break;
                }
                const KltTap u = klt_tap(cx, cy);
                long long sb1 = 0, sb2 = 0;
                for (int e = lane, x = x0, y = y0; e < ne; e += 64, klt_next(x, y, step_x, step_y, ww)) {
                    const int diff = klt_sample_img(LJ, ww, wh, u, x, y) - (int)sI[e];
                    sb1 += (long long)(diff * (int)sIx[e]); sb2 += (long long)(diff * (int)sIy[e]);
                }
                sb1 = sslam::wave_sum(sb1); sb2 = sslam::wave_sum(sb2);
                const float b1 = klt_to_float(sb1) * FLT_SCALE, b2 = klt_to_float(sb2) * FLT_SCALE;
                const float dx = (A12 * b2 - A22 * b1) * Dinv, dy = (A12 * b1 - A11 * b2) * Dinv;
                cx = cx + dx; cy = cy + dy;
                nx = cx + halfx; ny = cy + halfy;
                if ((double)dx * (double)dx + (double)dy * (double)dy <= a.eps2) break;
                if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                    nx = nx - dx * 0.5f; ny = ny - dy * 0.5f;
                    break;
                }
                pdx = dx; pdy = dy;
            }
            if (level == 0 && status && !(a.flags & KLT_GET_MIN_EIGENVALS)) {
                const float ex = nx - halfx, ey = ny - halfy;
                if (!klt_inside(ex, ey, LJ.w, LJ.h, ww, wh)) {
                    status = 0;
                } else {
                    const KltTap u = klt_tap(ex, ey);
                    long long se = 0;
                    for (int e = lane, x = x0, y = y0; e < ne; e += 64, klt_next(x, y, step_x, step_y, ww)) {
                        const int diff = klt_sample_img(LJ, ww, wh, u, x, y) - (int)sI[e];
                        se += (long long)(diff < 0 ? -diff : diff);
                    }
                    se = sslam::wave_sum(se);
                    err = klt_div(klt_to_float(se), den_err);
                }
            }
        }
    }
    if (lane == 0) {
        a.next[2 * (size_t)p] = nx; a.next[2 * (size_t)p + 1] = ny;
        a.status[p] = (uint8_t)status;
        a.err[p] = err;
    }
}

// mask bits per point
constexpr int KLT_M_STATUS = 1, KLT_M_ERR = 2, KLT_M_FB = 4, KLT_M_KEPT = 8;

__global__ __launch_bounds__(KLT_T)
void klt_gate_kernel(int n, const float* __restrict__ prev, const float* __restrict__ next, const float* __restrict__ back,
                     const uint8_t* __restrict__ st, const float* __restrict__ err, const uint8_t* __restrict__ stb, float err_thr,
                     float fb_thr, float* __restrict__ pts0, float* __restrict__ pts1, int* __restrict__ counts,
                     uint8_t* __restrict__ mask) {
    __shared__ int s_wave[KLT_WAVES];
    __shared__ int s_cnt[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    int base = 0;                                        // pairs kept before this chunk (the same in every thread)
    for (int c0 = 0; c0 < n; c0 += KLT_T) {              // (n is uniform: every thread runs every chunk and meets both barriers)
        const int i = c0 + threadIdx.x;
        bool s = false, e = false, f = false;
        float p0x = 0, p0y = 0, p1x = 0, p1y = 0;
        if (i < n) {
            p0x = prev[2 * (size_t)i]; p0y = prev[2 * (size_t)i + 1];
            p1x = next[2 * (size_t)i]; p1y = next[2 * (size_t)i + 1];
            s = st[i] == 1;
            e = err[i] < err_thr;
            const float dx = back[2 * (size_t)i] - p0x, dy = back[2 * (size_t)i + 1] - p0y;
            f = stb[i] == 1 && klt_sqrt(dx * dx + dy * dy) < fb_thr;
        }
        const bool keep = s && e && f;
        const unsigned long long bs = __ballot(s), be = __ballot(s && e), bk = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(bk);
        __syncthreads();
        int before = __popcll(bk & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
        for (int w = 0; w < KLT_WAVES; ++w) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (lane == 0) { atomicAdd(&s_cnt[0], __popcll(bs)); atomicAdd(&s_cnt[1], __popcll(be)); atomicAdd(&s_cnt[2], __popcll(bk)); }
        if (i < n) {
            if (keep) {
                const size_t o = 2 * (size_t)(base + before);
                pts0[o] = p0x; pts0[o + 1] = p0y; pts1[o] = p1x; pts1[o + 1] = p1y;
            }
            if (mask) mask[i] = (uint8_t)((s ? KLT_M_STATUS : 0) | (e ? KLT_M_ERR : 0) | (f ? KLT_M_FB : 0) | (keep ? KLT_M_KEPT : 0));
        }
        base += total;
        __syncthreads();                                 // s_wave is rewritten by the next chunk
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[0] = n; counts[1] = s_cnt[0]; counts[2] = s_cnt[1]; counts[3] = s_cnt[2]; counts[4] = s_cnt[2];
    }
}

unsigned klt_blocks(size_t threads) { return (unsigned)((threads + KLT_T - 1) / KLT_T); }

size_t klt_padded(const sslam_klt* k, int w, int h) { return (size_t)(w + 2 * k->ww) * (h + 2 * k->wh); }

uint8_t* klt_interior(const sslam_klt* k, const KltLevel& L) { return L.img + (size_t)k->wh * (L.w + 2 * k->ww) + k->ww; }

// the slab-backed pointers of the instance, in slab order
void klt_bind(sslam_klt* k, sslam::Slab& S) {
    for (int f = 0; f < 2; ++f) {
        int w = k->max_w, h = k->max_h;
        for (int l = 0; l <= k->max_level; ++l) {        // (every level up to maxLevel at the largest size: the stop rule is per frame)
            k->fr[f].lv[l].img = S.take<uint8_t>(klt_padded(k, w, h));
            k->fr[f].lv[l].der = S.take<uint32_t>(klt_padded(k, w, h));
            w = (w + 1) / 2; h = (h + 1) / 2;
        }
    }
    const size_t np = (size_t)k->max_points;
    k->prev = S.take<float>(2 * np); k->init = S.take<float>(2 * np); k->next = S.take<float>(2 * np);
    k->back = S.take<float>(2 * np); k->pts0 = S.take<float>(2 * np); k->pts1 = S.take<float>(2 * np);
    k->err = S.take<float>(np); k->err_back = S.take<float>(np);
    k->status = S.take<uint8_t>(np); k->st_back = S.take<uint8_t>(np); k->mask = S.take<uint8_t>(np);
    k->counts = S.take<int>(5);
}

int klt_check_image(const char* who, sslam_klt* k, const uint8_t* img, int h, int w, int c) {
    SSLAM_REQUIRE(k != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(img != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(c == 1 || c == 3 || c == 4, "%s: %d channels (want 1, 3 or 4)", who, c);
    SSLAM_REQUIRE(w >= 1 && w <= k->max_w && h >= 1 && h <= k->max_h, "%s: frame size %dx%d outside 1..%dx%d (the instance's maximum)",
                  who, w, h, k->max_w, k->max_h);
    return 0;
}

// the frame at device address `img` -> the pyramid of the slot that becomes "current"
int klt_enqueue_push(sslam_klt* k, const uint8_t* img, int h, int w, int c) {
    hipStream_t s = k->ctx->stream;
    KltFrame& F = k->fr[k->cur ^ 1];
    F.top = -1;
    int top = 0;
    F.lv[0].w = w; F.lv[0].h = h;
    for (int l = 1; l <= k->max_level; ++l) {            // buildOpticalFlowPyramid's stop rule
        const int lw = (F.lv[l - 1].w + 1) / 2, lh = (F.lv[l - 1].h + 1) / 2;
        if (lw <= k->ww || lh <= k->wh) break;
        F.lv[l].w = lw; F.lv[l].h = lh;
        top = l;
    }
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    hipLaunchKernelGGL(klt_gray_kernel, dim3(klt_blocks((size_t)h * w)), dim3(KLT_T), 0, s, img, h, w, c, klt_interior(k, F.lv[0]),
                       w + 2 * k->ww);
    for (int l = 0; l <= top; ++l) {
        const KltLevel& L = F.lv[l];
        if (l < top) {
            const KltLevel& N = F.lv[l + 1];
            hipLaunchKernelGGL(klt_down_kernel, dim3(klt_blocks((size_t)N.h * N.w)), dim3(KLT_T), 0, s, klt_interior(k, L), L.h, L.w,
                               L.w + 2 * k->ww, klt_interior(k, N), N.h, N.w, N.w + 2 * k->ww);
        }
        hipLaunchKernelGGL(klt_ring_deriv_kernel, dim3(klt_blocks(klt_padded(k, L.w, L.h))), dim3(KLT_T), 0, s, L.img, L.der, L.h, L.w,
                           k->ww, k->wh);
    }
    SSLAM_HIP_CHECK(hipGetLastError());
    F.top = top;
    k->cur ^= 1;
    return 0;
}

int klt_criteria(const char* who, int type, int max_count, double epsilon, double min_eig, int* count, double* eps2) {
    SSLAM_REQUIRE(std::isfinite(epsilon) && std::isfinite(min_eig), "%s: epsilon / minEigThreshold is not finite", who);
    *count = (type & 1) ? (max_count < 0 ? 0 : max_count > 100 ? 100 : max_count) : 30;
    const double e = (type & 2) ? (epsilon < 0 ? 0.0 : epsilon > 10 ? 10.0 : epsilon) : 0.01;
    *eps2 = e * e;
    return 0;
}

int klt_check_track(const char* who, sslam_klt* k, int n) {
    SSLAM_REQUIRE(k != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(n >= 1 && n <= k->max_points, "%s: %d points outside 1..%d (the instance's capacity)", who, n, k->max_points);
    const KltFrame &A = k->fr[0], &B = k->fr[1];
    SSLAM_REQUIRE(A.top >= 0 && B.top >= 0, "%s: needs two pushed frames", who);
    SSLAM_REQUIRE(A.lv[0].w == B.lv[0].w && A.lv[0].h == B.lv[0].h, "%s: the two frames differ in size (%dx%d and %dx%d)", who,
                  A.lv[0].w, A.lv[0].h, B.lv[0].w, B.lv[0].h);
    return 0;
}

int klt_enqueue_track(sslam_klt* k, int reverse, int n, const float* prev, const float* init, int flags, int max_count, double eps2,
                      double min_eig, float* next, uint8_t* status, float* err) {
    const KltFrame& I = k->fr[reverse ? k->cur : k->cur ^ 1];
    const KltFrame& J = k->fr[reverse ? k->cur ^ 1 : k->cur];
    KltTrackArgs a{};
    a.top = I.top < J.top ? I.top : J.top;
    for (int l = 0; l <= a.top; ++l) { a.I[l] = I.lv[l]; a.J[l] = J.lv[l]; }
    a.n = n; a.ww = k->ww; a.wh = k->wh; a.flags = flags; a.max_count = max_count; a.eps2 = eps2; a.min_eig = min_eig;
    a.prev = prev; a.init = init; a.next = next; a.status = status; a.err = err;
    (void)hipGetLastError();
    hipLaunchKernelGGL(klt_track_kernel, dim3((unsigned)sslam::cdiv(n, KLT_WAVES)), dim3(KLT_T), 0, k->ctx->stream, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

// forward, backward from the forward result, gate: three launches, nothing returns to the host in between
int klt_enqueue_fb(sslam_klt* k, int n, const float* prev, int max_count, double eps2, double min_eig, double err_thresh,
                   double fb_thresh, float* next, float* pts0, float* pts1, int* counts, uint8_t* mask) {
    if (int rc = klt_enqueue_track(k, 0, n, prev, nullptr, 0, max_count, eps2, min_eig, next, k->status, k->err)) return rc;
    if (int rc = klt_enqueue_track(k, 1, n, next, nullptr, 0, max_count, eps2, min_eig, k->back, k->st_back, k->err_back)) return rc;
    hipLaunchKernelGGL(klt_gate_kernel, dim3(1), dim3(KLT_T), 0, k->ctx->stream, n, prev, (const float*)next, (const float*)k->back,
                       (const uint8_t*)k->status, (const float*)k->err, (const uint8_t*)k->st_back, (float)err_thresh, (float)fb_thresh,
                       pts0, pts1, counts, mask);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

int klt_check_flags(const char* who, int flags, const void* init) {
    SSLAM_REQUIRE((flags & ~(KLT_USE_INITIAL_FLOW | KLT_GET_MIN_EIGENVALS)) == 0, "%s: flags %d (want a combination of "
                  "OPTFLOW_USE_INITIAL_FLOW = 4 and OPTFLOW_LK_GET_MIN_EIGENVALS = 8)", who, flags);
    SSLAM_REQUIRE(!(flags & KLT_USE_INITIAL_FLOW) || init != nullptr, "%s: OPTFLOW_USE_INITIAL_FLOW without an initial guess (NULL)", who);
    return 0;
}

}  // namespace

extern "C" int sslam_klt_create(sslam_ctx* ctx, int max_w, int max_h, int max_points, int win_w, int win_h, int max_level,
                                sslam_klt** out) {
    const char* who = "sslam_klt_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(max_w >= 1 && max_w <= KLT_MAX_SIDE && max_h >= 1 && max_h <= KLT_MAX_SIDE, "%s: frame size %dx%d outside 1..%d", who,
                  max_w, max_h, KLT_MAX_SIDE);
    SSLAM_REQUIRE(max_points >= 1 && max_points <= KLT_MAX_POINTS, "%s: capacity of %d points outside 1..%d", who, max_points, KLT_MAX_POINTS);
    SSLAM_REQUIRE((win_w & 1) && (win_h & 1), "%s: window %dx%d has an even side (want odd sides)", who, win_w, win_h);
    SSLAM_REQUIRE(win_w >= KLT_MIN_WIN && win_w <= KLT_MAX_WIN && win_h >= KLT_MIN_WIN && win_h <= KLT_MAX_WIN,
                  "%s: window %dx%d outside %d..%d", who, win_w, win_h, KLT_MIN_WIN, KLT_MAX_WIN);
    SSLAM_REQUIRE(max_level >= 0 && max_level < KLT_MAX_LEVELS, "%s: maxLevel %d outside 0..%d", who, max_level, KLT_MAX_LEVELS - 1);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_klt> k(new sslam_klt);
    k->ctx = ctx; k->max_w = max_w; k->max_h = max_h; k->max_points = max_points; k->ww = win_w; k->wh = win_h; k->max_level = max_level;
    if (int rc = k->slab.alloc(who, false, [&](sslam::Slab& S) { klt_bind(k.get(), S); })) return rc;
    sslam::ctx_retain(ctx);
    *out = k.release();
    return 0;
}

extern "C" int sslam_klt_destroy(sslam_klt* k) {
    return sslam::destroy_instance(k);
}

extern "C" int sslam_klt_push_dev(sslam_klt* k, const uint8_t* img, int h, int w, int c) {
    if (int rc = klt_check_image("sslam_klt_push_dev", k, img, h, w, c)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    return klt_enqueue_push(k, img, h, w, c);
}

extern "C" int sslam_klt_push_host(sslam_klt* k, const uint8_t* img, int h, int w, int c) {
    if (int rc = klt_check_image("sslam_klt_push_host", k, img, h, w, c)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    const uint8_t* img_dev;
    if (int rc = sslam::feat_stage_image(k->ctx, img, h, w, c, &img_dev)) return rc;
    if (int rc = klt_enqueue_push(k, img_dev, h, w, c)) return rc;
    SSLAM_HIP_CHECK(hipStreamSynchronize(k->ctx->stream));            // the caller's image has been read, the scratch slab is free again
    return 0;
}

extern "C" int sslam_klt_gray_host(sslam_ctx* ctx, const uint8_t* img, int h, int w, int c, uint8_t* gray) {
    const char* who = "sslam_klt_gray_host";
    SSLAM_REQUIRE(ctx != nullptr && img != nullptr && gray != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(c == 1 || c == 3 || c == 4, "%s: %d channels (want 1, 3 or 4)", who, c);
    SSLAM_REQUIRE(w >= 1 && w <= KLT_MAX_SIDE && h >= 1 && h <= KLT_MAX_SIDE, "%s: frame size %dx%d outside 1..%d", who, w, h, KLT_MAX_SIDE);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)h * w;
    uint8_t *src = nullptr, *dst = nullptr;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& S) { src = S.take<uint8_t>(n * c); dst = S.take<uint8_t>(n); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, src, img, n * c));
    (void)hipGetLastError();
    hipLaunchKernelGGL(klt_gray_kernel, dim3(klt_blocks(n)), dim3(KLT_T), 0, s, (const uint8_t*)src, h, w, c, dst, w);
    SSLAM_HIP_CHECK(hipGetLastError());
    SSLAM_HIP_CHECK(sslam::copy_down(s, gray, dst, n));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_klt_info(sslam_klt* k, int previous, int* top_level, int* w, int* h) {
    const char* who = "sslam_klt_info";
    SSLAM_REQUIRE(k != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(top_level && w && h, "%s: NULL argument", who);
    const KltFrame& F = k->fr[previous ? k->cur ^ 1 : k->cur];
    SSLAM_REQUIRE(F.top >= 0, "%s: no %s frame has been pushed", who, previous ? "previous" : "current");
    *top_level = F.top; *w = F.lv[0].w; *h = F.lv[0].h;
    return 0;
}

extern "C" int sslam_klt_levels_read(sslam_klt* k, int previous, int level, uint8_t* img, int16_t* dx, int16_t* dy) {
    const char* who = "sslam_klt_levels_read";
    SSLAM_REQUIRE(k != nullptr, "%s: instance is NULL", who);
    const KltFrame& F = k->fr[previous ? k->cur ^ 1 : k->cur];
    SSLAM_REQUIRE(F.top >= 0, "%s: no %s frame has been pushed", who, previous ? "previous" : "current");
    SSLAM_REQUIRE(level >= 0 && level <= F.top, "%s: level %d outside 0..%d", who, level, F.top);
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    const KltLevel& L = F.lv[level];
    const size_t stride = (size_t)L.w + 2 * k->ww, np = klt_padded(k, L.w, L.h), o = (size_t)k->wh * stride + k->ww;
    hipStream_t s = k->ctx->stream;
    if (img) {
        std::vector<uint8_t> pad(np);
        SSLAM_HIP_CHECK(hipMemcpyAsync(pad.data(), L.img, np, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
        for (int y = 0; y < L.h; ++y) std::memcpy(img + (size_t)y * L.w, pad.data() + o + y * stride, (size_t)L.w);
    }
    if (dx || dy) {
        std::vector<uint32_t> pad(np);
        SSLAM_HIP_CHECK(hipMemcpyAsync(pad.data(), L.der, np * 4, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
        for (int y = 0; y < L.h; ++y)
            for (int x = 0; x < L.w; ++x) {
                const uint32_t r = pad[o + y * stride + x];
                if (dx) dx[(size_t)y * L.w + x] = (int16_t)(r & 0xffffu);
                if (dy) dy[(size_t)y * L.w + x] = (int16_t)(r >> 16);
            }
    }
    return 0;
}

extern "C" int sslam_klt_track_dev(sslam_klt* k, int reverse, int n, const float* prev_pts, const float* init_pts, int flags,
                                   int criteria_type, int max_count, double epsilon, double min_eig_threshold, float* next_pts,
                                   uint8_t* status, float* err) {
    const char* who = "sslam_klt_track_dev";
    if (int rc = klt_check_track(who, k, n)) return rc;
    SSLAM_REQUIRE(prev_pts && next_pts && status && err, "%s: NULL argument", who);
    if (int rc = klt_check_flags(who, flags, init_pts)) return rc;
    int count; double eps2;
    if (int rc = klt_criteria(who, criteria_type, max_count, epsilon, min_eig_threshold, &count, &eps2)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    return klt_enqueue_track(k, reverse, n, prev_pts, init_pts, flags, count, eps2, min_eig_threshold, next_pts, status, err);
}

extern "C" int sslam_klt_track_host(sslam_klt* k, int reverse, int n, const float* prev_pts, const float* init_pts, int flags,
                                    int criteria_type, int max_count, double epsilon, double min_eig_threshold, float* next_pts,
                                    uint8_t* status, float* err) {
    const char* who = "sslam_klt_track_host";
    if (int rc = klt_check_track(who, k, n)) return rc;
    SSLAM_REQUIRE(prev_pts && next_pts && status && err, "%s: NULL argument", who);
    if (int rc = klt_check_flags(who, flags, init_pts)) return rc;
    int count; double eps2;
    if (int rc = klt_criteria(who, criteria_type, max_count, epsilon, min_eig_threshold, &count, &eps2)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    hipStream_t s = k->ctx->stream;
    const size_t n8 = (size_t)n * 8;
    SSLAM_HIP_CHECK(hipMemcpyAsync(k->prev, prev_pts, n8, hipMemcpyHostToDevice, s));
    if (flags & KLT_USE_INITIAL_FLOW) SSLAM_HIP_CHECK(hipMemcpyAsync(k->init, init_pts, n8, hipMemcpyHostToDevice, s));
    if (int rc = klt_enqueue_track(k, reverse, n, k->prev, k->init, flags, count, eps2, min_eig_threshold, k->next, k->status, k->err))
        return rc;
    SSLAM_HIP_CHECK(hipMemcpyAsync(next_pts, k->next, n8, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipMemcpyAsync(status, k->status, (size_t)n, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipMemcpyAsync(err, k->err, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_klt_track_fb_dev(sslam_klt* k, int n, const float* prev_pts, int criteria_type, int max_count, double epsilon,
                                      double min_eig_threshold, double err_thresh, double fb_thresh, float* next_pts, float* pts0,
                                      float* pts1, int* counts, uint8_t* mask) {
    const char* who = "sslam_klt_track_fb_dev";
    if (int rc = klt_check_track(who, k, n)) return rc;
    SSLAM_REQUIRE(prev_pts && pts0 && pts1 && counts, "%s: NULL argument", who);
    int count; double eps2;
    if (int rc = klt_criteria(who, criteria_type, max_count, epsilon, min_eig_threshold, &count, &eps2)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    return klt_enqueue_fb(k, n, prev_pts, count, eps2, min_eig_threshold, err_thresh, fb_thresh, next_pts ? next_pts : k->next, pts0, pts1,
                          counts, mask);
}

extern "C" int sslam_klt_track_fb_host(sslam_klt* k, int n, const float* prev_pts, int criteria_type, int max_count, double epsilon,
                                       double min_eig_threshold, double err_thresh, double fb_thresh, float* next_pts, float* pts0,
                                       float* pts1, int* counts, uint8_t* mask) {
    const char* who = "sslam_klt_track_fb_host";
    if (int rc = klt_check_track(who, k, n)) return rc;
    SSLAM_REQUIRE(prev_pts && pts0 && pts1 && counts, "%s: NULL argument", who);
    int count; double eps2;
    if (int rc = klt_criteria(who, criteria_type, max_count, epsilon, min_eig_threshold, &count, &eps2)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(k->ctx->device));
    hipStream_t s = k->ctx->stream;
    const size_t n8 = (size_t)n * 8;
    SSLAM_HIP_CHECK(hipMemcpyAsync(k->prev, prev_pts, n8, hipMemcpyHostToDevice, s));
    if (int rc = klt_enqueue_fb(k, n, k->prev, count, eps2, min_eig_threshold, err_thresh, fb_thresh, k->next, k->pts0, k->pts1, k->counts,
                                k->mask))
        return rc;
    SSLAM_HIP_CHECK(hipMemcpyAsync(counts, k->counts, 5 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (next_pts) SSLAM_HIP_CHECK(hipMemcpyAsync(next_pts, k->next, n8, hipMemcpyDeviceToHost, s));
    if (mask) SSLAM_HIP_CHECK(hipMemcpyAsync(mask, k->mask, (size_t)n, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const size_t kept = (size_t)counts[4];               // only the kept pairs travel
    if (kept) {
        SSLAM_HIP_CHECK(hipMemcpyAsync(pts0, k->pts0, kept * 8, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipMemcpyAsync(pts1, k->pts1, kept * 8, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}
