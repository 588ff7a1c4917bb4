// sift_kernels.hip - SIFT on the GPU: `cv2.SIFT_create(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma)
// .detectAndCompute(img, None)` for 8-bit images.
//
// The float-descriptor detector of the reference's OpenCV branch (`--detector sift`, `_get_opencv_detector` at
// slam/core/features_utils.py:33-55); it produces what sslam_bf_match_dev consumes with NORM_L2 and D = 128: float32 rows of
// 128 integer values and a device count.  Semantics: tests/sift_ref.py restates OpenCV's SIFT_Impl::detectAndCompute stage by
// stage and lists what could not be confirmed without cv2; the kernels equal it bit for bit.  THE DEFINED ARITHMETIC: float32,
// one IEEE operation at a time in the order of the restatement (contraction is off for the whole file); exp, pow, cos and sin
// are the float64 function of the float32 argument rounded once; the 36-bin orientation histogram and the 128-bin descriptor
// histogram are sums of 64-bit integers at the plan's fixed-point scale (LDS atomics), so they are exact and order-free - a
// stated departure from OpenCV's build-dependent float accumulation.  THE ORDER of the output is KeyPoint_LessThan's (x, y
// ascending, size descending, angle ascending); duplicates are dropped before the quota, ties at the quota are kept.
//
// Everything the host decides is in sift_plan.hpp.  A frame of n octaves with L = nOctaveLayers is
//   1 memset of the control block
//   1 sift_base_kernel          grey (15-bit BGR2GRAY) and the INTER_LINEAR doubling, exact in float32
//   2 (1 + m (L + 2)) blurs     sift_blur_row_kernel, sift_blur_col_kernel: every Gaussian layer from the layer before it (the
//                               chain is serial by construction); the column pass also stores the DoG plane.  m = the plan's
//                               tail_first: the octaves above SIFT_TAIL_PIXELS pixels (and always octave 0)
//   m - 1 sift_decimate_kernel  the next octave's base: every second pixel of layer L
//   1 sift_tail_kernel          the n - m small octaves in one workgroup: their decimations and blurs with barriers between
//   1 sift_extrema_kernel       all octaves and layers through the plan's tile table: the 26-neighbour test with ties, one
//                               append per wavefront
//   1 sift_orient_kernel        a candidate per wavefront: adjustLocalExtrema, the contrast and edge tests, the orientation
//                               histogram, its peaks -> one keypoint each
//   1 sift_dup_kernel           removeDuplicatedSorted as a predicate: a keypoint is dropped when one with the same pt, size and
//                               angle precedes it
//   1 sift_quota_kernel         retainBest(nfeatures): kept when fewer than nfeatures keypoints have a larger response
//   1 sift_describe_kernel      a kept keypoint per wavefront: its rank under the output order, the first-octave rebase, the
//                               descriptor
// with every count on the device and no synchronisation.
// MEMORY SAFETY: a candidate is at least 5 pixels inside its octave and in layers 1 .. L of the L + 2 DoG planes; the
// refinement leaves (and the candidate with it) when a step takes it outside that range, so its reads at +-1 are inside.  The
// orientation and the descriptor read a Gaussian plane at x +- 1, y +- 1 only for 0 < x < w - 1, 0 < y < h - 1.  Histogram bins
// are range-checked before the add.  A list index is checked against its capacity before the store; the counters keep
// counting, and a frame whose count exceeds a capacity is voided (count 0, the sticky overflow word), never truncated.  The
// blurs reflect every tap into the plane (as often as it takes).  All loops are bounded by plan constants, by the radii
// (bounded by sigma <= 8 and the image diagonal) or by device counts clamped to the capacities.
// PARITY UNPINNED: cv2 is absent here; tests/sift_ref.py names what could not be confirmed.
#include "common.hpp"
#include "feat_device.hpp"
#include "feat_host.hpp"
#include "geom_common.hpp"
#include "sift_plan.hpp"

#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

using namespace sslam;

constexpr int SIFT_T = 256;
constexpr int SIFT_WAVES = SIFT_T / 64;

struct SiftCtl {                                 // zeroed at the head of every call
    int32_t ncand, nkp, nout, pad;               // the counters keep counting beyond the capacities
};

struct SiftOctDev {
    int w, h, tx, tile_base;
    long long goff, doff;
};

struct SiftArgs {
    int noct, nol, nfeatures, threshold, cand_cap, kp_cap, ext_tiles;
    double contrast, edge, sigma;
    SiftConsts k;
    SiftOctDev oc[SIFT_MAX_OCTAVES];
    float* gauss; float* dog;
    int32_t* cand;                               // [cand_cap][4] octave, layer, r, c
    int32_t* ref;                                // [cand_cap][8] ok, r, c, layer, octave field, x, y, size (float32 bits)
    float* hist;                                 // [cand_cap][40] the smoothed histogram, [36] the response
    uint32_t* kp;                                // [kp_cap][8] x, y, size, angle, response (float32 bits), octave field, candidate
    int32_t* flag;                               // [kp_cap] 1: duplicate, 2: kept
    float* rkey;                                 // [kp_cap] the response, -1 for a duplicate
    SiftCtl* ctl;
    int32_t* sticky;
    float* xy_out; float* aux_out; int32_t* oct_out; float* desc_out; int32_t* n_out;
};

// ---- the base image ---------------------------------------------------------------------------------------------------
// INTER_LINEAR at scale 2: destination d reads source (d + 0.5) / 2 - 0.5 = s + f with f = 0.75 (d even, s = d / 2 - 1) or 0.25
// (d odd, s = (d - 1) / 2); a tap outside the source clamps with weight 0
__device__ __forceinline__ void sift_up_tap(int d, int n, int& s0, int& s1, float& f) {
    int s = (d & 1) ? d >> 1 : (d >> 1) - 1;
    f = (d & 1) ? 0.25f : 0.75f;
    if (s < 0 || s >= n - 1) f = 0.f;
    s = min(max(s, 0), n - 1);
    s0 = s; s1 = min(s + 1, n - 1);
}

__device__ __forceinline__ float sift_grey(const uint8_t* __restrict__ s, int C) { return (float)bgr_to_grey(s, C); }

__global__ __launch_bounds__(SIFT_T) void sift_base_kernel(const uint8_t* __restrict__ src, int w, int h, int C, float* __restrict__ dst) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * SIFT_WAVES + (threadIdx.x >> 6);
    if (x >= 2 * w || y >= 2 * h) return;
    int x0, x1, y0, y1;
    float fx, fy;
    sift_up_tap(x, w, x0, x1, fx);
    sift_up_tap(y, h, y0, y1, fy);
    const float a = sift_grey(src + ((size_t)y0 * w + x0) * C, C), b = sift_grey(src + ((size_t)y0 * w + x1) * C, C);
    const float c = sift_grey(src + ((size_t)y1 * w + x0) * C, C), d = sift_grey(src + ((size_t)y1 * w + x1) * C, C);
    const float h0 = a * (1.f - fx) + b * fx, h1 = c * (1.f - fx) + d * fx;
    dst[(size_t)y * (2 * w) + x] = h0 * (1.f - fy) + h1 * fy;
}

// ---- the blurs: acc = 0; for k ascending: acc = acc + tap_k * px_k, the product and the sum each rounded ---------------------
// A thread makes SIFT_BLUR_R consecutive outputs along the blurred axis from one sliding read of n + SIFT_BLUR_R - 1 inputs:
// input m is tap m - j of output j, so every output still adds its taps in ascending order - the chains are independent.  The
// inputs and taps of SIFT_BLUR_CHUNK steps are loaded together, ahead of the arithmetic: a pass is bound by the latency of its
// loads, not by their number.
constexpr int SIFT_BLUR_R = 4, SIFT_BLUR_CHUNK = 16;

// src(m): input m of the sliding read
template <class Src>
__device__ __forceinline__ void sift_blur_run(Src src, const float* __restrict__ taps, int n, float (&acc)[SIFT_BLUR_R]) {
    const int total = n + SIFT_BLUR_R - 1;
    for (int m0 = 0; m0 < total; m0 += SIFT_BLUR_CHUNK) {
        float v[SIFT_BLUR_CHUNK], tp[SIFT_BLUR_CHUNK + SIFT_BLUR_R - 1];
#pragma unroll
        for (int u = 0; u < SIFT_BLUR_CHUNK; ++u) v[u] = src(min(m0 + u, total - 1));
#pragma unroll
        for (int q = 0; q < SIFT_BLUR_CHUNK + SIFT_BLUR_R - 1; ++q) tp[q] = taps[min(max(m0 - (SIFT_BLUR_R - 1) + q, 0), n - 1)];
#pragma unroll
        for (int u = 0; u < SIFT_BLUR_CHUNK; ++u)
#pragma unroll
            for (int j = 0; j < SIFT_BLUR_R; ++j) {
                const int k = m0 + u - j;                      // the tap of output j that input m0 + u meets: tp[u - j + R - 1]
                if (k >= 0 && k < n) { const float t = tp[u - j + SIFT_BLUR_R - 1] * v[u]; acc[j] = acc[j] + t; }
            }
    }
}

// outputs x0 .. x0 + R - 1 of row y
__device__ __forceinline__ void sift_blur_row_at(const float* __restrict__ src, float* __restrict__ dst, int w, const float* __restrict__ taps,
                                                 int n, int x0, int y) {
    const float* row = src + (size_t)y * w;
    const int first = x0 - (n >> 1);
    float acc[SIFT_BLUR_R] = {};
    sift_blur_run([&](int m) { return row[reflect101(first + m, w)]; }, taps, n, acc);
#pragma unroll
    for (int j = 0; j < SIFT_BLUR_R; ++j)
        if (x0 + j < w) dst[(size_t)y * w + x0 + j] = acc[j];
}

// outputs y0 .. y0 + R - 1 of column x, and the DoG plane against the layer before
__device__ __forceinline__ void sift_blur_col_at(const float* __restrict__ src, float* __restrict__ dst, int w, int h, const float* __restrict__ taps,
                                                 int n, const float* prev, float* __restrict__ dog, float* also, int x, int y0) {
    const int first = y0 - (n >> 1);
    float acc[SIFT_BLUR_R] = {};
    sift_blur_run([&](int m) { return src[(size_t)reflect101(first + m, h) * w + x]; }, taps, n, acc);
#pragma unroll
    for (int j = 0; j < SIFT_BLUR_R; ++j)
        if (y0 + j < h) {
            const size_t i = (size_t)(y0 + j) * w + x;
            dst[i] = acc[j];
            if (dog) dog[i] = acc[j] - prev[i];
            if (also) also[i] = acc[j];                        // (after prev[i] was read: `also` may be `prev`)
        }
}

__global__ __launch_bounds__(SIFT_T) void sift_blur_row_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h,
                                                               const float* __restrict__ taps, int n) {
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * SIFT_BLUR_R, y = blockIdx.y * SIFT_WAVES + (threadIdx.x >> 6);
    if (x0 >= w || y >= h) return;
    sift_blur_row_at(src, dst, w, taps, n, x0, y);
}

__global__ __launch_bounds__(SIFT_T) void sift_blur_col_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h,
                                                               const float* __restrict__ taps, int n, const float* __restrict__ prev,
                                                               float* __restrict__ dog) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y0 = (blockIdx.y * SIFT_WAVES + (threadIdx.x >> 6)) * SIFT_BLUR_R;
    if (x >= w || y0 >= h) return;
    sift_blur_col_at(src, dst, w, h, taps, n, prev, dog, nullptr, x, y0);
}

__global__ __launch_bounds__(SIFT_T) void sift_decimate_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * SIFT_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    dst[(size_t)y * w + x] = src[(size_t)(2 * y) * sw + 2 * x];
}

// The small octaves (the plan's tail_first .. noct - 1, each of at most SIFT_TAIL_PIXELS pixels) in ONE workgroup: decimate, then
// every layer's row pass and column pass with a barrier between the steps - the same per-output arithmetic as the kernels above,
// in place of eleven launches per octave that each cost more than their work.  The current layer and the row pass's
// intermediate stay in LDS (two planes of SIFT_TAIL_PIXELS floats); every layer and DoG plane is also stored to its slab.
struct SiftTailTaps { int n[SIFT_MAX_LAYERS], off[SIFT_MAX_LAYERS]; };

__global__ __launch_bounds__(SIFT_TAIL_T) void sift_tail_kernel(SiftArgs a, int first, const float* __restrict__ taps, SiftTailTaps tt) {
    __shared__ float s_cur[SIFT_TAIL_PIXELS], s_tmp[SIFT_TAIL_PIXELS];
    const int tid = threadIdx.x;
    for (int o = first; o < a.noct; ++o) {
        const SiftOctDev O = a.oc[o], S = a.oc[o - 1];
        const int w = O.w, h = O.h;
        if (w * h > SIFT_TAIL_PIXELS) continue;                 // (the plan never sends one)
        const size_t plane = (size_t)w * h;
        float* G = a.gauss + O.goff;
        float* D = a.dog + O.doff;
        const float* up = a.gauss + S.goff + (size_t)a.nol * S.w * S.h;
        __syncthreads();                                        // (the octave before has been read)
        for (int i = tid; i < w * h; i += SIFT_TAIL_T) {
            const int y = i / w, x = i - y * w;
            const float v = up[(size_t)(2 * y) * S.w + 2 * x];
            G[i] = v; s_cur[i] = v;
        }
        __syncthreads();
        const int gx = (w + SIFT_BLUR_R - 1) / SIFT_BLUR_R, gy = (h + SIFT_BLUR_R - 1) / SIFT_BLUR_R;
        for (int l = 1; l < a.nol + 3; ++l) {
            const float* tp = taps + tt.off[l];
            for (int i = tid; i < gx * h; i += SIFT_TAIL_T) { const int y = i / gx; sift_blur_row_at(s_cur, s_tmp, w, tp, tt.n[l], (i - y * gx) * SIFT_BLUR_R, y); }
            __syncthreads();
            for (int i = tid; i < w * gy; i += SIFT_TAIL_T) {
                const int yq = i / w;
                sift_blur_col_at(s_tmp, G + l * plane, w, h, tp, tt.n[l], s_cur, D + (l - 1) * plane, s_cur, i - yq * w, yq * SIFT_BLUR_R);
            }
            __syncthreads();
        }
    }
}

// ---- extrema ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SIFT_T) void sift_extrema_kernel(SiftArgs a) {
    int o = 0;
    for (int i = 1; i < SIFT_MAX_OCTAVES; ++i)
        if (i < a.noct && a.oc[i].tx > 0 && (int)blockIdx.x >= a.oc[i].tile_base) o = i;
    const SiftOctDev O = a.oc[o];
    const int tile = blockIdx.x - O.tile_base, lane = threadIdx.x & 63;
    const int x = (tile % O.tx) * SIFT_TILE_W + lane, y = (tile / O.tx) * SIFT_TILE_H + (threadIdx.x >> 6);
    const int layer = 1 + blockIdx.y;
    bool is = false;
    if (x >= SIFT_IMG_BORDER && x < O.w - SIFT_IMG_BORDER && y >= SIFT_IMG_BORDER && y < O.h - SIFT_IMG_BORDER) {
        const size_t plane = (size_t)O.w * O.h;
        const float* c = a.dog + O.doff + (size_t)layer * plane + (size_t)y * O.w + x;
        const float v = c[0];
        if (fabsf(v) > (float)a.threshold) {
            bool ge = true, le = true;
#pragma unroll
            for (int dl = -1; dl <= 1; ++dl)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        const float nb = c[(ptrdiff_t)dl * (ptrdiff_t)plane + dy * O.w + dx];
                        ge = ge && v >= nb; le = le && v <= nb;
                    }
            is = (v > 0.f && ge) || (v < 0.f && le);
        }
    }
    const unsigned long long bal = __ballot(is);
    if (!bal) return;
    int base = 0;
    if (lane == 0) base = atomicAdd(&a.ctl->ncand, __popcll(bal));
    base = __shfl(base, 0);
    if (is) {
        const int i = base + __popcll(bal & ((1ull << lane) - 1));
        if (i < a.cand_cap) {
            int32_t* q = a.cand + 4 * (size_t)i;
            q[0] = o; q[1] = layer; q[2] = y; q[3] = x;
        }
    }
}

// ---- refinement and orientation: a candidate per wavefront -----------------------------------------------------------------
__device__ __forceinline__ float sift_exp(float x) { return (float)exp((double)x); }

// cv::LU on a 3 x 3 float32 system, partial pivoting; x = 0 for a singular one
__device__ __forceinline__ void sift_solve3(float A[3][3], float b[3], float eps) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int k = i;
        for (int j = i + 1; j < 3; ++j)
            if (fabsf(A[j][i]) > fabsf(A[k][i])) k = j;
        if (fabsf(A[k][i]) < eps) { b[0] = b[1] = b[2] = 0.f; return; }
        if (k != i) {
            for (int c = 0; c < 3; ++c) { const float t = A[i][c]; A[i][c] = A[k][c]; A[k][c] = t; }
            const float t = b[i]; b[i] = b[k]; b[k] = t;
        }
        const float d = -1.f / A[i][i];
        for (int j = i + 1; j < 3; ++j) {
            const float alpha = A[j][i] * d;
            for (int c = i + 1; c < 3; ++c) { const float t = alpha * A[i][c]; A[j][c] = A[j][c] + t; }
            const float t = alpha * b[i];
            b[j] = b[j] + t;
        }
    }
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        float s = b[i];
        for (int c = i + 1; c < 3; ++c) { const float t = A[i][c] * b[c]; s = s - t; }
        b[i] = s / A[i][i];
    }
}

__global__ __launch_bounds__(SIFT_T) __attribute__((target("no-packed-fp32-ops"))) void sift_orient_kernel(SiftArgs a) {
    __shared__ unsigned long long s_acc[SIFT_WAVES][SIFT_ORI_BINS];
    __shared__ float s_raw[SIFT_WAVES][SIFT_ORI_BINS], s_hist[SIFT_WAVES][SIFT_ORI_BINS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = min(a.ctl->ncand, a.cand_cap);
    const SiftConsts& K = a.k;
    for (int ci = blockIdx.x * SIFT_WAVES + wave; ci < n; ci += gridDim.x * SIFT_WAVES) {
        const int32_t* q = a.cand + 4 * (size_t)ci;
        const int o = q[0];
        int layer = q[1], r = q[2], c = q[3];
        const SiftOctDev O = a.oc[o];
        const size_t plane = (size_t)O.w * O.h;
        const float* D = a.dog + O.doff;
        // adjustLocalExtrema, the same on every lane
        float xi = 0.f, xr = 0.f, xc = 0.f;
        bool ok = false;
        for (int step = 0; step < SIFT_MAX_INTERP_STEPS; ++step) {
            const float* img = D + (size_t)layer * plane + (size_t)r * O.w + c;
            const float* prv = img - plane;
            const float* nxt = img + plane;
            float b[3] = {(img[1] - img[-1]) * K.deriv_scale, (img[O.w] - img[-O.w]) * K.deriv_scale, (nxt[0] - prv[0]) * K.deriv_scale};
            const float v2 = img[0] * 2.f;
            const float dxx = (img[1] + img[-1] - v2) * K.second_scale, dyy = (img[O.w] + img[-O.w] - v2) * K.second_scale;
            const float dss = (nxt[0] + prv[0] - v2) * K.second_scale;
            const float dxy = (img[O.w + 1] - img[O.w - 1] - img[-O.w + 1] + img[-O.w - 1]) * K.cross_scale;
            const float dxs = (nxt[1] - nxt[-1] - prv[1] + prv[-1]) * K.cross_scale;
            const float dys = (nxt[O.w] - nxt[-O.w] - prv[O.w] + prv[-O.w]) * K.cross_scale;
            float A[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}};
            sift_solve3(A, b, K.flt_epsilon * 10.f);
            xi = -b[2]; xr = -b[1]; xc = -b[0];
            if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) { ok = true; break; }
            const float big = (float)(2147483647 / 3);
            if (!(fabsf(xi) <= big && fabsf(xr) <= big && fabsf(xc) <= big)) break;
            c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
            if (layer < 1 || layer > a.nol || c < SIFT_IMG_BORDER || c >= O.w - SIFT_IMG_BORDER || r < SIFT_IMG_BORDER || r >= O.h - SIFT_IMG_BORDER) break;
        }
        float contr = 0.f;
        if (ok) {
            const float* img = D + (size_t)layer * plane + (size_t)r * O.w + c;
            const float d0 = (img[1] - img[-1]) * K.deriv_scale, d1 = (img[O.w] - img[-O.w]) * K.deriv_scale;
            const float d2 = (img[plane] - (img - plane)[0]) * K.deriv_scale;
            float t = d0 * xc;
            float u = d1 * xr; t = t + u;
            u = d2 * xi; t = t + u;
            u = img[0] * K.img_scale; t = t * 0.5f;
            contr = u + t;
            const float v2 = img[0] * 2.f;
            const float dxx = (img[1] + img[-1] - v2) * K.second_scale, dyy = (img[O.w] + img[-O.w] - v2) * K.second_scale;
            const float dxy = (img[O.w + 1] - img[O.w - 1] - img[-O.w + 1] + img[-O.w - 1]) * K.cross_scale;
            const float tr = dxx + dyy;
            const float p0 = dxx * dyy, p1 = dxy * dxy, det = p0 - p1;
            const float tr2 = tr * tr;
            if ((double)(fabsf(contr) * (float)a.nol) < a.contrast) ok = false;
            else if (det <= 0.f || (double)tr2 * a.edge >= (a.edge + 1) * (a.edge + 1) * (double)det) ok = false;
        }
        const float p2 = (float)(1 << o);
        const float arg = ((float)layer + xi) / (float)a.nol;
        const float pw = (float)pow(2.0, (double)arg);
        const float size = (float)(a.sigma * (double)pw * (double)(1 << o) * 2.0);
        const float px = ((float)c + xc) * p2, py = ((float)r + xr) * p2;
        const float resp = fabsf(contr);
        const int field = o + (layer << 8) + ((int)rintf((xi + 0.5f) * 255.f) << 16);
        if (lane == 0) {
            int32_t* w = a.ref + 8 * (size_t)ci;
            w[0] = ok; w[1] = r; w[2] = c; w[3] = layer; w[4] = ok ? field : 0;
            w[5] = ok ? (int32_t)__float_as_uint(px) : 0; w[6] = ok ? (int32_t)__float_as_uint(py) : 0; w[7] = ok ? (int32_t)__float_as_uint(size) : 0;
        }
        if (!ok) continue;                                      // (uniform)
        // calcOrientationHist on the Gaussian layer
        const float scl = size * 0.5f / p2;
        const int radius = (int)rintf(4.5f * scl);
        const float sg = 1.5f * scl;
        const float escale = -1.f / (2.f * sg * sg);
        const float* G = a.gauss + O.goff + (size_t)layer * plane;
        if (lane < SIFT_ORI_BINS) s_acc[wave][lane] = 0ull;
        __builtin_amdgcn_wave_barrier();
        const int side = 2 * radius + 1;
        for (int e = lane; e < side * side; e += 64) {
            const int i = e / side - radius, j = e - (e / side) * side - radius;
            const int y = r + i, x = c + j;
            if (y <= 0 || y >= O.h - 1 || x <= 0 || x >= O.w - 1) continue;
            const float* g = G + (size_t)y * O.w + x;
            const float dx = g[1] - g[-1], dy = g[-O.w] - g[O.w];
            const float wgt = sift_exp((float)(i * i + j * j) * escale);
            const float ori = fast_atan2_deg(K.atan, dy, dx);
            const float xx = dx * dx, yy = dy * dy;
            const float mag = sqrtf(xx + yy);
            int bin = (int)rintf((float)SIFT_ORI_BINS / 360.f * ori);
            if (bin >= SIFT_ORI_BINS) bin -= SIFT_ORI_BINS;
            if (bin < 0) bin += SIFT_ORI_BINS;
            if ((unsigned)bin < (unsigned)SIFT_ORI_BINS) atomicAdd(&s_acc[wave][bin], to_fixed<SIFT_HIST_SCALE_LOG2, unsigned long long>(wgt * mag));
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (lane < SIFT_ORI_BINS) s_raw[wave][lane] = from_fixed<SIFT_HIST_SCALE_LOG2>(s_acc[wave][lane]);
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const int n36 = SIFT_ORI_BINS;
        float hv = 0.f;
        if (lane < n36) {
            const float* t = s_raw[wave];
            const float m2 = t[(lane + n36 - 2) % n36], m1 = t[(lane + n36 - 1) % n36], q1 = t[(lane + 1) % n36], q2 = t[(lane + 2) % n36];
            const float s2 = (m2 + q2) * (1.f / 16.f), s1 = (m1 + q1) * (4.f / 16.f), s0 = t[lane] * (6.f / 16.f);
            hv = s2 + s1;
            hv = hv + s0;
            s_hist[wave][lane] = hv;
            a.hist[40 * (size_t)ci + lane] = hv;
        }
        if (lane == 36) a.hist[40 * (size_t)ci + 36] = resp;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        float mx = s_hist[wave][0];
        for (int b = 1; b < n36; ++b) mx = fmaxf(mx, s_hist[wave][b]);
        const float thr = mx * 0.8f;
        bool peak = false;
        float ang = 0.f;
        if (lane < n36) {
            const float hl = s_hist[wave][(lane + n36 - 1) % n36], hr = s_hist[wave][(lane + 1) % n36];
            if (hv > hl && hv > hr && hv >= thr) {
                peak = true;
                float den = hl - 2.f * hv;
                den = den + hr;
                float bin = (float)lane + (0.5f * (hl - hr)) / den;
                bin = bin < 0.f ? (float)n36 + bin : (bin >= (float)n36 ? bin - (float)n36 : bin);
                ang = 360.f - (360.f / (float)n36) * bin;
                if (fabsf(ang - 360.f) < K.flt_epsilon) ang = 0.f;
            }
        }
        const unsigned long long bal = __ballot(peak);
        if (bal) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&a.ctl->nkp, __popcll(bal));
            base = __shfl(base, 0);
            if (peak) {
                const int i = base + __popcll(bal & ((1ull << lane) - 1));
                if (i < a.kp_cap) {
                    uint32_t* w = a.kp + 8 * (size_t)i;
                    w[0] = __float_as_uint(px); w[1] = __float_as_uint(py); w[2] = __float_as_uint(size); w[3] = __float_as_uint(ang);
                    w[4] = __float_as_uint(resp); w[5] = (uint32_t)field; w[6] = (uint32_t)ci; w[7] = 0;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- duplicates, the quota, the output order -----------------------------------------------------------------------------
struct SiftKey { float x, y, size, ang, resp; int oct; };

__device__ __forceinline__ SiftKey sift_key(const uint32_t* __restrict__ kp, int i) {
    const uint32_t* w = kp + 8 * (size_t)i;
    return SiftKey{__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]), __uint_as_float(w[4]), (int)w[5]};
}

__device__ __forceinline__ bool sift_same4(const SiftKey& p, const SiftKey& q) { return p.x == q.x && p.y == q.y && p.size == q.size && p.ang == q.ang; }

__global__ __launch_bounds__(SIFT_T) void sift_dup_kernel(SiftArgs a) {
    if (feat_voided(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.ctl->nkp;
    for (int j = blockIdx.x * SIFT_WAVES + wave; j < n; j += gridDim.x * SIFT_WAVES) {
        const SiftKey me = sift_key(a.kp, j);
        int before = 0;
        for (int i = lane; i < n; i += 64) {
            const SiftKey q = sift_key(a.kp, i);
            before += i != j && sift_same4(q, me) && (q.resp > me.resp || (q.resp == me.resp && (q.oct > me.oct || (q.oct == me.oct && i < j))));
        }
        before = wave_sum(before);
        if (lane == 0) { a.flag[j] = before ? 1 : 0; a.rkey[j] = before ? -1.f : me.resp; }
    }
}

__global__ __launch_bounds__(SIFT_T) void sift_quota_kernel(SiftArgs a) {
    if (feat_voided(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.ctl->nkp;
    for (int j = blockIdx.x * SIFT_WAVES + wave; j < n; j += gridDim.x * SIFT_WAVES) {
        if (a.flag[j] & 1) continue;
        int above = 0;
        if (a.nfeatures > 0) {
            const float mine = a.rkey[j];                       // (>= 0; a duplicate's key is -1 and never above)
            for (int i = lane; i < n; i += 64) above += a.rkey[i] > mine;
            above = wave_sum(above);
        }
        if (lane == 0 && (a.nfeatures == 0 || above < a.nfeatures)) {
            atomicOr(&a.flag[j], 2);
            atomicAdd(&a.ctl->nout, 1);
        }
    }
}

__global__ __launch_bounds__(SIFT_T) __attribute__((target("no-packed-fp32-ops"))) void sift_describe_kernel(SiftArgs a) {
    __shared__ unsigned long long s_acc[SIFT_WAVES][SIFT_DESCR_LEN];
    __shared__ float s_dst[SIFT_WAVES][SIFT_DESCR_LEN];
    __shared__ float s_scale[SIFT_WAVES], s_thr[SIFT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool voided = feat_voided(a);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.n_out[0] = voided ? 0 : a.ctl->nout;
        if (voided) atomicOr(a.sticky, (a.ctl->ncand > a.cand_cap ? 1 : 0) | (a.ctl->nkp > a.kp_cap ? 2 : 0));
    }
    if (voided) return;
    const int n = a.ctl->nkp;
    const SiftConsts& K = a.k;
    constexpr int d = SIFT_DESCR_WIDTH, nb = SIFT_DESCR_BINS;
    for (int j = blockIdx.x * SIFT_WAVES + wave; j < n; j += gridDim.x * SIFT_WAVES) {
        if (!(a.flag[j] & 2)) continue;                        // (uniform)
        const SiftKey me = sift_key(a.kp, j);
        int less = 0;
        for (int i = lane; i < n; i += 64)
            if (a.flag[i] & 2) {
                const SiftKey q = sift_key(a.kp, i);
                less += q.x < me.x || (q.x == me.x && (q.y < me.y || (q.y == me.y && (q.size > me.size || (q.size == me.size && q.ang < me.ang)))));
            }
        const int pos = wave_sum(less);
        // the first octave is -1: pt and size halved, the octave byte rebased; then unpackOctave and the descriptor's frame
        const int field = (me.oct & ~255) | ((me.oct - 1) & 255);
        const float x = me.x * 0.5f, y = me.y * 0.5f, size = me.size * 0.5f;
        const int o = me.oct & 255, layer = (me.oct >> 8) & 255;       // the octave's index in the pyramid
        const float scale = o >= 1 ? 1.f / (float)(1 << (o - 1)) : 2.f;
        const float pxf = x * scale, pyf = y * scale, scl = size * scale * 0.5f;
        float ori = 360.f - me.ang;
        if (fabsf(ori - 360.f) < K.flt_epsilon) ori = 0.f;
        const SiftOctDev O = a.oc[o];
        const float* G = a.gauss + O.goff + (size_t)layer * ((size_t)O.w * O.h);
        const int ix = (int)rintf(pxf), iy = (int)rintf(pyf);
        const float rad = ori * K.atan.deg2rad;
        float cos_t = (float)cos((double)rad), sin_t = (float)sin((double)rad);
        const float bins_per_deg = (float)nb / 360.f;
        const float exp_scale = -1.f / ((float)d * (float)d * 0.5f);
        const float hist_width = 3.f * scl;
        int radius = (int)rintf(hist_width * 1.4142135623730951f * (float)(d + 1) * 0.5f);
        radius = min(radius, (int)sqrt((double)O.w * O.w + (double)O.h * O.h));
        cos_t = cos_t / hist_width; sin_t = sin_t / hist_width;
        s_acc[wave][lane] = 0ull; s_acc[wave][lane + 64] = 0ull;
        __builtin_amdgcn_wave_barrier();
        const int side = 2 * radius + 1;
        for (int e = lane; e < side * side; e += 64) {
            const int i = e / side - radius, jj = e - (e / side) * side - radius;
            const float fi = (float)i, fj = (float)jj;
            const float t0 = fj * cos_t, t1 = fi * sin_t, t2 = fj * sin_t, t3 = fi * cos_t;
            const float c_rot = t0 - t1, r_rot = t2 + t3;
            float rbin = r_rot + (float)(d / 2) - 0.5f, cbin = c_rot + (float)(d / 2) - 0.5f;
            const int yy = iy + i, xx = ix + jj;
            if (!(rbin > -1.f && rbin < (float)d && cbin > -1.f && cbin < (float)d && yy > 0 && yy < O.h - 1 && xx > 0 && xx < O.w - 1)) continue;
            const float* g = G + (size_t)yy * O.w + xx;
            const float dx = g[1] - g[-1], dy = g[-O.w] - g[O.w];
            const float cc = c_rot * c_rot, rr = r_rot * r_rot;
            const float wgt = sift_exp((cc + rr) * exp_scale);
            const float so = fast_atan2_deg(K.atan, dy, dx);
            const float dx2 = dx * dx, dy2 = dy * dy;
            float mag = sqrtf(dx2 + dy2);
            float obin = (so - ori) * bins_per_deg;
            mag = mag * wgt;
            const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
            rbin = rbin - r0f; cbin = cbin - c0f; obin = obin - o0f;
            const int r0 = (int)r0f, c0 = (int)c0f;
            int o0 = (int)o0f;
            if (o0 < 0) o0 += nb;
            if (o0 >= nb) o0 -= nb;
            const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
#pragma unroll
            for (int dr = 0; dr < 2; ++dr) {
                const float vr = dr ? v_r1 : v_r0;
                const float v_c1 = vr * cbin, v_c0 = vr - v_c1;
#pragma unroll
                for (int dc = 0; dc < 2; ++dc) {
                    const float vc = dc ? v_c1 : v_c0;
                    const float v_o1 = vc * obin, v_o0 = vc - v_o1;
                    const int rr2 = r0 + dr, cc2 = c0 + dc;
                    if ((unsigned)rr2 < (unsigned)d && (unsigned)cc2 < (unsigned)d) {
                        unsigned long long* h = &s_acc[wave][(rr2 * d + cc2) * nb];
                        atomicAdd(&h[o0 & (nb - 1)], to_fixed<SIFT_HIST_SCALE_LOG2, unsigned long long>(v_o0));
                        atomicAdd(&h[(o0 + 1) & (nb - 1)], to_fixed<SIFT_HIST_SCALE_LOG2, unsigned long long>(v_o1));
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        s_dst[wave][lane] = from_fixed<SIFT_HIST_SCALE_LOG2>(s_acc[wave][lane]);
        s_dst[wave][lane + 64] = from_fixed<SIFT_HIST_SCALE_LOG2>(s_acc[wave][lane + 64]);
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (lane == 0) {                                       // the two norms: float32 sums in index order
            float nrm2 = 0.f;
            for (int k = 0; k < SIFT_DESCR_LEN; ++k) { const float v = s_dst[wave][k]; const float t = v * v; nrm2 = nrm2 + t; }
            const float thr = sqrtf(nrm2) * 0.2f;
            nrm2 = 0.f;
            for (int k = 0; k < SIFT_DESCR_LEN; ++k) { const float v = fminf(s_dst[wave][k], thr); const float t = v * v; nrm2 = nrm2 + t; }
            s_scale[wave] = 512.f / fmaxf(sqrtf(nrm2), K.flt_epsilon);
            s_thr[wave] = thr;
            a.xy_out[2 * (size_t)pos] = x; a.xy_out[2 * (size_t)pos + 1] = y;
            a.aux_out[3 * (size_t)pos] = size; a.aux_out[3 * (size_t)pos + 1] = me.ang; a.aux_out[3 * (size_t)pos + 2] = me.resp;
            a.oct_out[pos] = field;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const float thr = s_thr[wave], sc = s_scale[wave];
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const int k = lane + 64 * hlf;
            const float v = fminf(s_dst[wave][k], thr) * sc;
            a.desc_out[(size_t)pos * SIFT_DESCR_LEN + k] = fminf(fmaxf(rintf(v), 0.f), 255.f);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

struct sslam_sift {
    sslam_ctx* ctx = nullptr;
    SiftParams p;
    int max_w = 0, max_h = 0, cand_cap = 0, kp_cap = 0;
    SiftPlan plan{};                             // of the last call (stage_read reads it)
    bool have_plan = false;
    SiftTaps taps;
    sslam::OwnedSlab slab;
    float *gauss = nullptr, *dog = nullptr, *tmp_a = nullptr, *tmp_b = nullptr, *taps_dev = nullptr;
    int32_t *cand = nullptr, *ref = nullptr, *flag = nullptr, *sticky = nullptr;
    float *hist = nullptr, *rkey = nullptr;
    uint32_t* kp = nullptr;
    SiftCtl* ctl = nullptr;
    float *xy = nullptr, *aux = nullptr, *desc = nullptr;      // outputs of the host entry
    int32_t *oct = nullptr, *n = nullptr;
};

namespace {

// the slab-backed pointers of the instance, in slab order; P: the plan of the largest frame
void sift_bind(sslam_sift* o, const SiftPlan& P, sslam::Slab& S) {
    const size_t nc = (size_t)o->cand_cap, nk = (size_t)o->kp_cap;
    o->gauss = S.take<float>((size_t)std::max(P.gauss_floats, 1LL));
    o->dog = S.take<float>((size_t)std::max(P.dog_floats, 1LL));
    o->tmp_a = S.take<float>((size_t)P.tmp_floats);
    o->tmp_b = S.take<float>((size_t)P.tmp_floats);
    o->taps_dev = S.take<float>(o->taps.taps.size());
    o->cand = S.take<int32_t>(4 * nc);
    o->ref = S.take<int32_t>(8 * nc);
    o->hist = S.take<float>(40 * nc);
    o->kp = S.take<uint32_t>(8 * nk);
    o->flag = S.take<int32_t>(nk);
    o->rkey = S.take<float>(nk);
    o->ctl = S.take<SiftCtl>(1);
    o->sticky = S.take<int32_t>(1);
    o->xy = S.take<float>(2 * nk);
    o->aux = S.take<float>(3 * nk);
    o->oct = S.take<int32_t>(nk);
    o->desc = S.take<float>(SIFT_DESCR_LEN * nk);
    o->n = S.take<int32_t>(1);
}

int sift_enqueue(sslam_sift* o, const uint8_t* img_dev, int h, int w, int c, float* xy, float* aux, int32_t* oct, float* desc, int32_t* n_out) {
    const SiftPlan P = sift_plan(o->p, w, h);
    o->plan = P; o->have_plan = true;
    hipStream_t s = o->ctx->stream;
    (void)hipGetLastError();
    SSLAM_HIP_CHECK(hipMemsetAsync(o->ctl, 0, sizeof(SiftCtl), s));
    if (P.noct == 0) {                                         // too small for an octave
        SSLAM_HIP_CHECK(hipMemsetAsync(n_out, 0, sizeof(int32_t), s));
        return 0;
    }
    const int L = o->p.nol;
    SiftArgs a{};
    a.noct = P.noct; a.nol = L; a.nfeatures = o->p.nfeatures; a.threshold = P.threshold; a.cand_cap = o->cand_cap; a.kp_cap = o->kp_cap;
    a.ext_tiles = P.ext_tiles; a.contrast = o->p.contrast; a.edge = o->p.edge; a.sigma = o->p.sigma; a.k = sift_consts();
    for (int i = 0; i < P.noct; ++i) a.oc[i] = SiftOctDev{P.oc[i].w, P.oc[i].h, P.oc[i].tx, P.oc[i].tile_base, P.oc[i].goff, P.oc[i].doff};
    a.gauss = o->gauss; a.dog = o->dog; a.cand = o->cand; a.ref = o->ref; a.hist = o->hist; a.kp = o->kp; a.flag = o->flag; a.rkey = o->rkey; a.ctl = o->ctl;
    a.sticky = o->sticky; a.xy_out = xy; a.aux_out = aux; a.oct_out = oct; a.desc_out = desc; a.n_out = n_out;
    const SiftTaps& T = o->taps;
    auto grid = [](int gw, int gh) { return dim3(cdiv(gw, 64), cdiv(gh, SIFT_WAVES)); };
    auto rgrid = [](int gw, int gh) { return dim3(cdiv(gw, 64 * SIFT_BLUR_R), cdiv(gh, SIFT_WAVES)); };
    auto cgrid = [](int gw, int gh) { return dim3(cdiv(gw, 64), cdiv(gh, SIFT_WAVES * SIFT_BLUR_R)); };
    hipLaunchKernelGGL(sift_base_kernel, grid(2 * w, 2 * h), dim3(SIFT_T), 0, s, img_dev, w, h, c, o->tmp_a);
    for (int oi = 0; oi < P.tail_first; ++oi) {
        const SiftOctave& O = P.oc[oi];
        const size_t plane = (size_t)O.w * O.h;
        float* G = o->gauss + O.goff;
        float* D = o->dog + O.doff;
        if (oi == 0) {
            hipLaunchKernelGGL(sift_blur_row_kernel, rgrid(O.w, O.h), dim3(SIFT_T), 0, s, o->tmp_a, o->tmp_b, O.w, O.h, o->taps_dev + T.off[0], T.n[0]);
            hipLaunchKernelGGL(sift_blur_col_kernel, cgrid(O.w, O.h), dim3(SIFT_T), 0, s, o->tmp_b, G, O.w, O.h, o->taps_dev + T.off[0], T.n[0],
                               (const float*)nullptr, (float*)nullptr);
        } else {
            const SiftOctave& S = P.oc[oi - 1];
            hipLaunchKernelGGL(sift_decimate_kernel, grid(O.w, O.h), dim3(SIFT_T), 0, s, o->gauss + S.goff + (size_t)L * S.w * S.h, S.w, G, O.w, O.h);
        }
        for (int i = 1; i < L + 3; ++i) {
            hipLaunchKernelGGL(sift_blur_row_kernel, rgrid(O.w, O.h), dim3(SIFT_T), 0, s, G + (i - 1) * plane, o->tmp_b, O.w, O.h, o->taps_dev + T.off[i], T.n[i]);
            hipLaunchKernelGGL(sift_blur_col_kernel, cgrid(O.w, O.h), dim3(SIFT_T), 0, s, o->tmp_b, G + i * plane, O.w, O.h, o->taps_dev + T.off[i], T.n[i],
                               (const float*)(G + (i - 1) * plane), D + (i - 1) * plane);
        }
    }
    if (P.tail_first < P.noct) {
        SiftTailTaps tt{};
        for (int i = 0; i < L + 3; ++i) { tt.n[i] = T.n[i]; tt.off[i] = T.off[i]; }
        hipLaunchKernelGGL(sift_tail_kernel, dim3(1), dim3(SIFT_TAIL_T), 0, s, a, P.tail_first, (const float*)o->taps_dev, tt);
    }
    if (P.ext_tiles > 0) hipLaunchKernelGGL(sift_extrema_kernel, dim3(P.ext_tiles, L), dim3(SIFT_T), 0, s, a);
    hipLaunchKernelGGL(sift_orient_kernel, dim3(SIFT_KP_GX), dim3(SIFT_T), 0, s, a);
    hipLaunchKernelGGL(sift_dup_kernel, dim3(SIFT_KP_GX), dim3(SIFT_T), 0, s, a);
    hipLaunchKernelGGL(sift_quota_kernel, dim3(SIFT_KP_GX), dim3(SIFT_T), 0, s, a);
    hipLaunchKernelGGL(sift_describe_kernel, dim3(SIFT_KP_GX), dim3(SIFT_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int sslam_sift_create(sslam_ctx* ctx, int max_w, int max_h, int nfeatures, int n_octave_layers, double contrast_threshold,
                                 double edge_threshold, double sigma, int max_candidates, int max_keypoints, sslam_sift** out) {
    const char* who = "sslam_sift_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    SiftParams p;
    p.nfeatures = nfeatures; p.nol = n_octave_layers; p.contrast = contrast_threshold; p.edge = edge_threshold; p.sigma = sigma;
    char msg[160];
    if (sift_check_params(p, max_w, max_h, msg, sizeof msg)) { sslam::set_error("%s: %s", who, msg); return 2; }
    SSLAM_REQUIRE(max_candidates >= 0 && max_keypoints >= 0, "%s: max_candidates %d / max_keypoints %d is negative (0: the default)", who,
                  max_candidates, max_keypoints);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_sift> o(new sslam_sift);
    o->ctx = ctx; o->p = p; o->max_w = max_w; o->max_h = max_h;
    sift_capacities(p, max_w, max_h, max_candidates, max_keypoints, &o->cand_cap, &o->kp_cap);
    o->taps = sift_taps(p);
    const SiftPlan P = sift_plan(p, max_w, max_h);
    if (int rc = o->slab.alloc(who, false, [&](sslam::Slab& S) { sift_bind(o.get(), P, S); })) return rc;
    hipError_t e = hipMemcpy(o->taps_dev, o->taps.taps.data(), o->taps.taps.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o->sticky, 0, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(o->ctl, 0, sizeof(SiftCtl));
    if (e != hipSuccess) {
        sslam::set_error("%s: tap upload: %s", who, hipGetErrorString(e));
        return 1;
    }
    sslam::ctx_retain(ctx);
    *out = o.release();
    return 0;
}

extern "C" int sslam_sift_destroy(sslam_sift* o) {
    return sslam::destroy_instance(o);
}

extern "C" int sslam_sift_capacity(sslam_sift* o, int* rows, int* candidates) {
    return sslam::feat_capacity("sslam_sift_capacity", o, rows, candidates);
}

extern "C" int sslam_sift_overflow(sslam_sift* o, int* word) {
    return sslam::feat_overflow("sslam_sift_overflow", o, word);
}

extern "C" int sslam_sift_detect_dev(sslam_sift* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev, float* aux_out_dev,
                                     int32_t* octave_out_dev, float* desc_out_dev, int32_t* n_out_dev) {
    const char* who = "sslam_sift_detect_dev";
    if (int rc = feat_check_call(who, o, img_dev, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out_dev && aux_out_dev && octave_out_dev && desc_out_dev && n_out_dev, "%s: an output pointer is NULL", who);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    return sift_enqueue(o, img_dev, h, w, c, xy_out_dev, aux_out_dev, octave_out_dev, desc_out_dev, n_out_dev);
}

extern "C" int sslam_sift_detect_host(sslam_sift* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out,
                                      int32_t* octave_out, float* desc_out, int32_t* n_out) {
    const char* who = "sslam_sift_detect_host";
    if (int rc = feat_check_call(who, o, img, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out && aux_out && octave_out && desc_out && n_out, "%s: an output pointer is NULL", who);
    return sslam::feat_detect_host(
        who, o, img, h, w, c, "extrema",
        [&](const uint8_t* img_dev) { return sift_enqueue(o, img_dev, h, w, c, o->xy, o->aux, o->oct, o->desc, o->n); },
        {feat_rows(xy_out, o->xy, 2), feat_rows(aux_out, o->aux, 3), feat_rows(octave_out, o->oct, 1), feat_rows(desc_out, o->desc, SIFT_DESCR_LEN)},
        n_out);
}

extern "C" int sslam_sift_octave_info(sslam_sift* o, int octave, int* info8) {
    const char* who = "sslam_sift_octave_info";
    SSLAM_REQUIRE(o != nullptr && info8 != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(o->have_plan, "%s: no frame has been processed", who);
    SSLAM_REQUIRE(octave >= 0 && octave < SIFT_MAX_OCTAVES, "%s: octave %d outside 0..%d", who, octave, SIFT_MAX_OCTAVES - 1);
    const SiftOctave& O = o->plan.oc[octave];
    const bool on = octave < o->plan.noct;
    const int v[8] = {on ? O.w : 0, on ? O.h : 0, o->plan.noct, o->p.nol + 3, on && O.tx > 0, o->plan.threshold, o->cand_cap, o->kp_cap};
    for (int i = 0; i < 8; ++i) info8[i] = v[i];
    return 0;
}

extern "C" int sslam_sift_stage_read(sslam_sift* o, int octave, float* gauss, float* dog, int32_t* cand, int32_t* ref, float* hist,
                                     int32_t* counts) {
    const char* who = "sslam_sift_stage_read";
    SSLAM_REQUIRE(o != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(o->have_plan, "%s: no frame has been processed", who);
    SSLAM_REQUIRE(octave >= 0 && octave < o->plan.noct, "%s: octave %d is not among the %d computed octaves", who, octave, o->plan.noct);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    const SiftOctave& O = o->plan.oc[octave];
    hipStream_t s = o->ctx->stream;
    const size_t plane = (size_t)O.w * O.h;
    if (gauss) SSLAM_HIP_CHECK(sslam::copy_down(s, gauss, o->gauss + O.goff, plane * (o->p.nol + 3)));
    if (dog) SSLAM_HIP_CHECK(sslam::copy_down(s, dog, o->dog + O.doff, plane * (o->p.nol + 2)));
    SiftCtl ctl;
    SSLAM_HIP_CHECK(sslam::copy_down(s, &ctl, o->ctl, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    const size_t n = (size_t)std::min(ctl.ncand, o->cand_cap);
    if (counts) { counts[0] = ctl.ncand; counts[1] = ctl.nkp; counts[2] = ctl.nout; counts[3] = 0; }
    if (n > 0) {
        if (cand) SSLAM_HIP_CHECK(sslam::copy_down(s, cand, o->cand, n * 4));
        if (ref) SSLAM_HIP_CHECK(sslam::copy_down(s, ref, o->ref, n * 8));
        if (hist) SSLAM_HIP_CHECK(sslam::copy_down(s, hist, o->hist, n * 40));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}
