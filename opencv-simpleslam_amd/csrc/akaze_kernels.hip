// akaze_kernels.hip - AKAZE on the GPU: `cv2.AKAZE_create(DESCRIPTOR_MLDB, 0, 3, threshold, nOctaves, nOctaveLayers, DIFF_PM_G2,
// max_points).detectAndCompute(img, None)` for 8-bit images.
//
// The third detector of the reference's OpenCV branch (`--detector akaze`, `_get_opencv_detector` at
// slam/core/features_utils.py:33-55); it produces what sslam_bf_match_dev consumes with NORM_HAMMING and D = 61 and what the
// Hamming branch of the 2D-3D association takes: uint8 rows of 61 bytes and a device count.  Semantics: tests/akaze_ref.py
// restates OpenCV's AKAZEFeatures stage by stage and lists what could not be confirmed without cv2; the kernels equal it bit for
// bit.  THE DEFINED ARITHMETIC: float32, one IEEE operation at a time in the order of the restatement (contraction is off for the
// whole file); sqrt is correctly rounded (sqrtf in this build); cos and sin are the float64 function rounded once; fastAtan2 is ORB's polynomial; the
// refinement's 2 x 2 solve is float64 on the float32 entries.  Filter taps are added in ascending order through a float32
// intermediate; the orientation windows and the M-LDB cell sums are 64-bit integers at the plan's fixed-point scale (LDS atomics),
// exact and order-free - a stated departure from OpenCV's build-dependent float accumulation.  Suppression is a predicate over
// the candidates of the same and the adjacent levels, not a scan.  THE ORDER of the output: class_id, candidate row, column.
//
// Everything the host decides is in akaze_plan.hpp.  A frame of n levels with S FED steps on the levels above AKZ_WG_PIXELS is
//   1 memset of the control block
//   1 akz_grey_kernel                   grey (15-bit BGR2GRAY) / 255
//   2 + 2 blurs, akz_kgrad / akz_khist / akz_kfinal    level 0 and kcontrast: the Scharr magnitude's maximum (an integer atomic on
//                                       the float's bits), its 300-bin histogram (LDS bins, one merge), every octave's k
//   per further level: akz_halve_kernel at a new octave, then EITHER 2 blurs + akz_flow_kernel + one akz_step_kernel per FED
//                                       step (ping-pong between the level's plane and a temporary; no grid-wide barrier) OR one
//                                       akz_level_wg_kernel: blur, flow and ALL steps in one workgroup with Lt and Lflow in LDS
//   per level: 2 blurs, akz_deriv_kernel (Lx, Ly), akz_det_kernel (Ldet)
//   1 akz_cand_kernel                   all levels: threshold, strict 3 x 3 maximum inside the border, one append per wavefront
//   1 akz_suppress_kernel               a candidate per wavefront: the suppression predicate, then the 2-D refinement -> a keypoint
//   1 akz_quota_kernel                  retainBest(max_points) as a counting predicate, ties kept
//   1 akz_orient_kernel                 a kept keypoint per wavefront: 109 samples, 42 windows, integer sums
//   1 akz_describe_kernel               a kept keypoint per wavefront: its rank in the output order, the 29 cells, 486 bits, 61 bytes
// with every count on the device and no synchronisation.
// MEMORY SAFETY: a candidate is at least border = 2 sigma_size + 1 >= 5 pixels inside its level, so the refinement's reads at +-1
// are inside; blurs clamp and derivatives reflect every tap into the plane; orientation and descriptor samples are range-checked
// against the level before the read; LDS cell and bin indices are bounded by construction (bins are clamped to 299).  A list
// index is checked against its capacity before the store; the counters keep counting, and a frame whose count exceeds a
// capacity is voided (count 0, the sticky overflow word), never truncated.  A descriptor row is written as 61 single bytes.
// PARITY UNPINNED: cv2 is absent here; tests/akaze_ref.py names what could not be confirmed.
#include "common.hpp"
#include "feat_device.hpp"
#include "feat_host.hpp"
#include "geom_common.hpp"
#include "akaze_plan.hpp"

#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#pragma clang fp contract(off)

namespace {

using namespace sslam;

constexpr int AKZ_T = 256;
constexpr int AKZ_WAVES = AKZ_T / 64;
constexpr int AKZ_MAX_TAPS = 9;
constexpr int AKZ_CELLS = 4 + 9 + 16;
constexpr int AKZ_ORI_GRID = 13 * 13;

struct AkzCtl {                                  // zeroed at the head of every call
    int32_t ncand, nkp, nout, hmax_bits;         // the counters keep counting beyond the capacities
    uint32_t hist[AKZ_NBINS];
    float kc[AKZ_MAX_OCTAVES];
};

struct AkzTaps { int n; float t[AKZ_MAX_TAPS]; };

struct AkzLevDev {
    int w, h, border, tx, ty, octave;
    float size, radius, ratio, half;
    long long off;
};

struct AkzArgs {
    int nlev, cand_cap, kp_cap, max_points;
    float threshold;
    AkzConsts k;
    float *Lt, *Lx, *Ly, *Ldet;
    int32_t* cand;                               // [cand_cap][4] level, r, c, response (float32 bits)
    int32_t* cflag;                              // [cand_cap] 0: suppressed, 1: a keypoint, 2: survives, the refinement rejects it
    uint32_t* kp;                                // [kp_cap][8] x, y, size, angle, response (float32 bits), octave, class_id, candidate
    unsigned long long* kkey;                    // [kp_cap] the order key: class_id, row, column
    int32_t* kflag;                              // [kp_cap] 1: kept by the quota
    AkzCtl* ctl;
    int32_t* sticky;
    float* xy_out; float* aux_out; int32_t* lvl_out; uint8_t* desc_out; int32_t* n_out;
    AkzLevDev lv[AKZ_MAX_LEVELS];
};

__device__ __forceinline__ int akz_clamp(int i, int n) { return min(max(i, 0), n - 1); }

// ---- grey, the blurs, the halving -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AKZ_T) void akz_grey_kernel(const uint8_t* __restrict__ src, int w, int h, int C, float* __restrict__ dst) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* s = src + ((size_t)y * w + x) * C;
    dst[(size_t)y * w + x] = (float)bgr_to_grey(s, C) / 255.f;
}

// acc = 0; for k ascending: acc = acc + tap_k * px_k, the product and the sum each rounded; BORDER_REPLICATE
__device__ __forceinline__ float akz_blur_row_at(const float* src, int w, int x, int y, const AkzTaps& T) {
    const float* row = src + (size_t)y * w;
    const int r = T.n >> 1;
    float acc = 0.f;
    for (int k = 0; k < T.n; ++k) { const float t = T.t[k] * row[akz_clamp(x - r + k, w)]; acc = acc + t; }
    return acc;
}

__device__ __forceinline__ float akz_blur_col_at(const float* src, int w, int h, int x, int y, const AkzTaps& T) {
    const int r = T.n >> 1;
    float acc = 0.f;
    for (int k = 0; k < T.n; ++k) { const float t = T.t[k] * src[(size_t)akz_clamp(y - r + k, h) * w + x]; acc = acc + t; }
    return acc;
}

__global__ __launch_bounds__(AKZ_T) void akz_blur_row_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h, AkzTaps T) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    dst[(size_t)y * w + x] = akz_blur_row_at(src, w, x, y, T);
}

__global__ __launch_bounds__(AKZ_T) void akz_blur_col_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h, AkzTaps T) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    dst[(size_t)y * w + x] = akz_blur_col_at(src, w, h, x, y, T);
}

// the mean of the 2 x 2 block at (2y, 2x): 2x + 1 <= 2 (sw / 2) - 1 < sw, the same for the rows
__device__ __forceinline__ float akz_halve_at(const float* __restrict__ src, int sw, int x, int y) {
    const float* p = src + (size_t)(2 * y) * sw + 2 * x;
    const float t0 = p[0] + p[1], t1 = p[sw] + p[sw + 1];
    return (t0 + t1) * 0.25f;
}

__global__ __launch_bounds__(AKZ_T) void akz_halve_kernel(const float* __restrict__ src, int sw, float* __restrict__ dst, int w, int h) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    dst[(size_t)y * w + x] = akz_halve_at(src, sw, x, y);
}

// ---- the separable Scharr form at reach s with smoothing taps (a, b, a), BORDER_REFLECT_101 ---------------------------------------
// x: the row pass differentiates (p[+s] - p[-s]), the column pass smooths; y: the row pass smooths, the column pass differentiates
__device__ __forceinline__ float akz_dx(const float* p, int w, int h, int x, int y, int s, float a, float b) {
    const int xm = reflect101(x - s, w), xp = reflect101(x + s, w);
    const float* r0 = p + (size_t)reflect101(y - s, h) * w;
    const float* r1 = p + (size_t)y * w;
    const float* r2 = p + (size_t)reflect101(y + s, h) * w;
    const float d0 = r0[xp] - r0[xm], d1 = r1[xp] - r1[xm], d2 = r2[xp] - r2[xm];
    float acc = a * d0;
    float t = b * d1; acc = acc + t;
    t = a * d2; acc = acc + t;
    return acc;
}

__device__ __forceinline__ float akz_smooth_row(const float* r, int xm, int x, int xp, float a, float b) {
    float acc = a * r[xm];
    float t = b * r[x]; acc = acc + t;
    t = a * r[xp]; acc = acc + t;
    return acc;
}

__device__ __forceinline__ float akz_dy(const float* p, int w, int h, int x, int y, int s, float a, float b) {
    const int xm = reflect101(x - s, w), xp = reflect101(x + s, w);
    const float s0 = akz_smooth_row(p + (size_t)reflect101(y - s, h) * w, xm, x, xp, a, b);
    const float s1 = akz_smooth_row(p + (size_t)reflect101(y + s, h) * w, xm, x, xp, a, b);
    return s1 - s0;
}

__device__ __forceinline__ float akz_mag(float lx, float ly) {
    const float xx = lx * lx, yy = ly * ly;
    return sqrtf(xx + yy);                                     // correctly rounded in this build; the header's __fsqrt_rn is the native sqrt
}

// ---- kcontrast ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int akz_wave_max(int v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// the gradient magnitude of the interior pixels (stored for the histogram) and its maximum: a non-negative float's bits order as integers
__global__ __launch_bounds__(AKZ_T) void akz_kgrad_kernel(const float* __restrict__ sm, int w, int h, float* __restrict__ mag, AkzCtl* ctl) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    int bits = 0;
    if (x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
        const float g = akz_mag(akz_dx(sm, w, h, x, y, 1, 3.f, 10.f), akz_dy(sm, w, h, x, y, 1, 3.f, 10.f));
        mag[(size_t)y * w + x] = g;
        bits = __float_as_int(g);
    }
    bits = akz_wave_max(bits);
    if ((threadIdx.x & 63) == 0 && bits > ctl->hmax_bits) atomicMax(&ctl->hmax_bits, bits);      // (the plain read only spares atomics: the word grows monotonically)
}

__global__ __launch_bounds__(AKZ_T) void akz_khist_kernel(const float* __restrict__ mag, int w, int h, AkzCtl* ctl) {
    __shared__ uint32_t s_bins[AKZ_NBINS];
    for (int i = threadIdx.x; i < AKZ_NBINS; i += AKZ_T) s_bins[i] = 0u;
    __syncthreads();
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    const float hmax = __int_as_float(ctl->hmax_bits);
    if (hmax > 0.f && x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
        const float g = mag[(size_t)y * w + x];
        if (g != 0.f) {
            const int bin = min((int)floorf((float)AKZ_NBINS * (g / hmax)), AKZ_NBINS - 1);
            atomicAdd(&s_bins[max(bin, 0)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < AKZ_NBINS; i += AKZ_T)
        if (s_bins[i]) atomicAdd(&ctl->hist[i], s_bins[i]);
}

__global__ void akz_kfinal_kernel(AkzCtl* ctl, AkzConsts K) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float hmax = __int_as_float(ctl->hmax_bits);
    float kc = K.kfallback;
    if (hmax > 0.f) {
        long long npoints = 0;
        for (int i = 0; i < AKZ_NBINS; ++i) npoints += ctl->hist[i];
        const long long nthreshold = (long long)((double)npoints * AKZ_KCONTRAST_PERCENTILE);
        long long nelements = 0;
        int k = 0;
        for (; nelements < nthreshold && k < AKZ_NBINS; ++k) nelements += ctl->hist[k];
        if (!(nelements < nthreshold)) kc = hmax * ((float)k / (float)AKZ_NBINS);
    }
    for (int o = 0; o < AKZ_MAX_OCTAVES; ++o) { ctl->kc[o] = kc; kc = kc * K.koctave; }
}

// ---- the conductivity and the diffusion step --------------------------------------------------------------------------------------
__device__ __forceinline__ float akz_flow_at(const float* sm, int w, int h, int x, int y, float k2) {
    const float lx = akz_dx(sm, w, h, x, y, 1, 3.f, 10.f), ly = akz_dy(sm, w, h, x, y, 1, 3.f, 10.f);
    const float xx = lx * lx, yy = ly * ly;
    const float q = (xx + yy) / k2;
    return 1.f / (1.f + q);
}

__global__ __launch_bounds__(AKZ_T) void akz_flow_kernel(const float* __restrict__ sm, int w, int h, const AkzCtl* __restrict__ ctl, int octave,
                                                         float* __restrict__ flow) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float k = ctl->kc[octave];
    flow[(size_t)y * w + x] = akz_flow_at(sm, w, h, x, y, k * k);
}

// L + (0.5 tau) (((xpos - xneg) + ypos) - yneg); a neighbour outside the plane is the pixel itself, its flux an exact zero
__device__ __forceinline__ float akz_step_at(const float* L, const float* C, int w, int h, int x, int y, float half_tau) {
    const size_t i = (size_t)y * w + x;
    const size_t ixp = x + 1 < w ? i + 1 : i, ixm = x > 0 ? i - 1 : i, iyp = y + 1 < h ? i + w : i, iym = y > 0 ? i - w : i;
    const float l = L[i], c = C[i];
    const float xpos = (c + C[ixp]) * (L[ixp] - l), xneg = (C[ixm] + c) * (l - L[ixm]);
    const float ypos = (c + C[iyp]) * (L[iyp] - l), yneg = (C[iym] + c) * (l - L[iym]);
    float s = xpos - xneg;
    s = s + ypos;
    s = s - yneg;
    const float st = half_tau * s;
    return l + st;
}

__global__ __launch_bounds__(AKZ_T) void akz_step_kernel(const float* __restrict__ L, const float* __restrict__ C, float* __restrict__ out, int w, int h,
                                                         float tau) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    out[(size_t)y * w + x] = akz_step_at(L, C, w, h, x, y, 0.5f * tau);
}

// A level of at most AKZ_WG_PIXELS pixels in ONE workgroup: Lt (from `src`) and, in turn, the row pass's intermediate, Lsmooth and
// Lflow in LDS; every phase computes a thread's pixels into registers, a barrier, the store, a barrier - the same per-pixel
// arithmetic as the kernels above in place of 3 + n launches that each cost more than their work.
__global__ __launch_bounds__(AKZ_WG_T) void akz_level_wg_kernel(const float* __restrict__ src, int w, int h, AkzTaps T, const AkzCtl* __restrict__ ctl,
                                                                int octave, const float* __restrict__ taus, int nsteps, float* __restrict__ flow_out,
                                                                float* __restrict__ lt_out) {
    extern __shared__ float akz_lds[];
    const int npx = w * h, tid = threadIdx.x;
    if (npx > AKZ_WG_PIXELS) return;                           // (the plan never sends one)
    float* s_L = akz_lds;
    float* s_C = akz_lds + npx;
    float r[AKZ_WG_PER_THREAD];
    int py[AKZ_WG_PER_THREAD];                                 // the row of pixel tid + q AKZ_WG_T
#pragma unroll
    for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) py[q] = (tid + q * AKZ_WG_T) / w;
    for (int i = tid; i < npx; i += AKZ_WG_T) s_L[i] = src[i];
    __syncthreads();
    for (int i = tid; i < npx; i += AKZ_WG_T) { const int y = i / w; s_C[i] = akz_blur_row_at(s_L, w, i - y * w, y, T); }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
        const int i = tid + q * AKZ_WG_T;
        if (i < npx) { const int y = py[q]; r[q] = akz_blur_col_at(s_C, w, h, i - y * w, y, T); }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
        const int i = tid + q * AKZ_WG_T;
        if (i < npx) s_C[i] = r[q];
    }
    __syncthreads();
    const float k = ctl->kc[octave], k2 = k * k;
#pragma unroll
    for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
        const int i = tid + q * AKZ_WG_T;
        if (i < npx) { const int y = py[q]; r[q] = akz_flow_at(s_C, w, h, i - y * w, y, k2); }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
        const int i = tid + q * AKZ_WG_T;
        if (i < npx) { s_C[i] = r[q]; flow_out[i] = r[q]; }
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const float half_tau = 0.5f * taus[st];
#pragma unroll
        for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
            const int i = tid + q * AKZ_WG_T;
            if (i < npx) { const int y = py[q]; r[q] = akz_step_at(s_L, s_C, w, h, i - y * w, y, half_tau); }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < AKZ_WG_PER_THREAD; ++q) {
            const int i = tid + q * AKZ_WG_T;
            if (i < npx) s_L[i] = r[q];
        }
        __syncthreads();
    }
    for (int i = tid; i < npx; i += AKZ_WG_T) lt_out[i] = s_L[i];
}

// ---- the response ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AKZ_T) void akz_deriv_kernel(const float* __restrict__ sm, int w, int h, int s, float a, float b, float* __restrict__ lx,
                                                          float* __restrict__ ly) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    lx[(size_t)y * w + x] = akz_dx(sm, w, h, x, y, s, a, b);
    ly[(size_t)y * w + x] = akz_dy(sm, w, h, x, y, s, a, b);
}

__global__ __launch_bounds__(AKZ_T) void akz_det_kernel(const float* __restrict__ lx, const float* __restrict__ ly, int w, int h, int s, float a, float b,
                                                        float quat, float* __restrict__ det) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * AKZ_WAVES + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const float lxx = akz_dx(lx, w, h, x, y, s, a, b), lxy = akz_dy(lx, w, h, x, y, s, a, b), lyy = akz_dy(ly, w, h, x, y, s, a, b);
    const float p0 = lxx * lyy, p1 = lxy * lxy;
    det[(size_t)y * w + x] = (p0 - p1) * quat;
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AKZ_T) void akz_cand_kernel(AkzArgs a) {
    const int l = blockIdx.y;
    const AkzLevDev L = a.lv[l];
    if ((int)blockIdx.x >= L.tx * L.ty) return;                // (a level without an interior has no tile)
    const int lane = threadIdx.x & 63;
    const int x = ((int)blockIdx.x % L.tx) * AKZ_TILE_W + lane, y = ((int)blockIdx.x / L.tx) * AKZ_TILE_H + (threadIdx.x >> 6);
    bool is = false;
    float v = 0.f;
    if (x >= L.border && x < L.w - L.border && y >= L.border && y < L.h - L.border) {
        const float* c = a.Ldet + L.off + (size_t)y * L.w + x;
        v = c[0];
        if (v > a.threshold) {
            is = true;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) is = is && v > c[dy * L.w + dx];
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
            q[0] = l; q[1] = y; q[2] = x; q[3] = __float_as_int(v);
        }
    }
}

// ---- suppression and refinement: a candidate per wavefront -----------------------------------------------------------------------
__global__ __launch_bounds__(AKZ_T) __attribute__((target("no-packed-fp32-ops"))) void akz_suppress_kernel(AkzArgs a) {
    if (a.ctl->ncand > a.cand_cap) return;                     // (voided)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.ctl->ncand;
    for (int i = blockIdx.x * AKZ_WAVES + wave; i < n; i += gridDim.x * AKZ_WAVES) {
        const int32_t* me = a.cand + 4 * (size_t)i;
        const int lvl = me[0], r = me[1], c = me[2];
        const float resp = __int_as_float(me[3]);
        const AkzLevDev L = a.lv[lvl];
        const float px = (float)c * L.ratio + L.half, py = (float)r * L.ratio + L.half, r2 = L.radius * L.radius;
        bool hit = false;
        for (int j = lane; j < n; j += 64) {
            const int4 q = reinterpret_cast<const int4*>(a.cand)[j];       // (a record is 16 bytes and the list 256-byte aligned)
            const int ql = q.x, qr = q.y, qc = q.z;
            if (j == i || ql < lvl - 1 || ql > lvl + 1) continue;
            const float qresp = __int_as_float(q.w);
            const float qratio = a.lv[ql].ratio, qhalf = a.lv[ql].half;
            const float dx = ((float)qc * qratio + qhalf) - px, dy = ((float)qr * qratio + qhalf) - py;
            const float xx = dx * dx, yy = dy * dy;
            const bool lower = ql < lvl || (ql == lvl && (qr < r || (qr == r && qc < c)));
            hit = hit || ((xx + yy) <= r2 && (qresp > resp || (qresp == resp && lower)));
        }
        const bool dropped = __ballot(hit) != 0ull;
        if (lane != 0) continue;
        if (dropped) { a.cflag[i] = 0; continue; }
        // the 2-D refinement on Ldet
        const float* D = a.Ldet + L.off + (size_t)r * L.w + c;
        const int w = L.w;
        const float Dx = 0.5f * (D[1] - D[-1]), Dy = 0.5f * (D[w] - D[-w]);
        const float c2 = 2.f * D[0];
        const float Dxx = (D[1] + D[-1]) - c2, Dyy = (D[w] + D[-w]) - c2;
        const float d0 = 0.25f * (D[w + 1] + D[-w - 1]), d1 = 0.25f * (D[-w + 1] + D[w - 1]);
        const float Dxy = d0 - d1;
        const double a00 = Dxx, a01 = Dxy, a11 = Dyy, b0 = -(double)Dx, b1 = -(double)Dy;
        const double m0 = a00 * a11, m1 = a01 * a01, det = m0 - m1;
        bool ok = det != 0.0;
        float ox = 0.f, oy = 0.f;
        if (ok) {
            const double d = 1.0 / det;
            const double n0 = b0 * a11, n1 = b1 * a01, n2 = b1 * a00, n3 = b0 * a01;
            ox = (float)((n0 - n1) * d); oy = (float)((n2 - n3) * d);
            ok = fabsf(ox) <= 1.f && fabsf(oy) <= 1.f;
        }
        a.cflag[i] = ok ? 1 : 2;
        if (!ok) continue;
        const int k = atomicAdd(&a.ctl->nkp, 1);
        if (k < a.kp_cap) {
            uint32_t* o = a.kp + 8 * (size_t)k;
            const float fx = ((float)c + ox) * L.ratio + L.half, fy = ((float)r + oy) * L.ratio + L.half;
            o[0] = __float_as_uint(fx); o[1] = __float_as_uint(fy); o[2] = __float_as_uint(L.size); o[3] = 0u;
            o[4] = (uint32_t)me[3]; o[5] = (uint32_t)L.octave; o[6] = (uint32_t)lvl; o[7] = (uint32_t)i;
            a.kkey[k] = ((unsigned long long)lvl << 40) | ((unsigned long long)r << 20) | (unsigned long long)c;
        }
    }
}

__global__ __launch_bounds__(AKZ_T) void akz_quota_kernel(AkzArgs a) {
    if (feat_voided(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.ctl->nkp;
    for (int j = blockIdx.x * AKZ_WAVES + wave; j < n; j += gridDim.x * AKZ_WAVES) {
        int above = 0;
        if (a.max_points > 0) {
            const float mine = __uint_as_float(a.kp[8 * (size_t)j + 4]);
            for (int i = lane; i < n; i += 64) above += __uint_as_float(a.kp[8 * (size_t)i + 4]) > mine;
            above = wave_sum(above);
        }
        const bool kept = a.max_points <= 0 || above < a.max_points;
        if (lane == 0) {
            a.kflag[j] = kept ? 1 : 0;
            if (kept) atomicAdd(&a.ctl->nout, 1);
        }
    }
}

// ---- the main orientation: a kept keypoint per wavefront -------------------------------------------------------------------------
struct AkzGauss { float g[7][7]; };

__global__ __launch_bounds__(AKZ_T) __attribute__((target("no-packed-fp32-ops"))) void akz_orient_kernel(AkzArgs a, AkzGauss G) {
    __shared__ long long s_fx[AKZ_WAVES][AKZ_ORI_GRID], s_fy[AKZ_WAVES][AKZ_ORI_GRID];
    __shared__ float s_ang[AKZ_WAVES][AKZ_ORI_GRID];
    if (feat_voided(a)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.ctl->nkp;
    const AkzConsts& K = a.k;
    for (int j = blockIdx.x * AKZ_WAVES + wave; j < n; j += gridDim.x * AKZ_WAVES) {
        if (!a.kflag[j]) continue;                             // (uniform)
        uint32_t* rec = a.kp + 8 * (size_t)j;
        const AkzLevDev L = a.lv[rec[6]];
        const float xf = __uint_as_float(rec[0]) / L.ratio, yf = __uint_as_float(rec[1]) / L.ratio;
        const int s = (int)rintf((0.5f * __uint_as_float(rec[2])) / L.ratio);
        const float* LX = a.Lx + L.off;
        const float* LY = a.Ly + L.off;
        for (int e = lane; e < AKZ_ORI_GRID; e += 64) {
            const int i = e / 13 - 6, jj = e - (e / 13) * 13 - 6;
            float ang = -1.f;                                  // (no window takes it)
            long long fx = 0, fy = 0;
            if (i * i + jj * jj < 36) {
                const int iy = (int)rintf(yf + (float)(jj * s)), ix = (int)rintf(xf + (float)(i * s));
                if (iy >= 0 && iy < L.h && ix >= 0 && ix < L.w) {
                    const float gw = G.g[abs(i)][abs(jj)];
                    const float rx = gw * LX[(size_t)iy * L.w + ix], ry = gw * LY[(size_t)iy * L.w + ix];
                    ang = fast_atan2_deg(K.atan, ry, rx) * K.atan.deg2rad;
                    fx = to_fixed<AKZ_FIXED_LOG2>(rx); fy = to_fixed<AKZ_FIXED_LOG2>(ry);
                }
            }
            s_fx[wave][e] = fx; s_fy[wave][e] = fy; s_ang[wave][e] = ang;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        float best = -1.f, sxf = 0.f, syf = 0.f;
        if (lane < AKZ_N_WINDOWS) {
            const float a1 = K.win_step * (float)lane;
            float a2 = a1 + K.pi3;
            if (a2 > K.two_pi) a2 = a1 - K.five_pi3;
            long long sx = 0, sy = 0;
            for (int e = 0; e < AKZ_ORI_GRID; ++e) {
                const float ang = s_ang[wave][e];
                const bool in = a1 < a2 ? (a1 < ang && ang < a2) : ((ang > 0.f && ang < a2) || (ang > a1 && ang < K.two_pi));
                if (in) { sx += s_fx[wave][e]; sy += s_fy[wave][e]; }
            }
            sxf = from_fixed<AKZ_FIXED_LOG2>(sx); syf = from_fixed<AKZ_FIXED_LOG2>(sy);
            const float xx = sxf * sxf, yy = syf * syf;
            best = xx + yy;
        }
        // the first window with the largest value, and only a value above 0
        float bv = best;
        int bw = lane;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_xor(bv, o);
            const int ow = __shfl_xor(bw, o);
            if (ov > bv || (ov == bv && ow < bw)) { bv = ov; bw = ow; }
        }
        const float angle = fast_atan2_deg(K.atan, syf, sxf);
        const float win = __shfl(angle, bw);
        if (lane == 0) rec[3] = __float_as_uint(bv > 0.f ? win : 0.f);
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- M-LDB: a kept keypoint per wavefront ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AKZ_T) __attribute__((target("no-packed-fp32-ops"))) void akz_describe_kernel(AkzArgs a) {
    __shared__ unsigned long long s_acc[AKZ_WAVES][AKZ_CELLS][3];
    __shared__ int s_cnt[AKZ_WAVES][AKZ_CELLS];
    __shared__ float s_val[AKZ_WAVES][AKZ_CELLS][3];
    __shared__ uint32_t s_bits[AKZ_WAVES][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool voided = feat_voided(a);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.n_out[0] = voided ? 0 : a.ctl->nout;
        if (voided) atomicOr(a.sticky, (a.ctl->ncand > a.cand_cap ? 1 : 0) | (a.ctl->nkp > a.kp_cap ? 2 : 0));
    }
    if (voided) return;
    const int n = a.ctl->nkp;
    const AkzConsts& K = a.k;
    for (int j = blockIdx.x * AKZ_WAVES + wave; j < n; j += gridDim.x * AKZ_WAVES) {
        if (!a.kflag[j]) continue;                             // (uniform)
        const unsigned long long key = a.kkey[j];
        int less = 0;
        for (int i = lane; i < n; i += 64) less += a.kflag[i] && a.kkey[i] < key;
        const int pos = wave_sum(less);
        const uint32_t* rec = a.kp + 8 * (size_t)j;
        const AkzLevDev L = a.lv[rec[6]];
        const float x = __uint_as_float(rec[0]), y = __uint_as_float(rec[1]), size = __uint_as_float(rec[2]), angle = __uint_as_float(rec[3]);
        const float xf = x / L.ratio, yf = y / L.ratio;
        const float scale = (float)(int)rintf((0.5f * size) / L.ratio);
        const float rad = angle * K.atan.deg2rad;
        const float co = (float)cos((double)rad), si = (float)sin((double)rad);
        const float* LT = a.Lt + L.off;
        const float* LX = a.Lx + L.off;
        const float* LY = a.Ly + L.off;
        if (lane < AKZ_CELLS) { s_acc[wave][lane][0] = 0ull; s_acc[wave][lane][1] = 0ull; s_acc[wave][lane][2] = 0ull; s_cnt[wave][lane] = 0; }
        if (lane < 16) s_bits[wave][lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        int cell0 = 0;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int cells = g + 2, step = g == 0 ? 10 : (g == 1 ? 7 : 5), side = cells * step;
            for (int e = lane; e < side * side; e += 64) {
                const int kk = e / side, ll = e - kk * side;
                const float fk = (float)(kk - 10), fl = (float)(ll - 10);
                const float y0 = (fl * co) * scale, y1 = (fk * si) * scale, x0 = ((-fl) * si) * scale, x1 = (fk * co) * scale;
                const float sy = yf + (y0 + y1), sx = xf + (x0 + x1);
                const int iy = (int)rintf(sy), ix = (int)rintf(sx);
                if (iy < 0 || iy >= L.h || ix < 0 || ix >= L.w) continue;
                const size_t at = (size_t)iy * L.w + ix;
                const float ri = LT[at], rx = LX[at], ry = LY[at];
                const float t0 = rx * co, t1 = ry * si, t2 = (-rx) * si, t3 = ry * co;
                const float rry = t0 + t1, rrx = t2 + t3;
                const int cell = cell0 + (kk / step) * cells + ll / step;          // < AKZ_CELLS: kk, ll < cells * step
                atomicAdd(&s_acc[wave][cell][0], (unsigned long long)to_fixed<AKZ_FIXED_LOG2>(ri));
                atomicAdd(&s_acc[wave][cell][1], (unsigned long long)to_fixed<AKZ_FIXED_LOG2>(rrx));
                atomicAdd(&s_acc[wave][cell][2], (unsigned long long)to_fixed<AKZ_FIXED_LOG2>(rry));
                atomicAdd(&s_cnt[wave][cell], 1);
            }
            cell0 += cells * cells;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (lane < AKZ_CELLS) {
            const int cnt = s_cnt[wave][lane];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s_val[wave][lane][ch] = cnt > 0 ? from_fixed<AKZ_FIXED_LOG2>((long long)s_acc[wave][lane][ch]) / (float)cnt : 0.f;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int b = lane; b < AKZ_DESC_BITS; b += 64) {
            // bit b: grid, then channel, then the pairs i < j of the grid's cells
            const int g = b < 18 ? 0 : (b < 126 ? 1 : 2);
            const int first = g == 0 ? 0 : (g == 1 ? 18 : 126), cbase = g == 0 ? 0 : (g == 1 ? 4 : 13), cnt = (g + 2) * (g + 2);
            const int npairs = cnt * (cnt - 1) / 2;
            const int ch = (b - first) / npairs;
            int p = (b - first) - ch * npairs, i = 0;
            while (i < cnt - 2 && p >= cnt - 1 - i) { p -= cnt - 1 - i; ++i; }
            const int jj = i + 1 + p;                          // < cnt
            if (s_val[wave][cbase + i][ch] > s_val[wave][cbase + jj][ch]) atomicOr(&s_bits[wave][b >> 5], 1u << (b & 31));
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        if (lane < AKZ_DESC_BYTES) a.desc_out[(size_t)pos * AKZ_DESC_BYTES + lane] = (uint8_t)((s_bits[wave][lane >> 2] >> (8 * (lane & 3))) & 255u);
        if (lane == 0) {
            a.xy_out[2 * (size_t)pos] = x; a.xy_out[2 * (size_t)pos + 1] = y;
            a.aux_out[3 * (size_t)pos] = size; a.aux_out[3 * (size_t)pos + 1] = angle; a.aux_out[3 * (size_t)pos + 2] = __uint_as_float(rec[4]);
            a.lvl_out[2 * (size_t)pos] = (int32_t)rec[5]; a.lvl_out[2 * (size_t)pos + 1] = (int32_t)rec[6];
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

struct sslam_akaze {
    sslam_ctx* ctx = nullptr;
    AkzParams p;
    int max_w = 0, max_h = 0, cand_cap = 0, kp_cap = 0;
    AkzPlan plan{};                              // of the last call (stage_read reads it)
    bool have_plan = false;
    AkzFed fed;
    AkzTaps t16{}, t1{};
    sslam::OwnedSlab slab;
    float *Lt = nullptr, *Lflow = nullptr, *Lx = nullptr, *Ly = nullptr, *Ldet = nullptr;
    float *img = nullptr, *sm = nullptr, *row = nullptr, *pp = nullptr, *half = nullptr, *fed_dev = nullptr;
    int32_t *cand = nullptr, *cflag = nullptr, *kflag = nullptr, *sticky = nullptr;
    uint32_t* kp = nullptr;
    unsigned long long* kkey = nullptr;
    AkzCtl* ctl = nullptr;
    float *xy = nullptr, *aux = nullptr;         // outputs of the host entry
    int32_t *lvl = nullptr, *n = nullptr;
    uint8_t* desc = nullptr;
};

namespace {

// the slab-backed pointers of the instance, in slab order; P: the plan of the largest frame
void akaze_bind(sslam_akaze* o, const AkzPlan& P, sslam::Slab& S) {
    const size_t nc = (size_t)o->cand_cap, nk = (size_t)o->kp_cap, planes = (size_t)std::max(P.plane_floats, 1LL), tmp = (size_t)P.tmp_floats;
    o->Lt = S.take<float>(planes);
    o->Lflow = S.take<float>(planes);
    o->Lx = S.take<float>(planes);
    o->Ly = S.take<float>(planes);
    o->Ldet = S.take<float>(planes);
    o->img = S.take<float>(tmp);
    o->sm = S.take<float>(tmp);
    o->row = S.take<float>(tmp);
    o->pp = S.take<float>(tmp);
    o->half = S.take<float>(tmp);
    o->fed_dev = S.take<float>(std::max<size_t>(o->fed.tau.size(), 1));
    o->cand = S.take<int32_t>(4 * nc);
    o->cflag = S.take<int32_t>(nc);
    o->kp = S.take<uint32_t>(8 * nk);
    o->kkey = S.take<unsigned long long>(nk);
    o->kflag = S.take<int32_t>(nk);
    o->ctl = S.take<AkzCtl>(1);
    o->sticky = S.take<int32_t>(1);
    o->xy = S.take<float>(2 * nk);
    o->aux = S.take<float>(3 * nk);
    o->lvl = S.take<int32_t>(2 * nk);
    o->desc = S.take<uint8_t>(AKZ_DESC_BYTES * nk);
    o->n = S.take<int32_t>(1);
}

AkzTaps akaze_taps(double sigma) {
    const std::vector<float> t = akz_gauss_taps(sigma);
    AkzTaps T{};
    T.n = (int)std::min<size_t>(t.size(), AKZ_MAX_TAPS);
    for (int i = 0; i < T.n; ++i) T.t[i] = t[i];
    return T;
}

int akaze_enqueue(sslam_akaze* o, const uint8_t* img_dev, int h, int w, int c, float* xy, float* aux, int32_t* lvl, uint8_t* desc, int32_t* n_out) {
    const AkzPlan P = akz_plan(o->p, w, h);
    o->plan = P; o->have_plan = true;
    hipStream_t s = o->ctx->stream;
    (void)hipGetLastError();
    SSLAM_HIP_CHECK(hipMemsetAsync(o->ctl, 0, sizeof(AkzCtl), s));
    if (!P.interior) {                                         // no pixel of level 0 inside its border
        SSLAM_HIP_CHECK(hipMemsetAsync(n_out, 0, sizeof(int32_t), s));
        return 0;
    }
    AkzArgs a{};
    a.nlev = P.nlev; a.cand_cap = o->cand_cap; a.kp_cap = o->kp_cap; a.max_points = o->p.max_points; a.threshold = (float)o->p.threshold;
    a.k = akz_consts();
    a.Lt = o->Lt; a.Lx = o->Lx; a.Ly = o->Ly; a.Ldet = o->Ldet; a.cand = o->cand; a.cflag = o->cflag; a.kp = o->kp; a.kkey = o->kkey; a.kflag = o->kflag;
    a.ctl = o->ctl; a.sticky = o->sticky; a.xy_out = xy; a.aux_out = aux; a.lvl_out = lvl; a.desc_out = desc; a.n_out = n_out;
    for (int i = 0; i < P.nlev; ++i) {
        const AkzLevel& L = P.lv[i];
        a.lv[i] = AkzLevDev{L.w, L.h, L.border, L.tx, L.ty, L.octave, L.size, L.radius, L.ratio, L.half, L.off};
    }
    auto grid = [](int gw, int gh) { return dim3(cdiv(gw, 64), cdiv(gh, AKZ_WAVES)); };
    auto blur = [&](const float* src, float* dst, int bw, int bh, const AkzTaps& T) {
        hipLaunchKernelGGL(akz_blur_row_kernel, grid(bw, bh), dim3(AKZ_T), 0, s, src, o->row, bw, bh, T);
        hipLaunchKernelGGL(akz_blur_col_kernel, grid(bw, bh), dim3(AKZ_T), 0, s, (const float*)o->row, dst, bw, bh, T);
    };
    hipLaunchKernelGGL(akz_grey_kernel, grid(w, h), dim3(AKZ_T), 0, s, img_dev, w, h, c, o->img);
    blur(o->img, o->Lt + P.lv[0].off, w, h, o->t16);
    blur(o->img, o->sm, w, h, o->t1);
    hipLaunchKernelGGL(akz_kgrad_kernel, grid(w, h), dim3(AKZ_T), 0, s, (const float*)o->sm, w, h, o->pp, o->ctl);
    hipLaunchKernelGGL(akz_khist_kernel, grid(w, h), dim3(AKZ_T), 0, s, (const float*)o->pp, w, h, o->ctl);
    hipLaunchKernelGGL(akz_kfinal_kernel, dim3(1), dim3(64), 0, s, o->ctl, a.k);
    for (int i = 1; i < P.nlev; ++i) {
        const AkzLevel &L = P.lv[i], &Q = P.lv[i - 1];
        const float* src = o->Lt + Q.off;
        if (L.octave != Q.octave) {
            hipLaunchKernelGGL(akz_halve_kernel, grid(L.w, L.h), dim3(AKZ_T), 0, s, src, Q.w, o->half, L.w, L.h);
            src = o->half;
        }
        float* lt = o->Lt + L.off;
        float* fl = o->Lflow + L.off;
        const int nst = o->fed.n[i];
        const float* taus = o->fed.tau.data() + o->fed.off[i];
        if (L.one_wg) {
            hipLaunchKernelGGL(akz_level_wg_kernel, dim3(1), dim3(AKZ_WG_T), 8 * (size_t)L.w * L.h, s, src, L.w, L.h, o->t1, (const AkzCtl*)o->ctl, L.octave,
                               (const float*)(o->fed_dev + o->fed.off[i]), nst, fl, lt);
            continue;
        }
        blur(src, o->sm, L.w, L.h, o->t1);
        hipLaunchKernelGGL(akz_flow_kernel, grid(L.w, L.h), dim3(AKZ_T), 0, s, (const float*)o->sm, L.w, L.h, (const AkzCtl*)o->ctl, L.octave, fl);
        for (int j = 0; j < nst; ++j) {                        // the last step writes the level's plane
            float* dst = (nst - 1 - j) % 2 == 0 ? lt : o->pp;
            hipLaunchKernelGGL(akz_step_kernel, grid(L.w, L.h), dim3(AKZ_T), 0, s, src, (const float*)fl, dst, L.w, L.h, taus[j]);
            src = dst;
        }
    }
    for (int i = 0; i < P.nlev; ++i) {
        const AkzLevel& L = P.lv[i];
        blur(o->Lt + L.off, o->sm, L.w, L.h, o->t1);
        hipLaunchKernelGGL(akz_deriv_kernel, grid(L.w, L.h), dim3(AKZ_T), 0, s, (const float*)o->sm, L.w, L.h, L.sigma_size, L.norm, L.wnorm, o->Lx + L.off,
                           o->Ly + L.off);
        hipLaunchKernelGGL(akz_det_kernel, grid(L.w, L.h), dim3(AKZ_T), 0, s, (const float*)(o->Lx + L.off), (const float*)(o->Ly + L.off), L.w, L.h,
                           L.sigma_size, L.norm, L.wnorm, L.quat, o->Ldet + L.off);
    }
    AkzGauss G{};
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j) G.g[i][j] = AKZ_GAUSS25[i][j];
    hipLaunchKernelGGL(akz_cand_kernel, dim3(P.max_tiles, P.nlev), dim3(AKZ_T), 0, s, a);
    hipLaunchKernelGGL(akz_suppress_kernel, dim3(AKZ_KP_GX), dim3(AKZ_T), 0, s, a);
    hipLaunchKernelGGL(akz_quota_kernel, dim3(AKZ_KP_GX), dim3(AKZ_T), 0, s, a);
    hipLaunchKernelGGL(akz_orient_kernel, dim3(AKZ_KP_GX), dim3(AKZ_T), 0, s, a, G);
    hipLaunchKernelGGL(akz_describe_kernel, dim3(AKZ_KP_GX), dim3(AKZ_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int sslam_akaze_create(sslam_ctx* ctx, int max_w, int max_h, int descriptor_type, int descriptor_size, int descriptor_channels,
                                  double threshold, int n_octaves, int n_octave_layers, int diffusivity, int max_points, int max_candidates,
                                  int max_keypoints, sslam_akaze** out) {
    const char* who = "sslam_akaze_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    AkzParams p;
    p.descriptor_type = descriptor_type; p.descriptor_size = descriptor_size; p.descriptor_channels = descriptor_channels; p.threshold = threshold;
    p.noct = n_octaves; p.nol = n_octave_layers; p.diffusivity = diffusivity; p.max_points = max_points;
    char msg[160];
    if (akz_check_params(p, max_w, max_h, msg, sizeof msg)) { sslam::set_error("%s: %s", who, msg); return 2; }
    SSLAM_REQUIRE(max_candidates >= 0 && max_keypoints >= 0, "%s: max_candidates %d / max_keypoints %d is negative (0: the default)", who,
                  max_candidates, max_keypoints);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_akaze> o(new sslam_akaze);
    o->ctx = ctx; o->p = p; o->max_w = max_w; o->max_h = max_h;
    akz_capacities(p, max_w, max_h, max_candidates, max_keypoints, &o->cand_cap, &o->kp_cap);
    o->fed = akz_fed(p);
    o->t16 = akaze_taps(AKZ_SOFFSET); o->t1 = akaze_taps(1.0);
    const AkzPlan P = akz_plan(p, max_w, max_h);
    if (int rc = o->slab.alloc(who, false, [&](sslam::Slab& S) { akaze_bind(o.get(), P, S); })) return rc;
    hipError_t e = hipSuccess;
    if (!o->fed.tau.empty()) e = hipMemcpy(o->fed_dev, o->fed.tau.data(), o->fed.tau.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o->sticky, 0, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemset(o->ctl, 0, sizeof(AkzCtl));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)akz_level_wg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * AKZ_WG_PIXELS);
    if (e != hipSuccess) {
        sslam::set_error("%s: step table upload: %s", who, hipGetErrorString(e));
        return 1;
    }
    sslam::ctx_retain(ctx);
    *out = o.release();
    return 0;
}

extern "C" int sslam_akaze_destroy(sslam_akaze* o) {
    return sslam::destroy_instance(o);
}

extern "C" int sslam_akaze_capacity(sslam_akaze* o, int* rows, int* candidates) {
    return sslam::feat_capacity("sslam_akaze_capacity", o, rows, candidates);
}

extern "C" int sslam_akaze_overflow(sslam_akaze* o, int* word) {
    return sslam::feat_overflow("sslam_akaze_overflow", o, word);
}

extern "C" int sslam_akaze_detect_dev(sslam_akaze* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev, float* aux_out_dev,
                                      int32_t* lvl_out_dev, uint8_t* desc_out_dev, int32_t* n_out_dev) {
    const char* who = "sslam_akaze_detect_dev";
    if (int rc = feat_check_call(who, o, img_dev, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out_dev && aux_out_dev && lvl_out_dev && desc_out_dev && n_out_dev, "%s: an output pointer is NULL", who);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    return akaze_enqueue(o, img_dev, h, w, c, xy_out_dev, aux_out_dev, lvl_out_dev, desc_out_dev, n_out_dev);
}

extern "C" int sslam_akaze_detect_host(sslam_akaze* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out, int32_t* lvl_out,
                                       uint8_t* desc_out, int32_t* n_out) {
    const char* who = "sslam_akaze_detect_host";
    if (int rc = feat_check_call(who, o, img, h, w, c)) return rc;
    SSLAM_REQUIRE(xy_out && aux_out && lvl_out && desc_out && n_out, "%s: an output pointer is NULL", who);
    return sslam::feat_detect_host(
        who, o, img, h, w, c, "candidates",
        [&](const uint8_t* img_dev) { return akaze_enqueue(o, img_dev, h, w, c, o->xy, o->aux, o->lvl, o->desc, o->n); },
        {feat_rows(xy_out, o->xy, 2), feat_rows(aux_out, o->aux, 3), feat_rows(lvl_out, o->lvl, 2), feat_rows(desc_out, o->desc, AKZ_DESC_BYTES)},
        n_out);
}

extern "C" int sslam_akaze_level_info(sslam_akaze* o, int level, int* info12) {
    const char* who = "sslam_akaze_level_info";
    SSLAM_REQUIRE(o != nullptr && info12 != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(o->have_plan, "%s: no frame has been processed", who);
    SSLAM_REQUIRE(level >= 0 && level < AKZ_MAX_LEVELS, "%s: level %d outside 0..%d", who, level, AKZ_MAX_LEVELS - 1);
    const AkzLevel& L = o->plan.lv[level];
    const bool on = level < o->plan.nlev;
    const int v[12] = {on ? L.w : 0, on ? L.h : 0, o->plan.nlev, o->plan.noct, on ? L.octave : 0, on ? L.sigma_size : 0, on ? L.border : 0,
                       on ? L.one_wg : 0, on ? o->fed.n[level] : 0, o->plan.interior, o->cand_cap, o->kp_cap};
    for (int i = 0; i < 12; ++i) info12[i] = v[i];
    return 0;
}

extern "C" int sslam_akaze_stage_read(sslam_akaze* o, int level, float* lt, float* lflow, float* lx, float* ly, float* ldet, float* kcontrast8,
                                      int32_t* cand, int32_t* cflag, uint32_t* kp, int32_t* kflag, int32_t* counts) {
    const char* who = "sslam_akaze_stage_read";
    SSLAM_REQUIRE(o != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(o->have_plan && o->plan.interior, "%s: no frame with an interior has been processed", who);
    SSLAM_REQUIRE(level >= 0 && level < o->plan.nlev, "%s: level %d is not among the %d computed levels", who, level, o->plan.nlev);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    const AkzLevel& L = o->plan.lv[level];
    hipStream_t s = o->ctx->stream;
    const size_t plane = (size_t)L.w * L.h;
    if (lt) SSLAM_HIP_CHECK(sslam::copy_down(s, lt, o->Lt + L.off, plane));
    if (lflow && level > 0) SSLAM_HIP_CHECK(sslam::copy_down(s, lflow, o->Lflow + L.off, plane));
    if (lx) SSLAM_HIP_CHECK(sslam::copy_down(s, lx, o->Lx + L.off, plane));
    if (ly) SSLAM_HIP_CHECK(sslam::copy_down(s, ly, o->Ly + L.off, plane));
    if (ldet) SSLAM_HIP_CHECK(sslam::copy_down(s, ldet, o->Ldet + L.off, plane));
    AkzCtl ctl;
    SSLAM_HIP_CHECK(sslam::copy_down(s, &ctl, o->ctl, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (kcontrast8)
        for (int i = 0; i < AKZ_MAX_OCTAVES; ++i) kcontrast8[i] = ctl.kc[i];
    if (counts) { counts[0] = ctl.ncand; counts[1] = ctl.nkp; counts[2] = ctl.nout; counts[3] = 0; }
    const size_t nc = (size_t)std::min(ctl.ncand, o->cand_cap), nk = (size_t)std::min(ctl.nkp, o->kp_cap);
    if (nc > 0) {
        if (cand) SSLAM_HIP_CHECK(sslam::copy_down(s, cand, o->cand, nc * 4));
        if (cflag && ctl.ncand <= o->cand_cap) SSLAM_HIP_CHECK(sslam::copy_down(s, cflag, o->cflag, nc));
    }
    if (nk > 0 && ctl.ncand <= o->cand_cap) {
        if (kp) SSLAM_HIP_CHECK(sslam::copy_down(s, kp, o->kp, nk * 8));
        if (kflag && ctl.nkp <= o->kp_cap) SSLAM_HIP_CHECK(sslam::copy_down(s, kflag, o->kflag, nk));
    }
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
