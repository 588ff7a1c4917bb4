// stereo_kernels.hip - semi-global stereo matching (cv2.StereoSGBM_create(...).compute, 8-bit, MODE_SGBM, no speckle filter) and the
// lift of keypoints through the disparity to metric 3-D points, on the device.
//
// Replaces the stereo leg of the reference's prototype (refrences/sfm_lightglue_aliked.py:109-121, :357-396): the SGBM call on both
// frames of a pair, the disparity lookup at the matched keypoints and `cv2.triangulatePoints(Proj, Proj_r, ...)`.  All arithmetic
// of the matcher is in integers and every stage equals tests/stereo_ref.py bit for bit (PARITY UNPINNED: never compared with cv2, the
// restatement names what could not be confirmed).  One compute is twelve launches on the context's stream, one more for colour:
//   * sg_grey_kernel       3 or 4 channels -> grey (feat_device.hpp: bgr_to_grey), both images.  NOT cv2's multi-channel cost: the
//                          prototype converts before it calls compute, and so does this.
//   * sg_prefilter_kernel  the clipped horizontal Sobel plane of both images.
//   * sg_rowsum_kernel     Birchfield-Tomasi pixel costs of both planes, summed over the block's row: int16 [H][W1][D], d innermost.
//   * sg_colsum_kernel     the block's column sum as a sliding window down a chunk of rows: C int16 [H][W1][D].
//   * sg_path_kernel<DPL>  one launch per direction (->, <-, down, down-right, down-left).  A path is walked from its border pixel
//                          by a group of min(Dp, 64) lanes, DPL = Dp / lanes disparities each (Dp: D rounded up to a power of
//                          two); the d - 1 / d + 1 neighbours come by lane shuffle, the minimum by a butterfly over the group.
//                          Every (y, x, d) lies on exactly one path of a direction and the directions are separate launches,
//                          so S is a plain read-modify-write (the first direction stores).  The sum saturates at 32767 after
//                          each direction; all terms are non-negative, so that equals saturating once.  The next step's C
//                          and S are loaded before the current step's chain.
//   * sg_select_kernel     16 lanes per pixel: lowest d of the minimum, uniqueness, sub-pixel step; leaves (cost << 8 | d) per pixel.
//   * sg_right_kernel      the right view as a gather over d per right pixel (no atomics): smallest cost, largest x among equals.
//   * sg_check_kernel, sg_median_kernel: the left-right check and the 3 x 3 median over the whole image.
// W1 = W - maxD computed columns; W <= maxD is not an error: every pixel is INVALID and the cost kernels are not launched.
// Every index is formed in size_t from coordinates that were clamped or range-checked first.  Wave size is 64.
#include "common.hpp"
#include "dlt_svd.hpp"
#include "feat_device.hpp"
#include "stereo_plan.hpp"

#include <climits>
#include <cmath>

using sslam::SgbmParams;
using sslam::SgbmPath;

struct sslam_sgbm {
    sslam_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0;
    SgbmParams p{};
    sslam::OwnedSlab slab;
    uint8_t* stage[2] = {nullptr, nullptr};      // the host entry's images [max_h][max_w][4]
    uint8_t* grey[2] = {nullptr, nullptr};
    uint8_t* pf[2] = {nullptr, nullptr};
    int16_t *rows = nullptr, *C = nullptr, *S = nullptr;
    int32_t* key = nullptr;                      // [H][W1]: cost << 8 | d of the accepted pixel, -1 when rejected
    int16_t *raw = nullptr, *right = nullptr, *checked = nullptr, *fin = nullptr;
    int last_h = 0, last_w = 0;
};

namespace {

constexpr int SG_T = sslam::SGBM_PATH_T;      // one workgroup size for every kernel; the plan sizes the path grids with it
constexpr int SG_ROWS = 16;          // rows per thread of the column sum
constexpr int SG_SEL_LANES = 16;     // lanes per pixel of the selection

__global__ __launch_bounds__(SG_T)
void sg_grey_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t n, int C, uint8_t* __restrict__ ga, uint8_t* __restrict__ gb) {
    const size_t i = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (i >= n) return;
    const uint8_t* s = blockIdx.y ? b : a;
    (blockIdx.y ? gb : ga)[i] = (uint8_t)sslam::bgr_to_grey(s + i * (size_t)C, C);
}

__global__ __launch_bounds__(SG_T)
void sg_prefilter_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R, int H, int W, int ftzero, uint8_t* __restrict__ pl,
                         uint8_t* __restrict__ pr) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const uint8_t* I = blockIdx.z ? R : L;
    int v = ftzero;
    if (x >= 1 && x <= W - 2) {
        const uint8_t* r0 = I + (size_t)max(y - 1, 0) * W;
        const uint8_t* r1 = I + (size_t)y * W;
        const uint8_t* r2 = I + (size_t)min(y + 1, H - 1) * W;
        const int g = 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r0[x + 1] - (int)r0[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
        v = min(max(g, -ftzero), ftzero) + ftzero;
    }
    (blockIdx.z ? pr : pl)[(size_t)y * W + x] = (uint8_t)v;
}

// Birchfield-Tomasi of one plane: rows l, r of W pixels, left pixel x against right pixel xr (both inside the row)
__device__ __forceinline__ int sg_bt(const uint8_t* __restrict__ l, const uint8_t* __restrict__ r, int W, int x, int xr) {
    const int u = l[x], ul = (u + (int)l[max(x - 1, 0)]) >> 1, ur = (u + (int)l[min(x + 1, W - 1)]) >> 1;
    const int v = r[xr], vl = (v + (int)r[max(xr - 1, 0)]) >> 1, vr = (v + (int)r[min(xr + 1, W - 1)]) >> 1;
    const int umin = min(u, min(ul, ur)), umax = max(u, max(ul, ur));
    const int vmin = min(v, min(vl, vr)), vmax = max(v, max(vl, vr));
    const int c0 = max(0, max(u - vmax, vmin - u)), c1 = max(0, max(v - umax, umin - v));
    return min(c0, c1) >> 2;
}

// rows[y][xc][d] = sum over the block's row of the pixel cost, columns replicated at the edges of the computed region
__global__ __launch_bounds__(SG_T)
void sg_rowsum_kernel(const uint8_t* __restrict__ L, const uint8_t* __restrict__ R, const uint8_t* __restrict__ pl, const uint8_t* __restrict__ pr,
                      int H, int W, SgbmParams p, int16_t* __restrict__ rows) {
    const int W1 = W - p.maxD;
    const size_t i = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (i >= (size_t)H * W1 * p.D) return;
    const int d = (int)(i % (size_t)p.D);
    const size_t px = i / (size_t)p.D;
    const int xc = (int)(px % (size_t)W1), y = (int)(px / (size_t)W1);
    const size_t row = (size_t)y * W;
    const int rad = p.bs >> 1;
    int sum = 0;
    for (int k = -rad; k <= rad; ++k) {
        const int x = p.maxD + min(max(xc + k, 0), W1 - 1);      // maxD .. W - 1
        const int xr = x - p.minD - d;                           // 1 .. W - 1
        sum += sg_bt(pl + row, pr + row, W, x, xr) + sg_bt(L + row, R + row, W, x, xr);
    }
    rows[i] = (int16_t)sum;
}

// C[y][col] = sum over the block's column of rows[.][col], rows replicated at the top and bottom; col = xc * D + d
__global__ __launch_bounds__(SG_T)
void sg_colsum_kernel(const int16_t* __restrict__ rows, int H, size_t cols, int rad, int16_t* __restrict__ C) {
    const size_t col = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (col >= cols) return;
    const int y0 = blockIdx.y * SG_ROWS, y1 = min(y0 + SG_ROWS, H);
    int sum = 0;
    for (int k = -rad; k <= rad; ++k) sum += rows[(size_t)min(max(y0 + k, 0), H - 1) * cols + col];
    C[(size_t)y0 * cols + col] = (int16_t)sum;
    for (int y = y0 + 1; y < y1; ++y) {
        sum += (int)rows[(size_t)min(y + rad, H - 1) * cols + col] - (int)rows[(size_t)max(y - 1 - rad, 0) * cols + col];
        C[(size_t)y * cols + col] = (int16_t)sum;
    }
}

// One direction.  Lanes gl = 0 .. LG - 1 of a group hold disparities gl * DPL .. gl * DPL + DPL - 1 of their path; a slot at or
// beyond D (D is no power of two) keeps the out-of-range value 32767, is left out of the minimum and touches no memory.
template <int DPL>
__global__ __launch_bounds__(SG_T)
void sg_path_kernel(const int16_t* __restrict__ C, int16_t* __restrict__ S, int H, int W1, int D, int dir, int P1, int P2, int first) {
    const int LG = sslam::sgbm_group_lanes(D);                   // 16, 32 or 64; LG * DPL >= D
    const int gl = threadIdx.x & (LG - 1);
    const int path = blockIdx.x * sslam::sgbm_paths_per_block(D) + (int)(threadIdx.x / LG);
    if (path >= sslam::sgbm_path_count(dir, H, W1)) return;      // (a whole group)
    const SgbmPath q = sslam::sgbm_path(dir, path, H, W1);
    const ptrdiff_t step = ((ptrdiff_t)q.dy * W1 + q.dx) * D;
    size_t off = ((size_t)q.y0 * W1 + q.x0) * D + (size_t)gl * DPL;
    bool live[DPL];
    int Lp[DPL], c[DPL], s[DPL];
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
        live[j] = gl * DPL + j < D;
        Lp[j] = live[j] ? 0 : sslam::SGBM_MAX_COST;
        c[j] = live[j] ? (int)C[off + j] : 0;
        s[j] = live[j] && !first ? (int)S[off + j] : 0;
    }
    int m = 0;
    for (int k = 0; k < q.len; ++k) {
        int cn[DPL], sn[DPL];
        const size_t offn = (size_t)((ptrdiff_t)off + step);
        const bool more = k + 1 < q.len;                         // the next pixel of the path is inside the region
#pragma unroll
        for (int j = 0; j < DPL; ++j) {
            cn[j] = more && live[j] ? (int)C[offn + j] : 0;
            sn[j] = more && live[j] && !first ? (int)S[offn + j] : 0;
        }
        int lo = __shfl_up(Lp[DPL - 1], 1, LG), hi = __shfl_down(Lp[0], 1, LG);
        if (gl == 0) lo = sslam::SGBM_MAX_COST;
        if (gl == LG - 1) hi = sslam::SGBM_MAX_COST;
        int Ln[DPL], mn = INT_MAX;
#pragma unroll
        for (int j = 0; j < DPL; ++j) {
            const int a = j > 0 ? Lp[j - 1] : lo, b = j < DPL - 1 ? Lp[j + 1] : hi;
            Ln[j] = live[j] ? c[j] + min(min(Lp[j], m + P2), min(a, b) + P1) - m : sslam::SGBM_MAX_COST;
            if (live[j]) mn = min(mn, Ln[j]);
        }
        for (int w = LG >> 1; w > 0; w >>= 1) mn = min(mn, __shfl_xor(mn, w, LG));
        m = mn;
#pragma unroll
        for (int j = 0; j < DPL; ++j) {
            if (live[j]) S[off + j] = (int16_t)min(s[j] + Ln[j], sslam::SGBM_MAX_COST);
            Lp[j] = Ln[j]; c[j] = cn[j]; s[j] = sn[j];
        }
        off = offn;
    }
}

// 16 lanes per pixel of the whole image; lane 0 of the group writes
__global__ __launch_bounds__(SG_T)
void sg_select_kernel(const int16_t* __restrict__ S, int H, int W, SgbmParams p, int16_t* __restrict__ raw, int32_t* __restrict__ key) {
    const int l = threadIdx.x & (SG_SEL_LANES - 1);
    const size_t pix = (size_t)blockIdx.x * (SG_T / SG_SEL_LANES) + threadIdx.x / SG_SEL_LANES;
    if (pix >= (size_t)H * W) return;                            // (a whole group)
    const int x = (int)(pix % (size_t)W), y = (int)(pix / (size_t)W);
    if (x < p.maxD) {
        if (l == 0) raw[pix] = (int16_t)p.invalid;
        return;
    }
    const int W1 = W - p.maxD;
    const size_t cell = (size_t)y * W1 + (x - p.maxD);
    const int16_t* Sp = S + cell * p.D;
    int k = INT_MAX;
    for (int d = l; d < p.D; d += SG_SEL_LANES) k = min(k, ((int)Sp[d] << 8) | d);      // the lowest d of the minimum
    for (int w = SG_SEL_LANES >> 1; w > 0; w >>= 1) k = min(k, __shfl_xor(k, w, SG_SEL_LANES));
    const int minS = k >> 8, best = k & 255;
    int rej = 0;
    for (int d = l; d < p.D; d += SG_SEL_LANES) rej |= (abs(d - best) > 1 && (int)Sp[d] * (100 - p.uniq) < minS * 100) ? 1 : 0;
    for (int w = SG_SEL_LANES >> 1; w > 0; w >>= 1) rej |= __shfl_xor(rej, w, SG_SEL_LANES);
    if (l != 0) return;
    int disp = 16 * best;
    if (best > 0 && best < p.D - 1) {
        const int lo = Sp[best - 1], hi = Sp[best + 1];
        const int den = max(lo + hi - 2 * minS, 1);
        disp += ((lo - hi) * 16 + den) / (2 * den);              // C's truncating division
    }
    raw[pix] = (int16_t)(rej ? p.invalid : disp + 16 * p.minD);
    key[cell] = rej ? -1 : k;
}

// the right view: per right pixel x2 the accepted left pixels x = x2 + minD + d with d* == d, by ascending d (= ascending x)
__global__ __launch_bounds__(SG_T)
void sg_right_kernel(const int32_t* __restrict__ key, int H, int W, SgbmParams p, int16_t* __restrict__ right) {
    const size_t pix = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int x2 = (int)(pix % (size_t)W), y = (int)(pix / (size_t)W);
    const int W1 = W - p.maxD;
    int cost = INT_MAX, out = p.invalid;
    for (int d = 0; d < p.D; ++d) {
        const int x = x2 + p.minD + d;
        if (x >= W) break;
        if (x < p.maxD) continue;
        const int k = key[(size_t)y * W1 + (x - p.maxD)];
        if (k >= 0 && (k & 255) == d && (k >> 8) <= cost) { cost = k >> 8; out = d + p.minD; }
    }
    right[pix] = (int16_t)out;
}

__global__ __launch_bounds__(SG_T)
void sg_check_kernel(const int16_t* __restrict__ raw, const int16_t* __restrict__ right, int H, int W, SgbmParams p, int16_t* __restrict__ checked) {
    const size_t pix = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int x = (int)(pix % (size_t)W);
    const size_t row = pix - (size_t)x;
    const int d1 = raw[pix];
    int out = d1;
    if (x >= p.maxD && d1 != p.invalid) {
        const int da = d1 >> 4, db = (d1 + 15) >> 4;
        const int xa = x - da, xb = x - db;
        bool bad = xa >= 0 && xa < W && xb >= 0 && xb < W;
        if (bad) {
            const int ra = right[row + xa], rb = right[row + xb];
            bad = ra >= p.minD && abs(ra - da) > p.d12 && rb >= p.minD && abs(rb - db) > p.d12;
        }
        if (bad) out = p.invalid;
    }
    checked[pix] = (int16_t)out;
}

__global__ __launch_bounds__(SG_T)
void sg_median_kernel(const int16_t* __restrict__ in, int H, int W, int16_t* __restrict__ out) {
    const size_t pix = (size_t)blockIdx.x * SG_T + threadIdx.x;
    if (pix >= (size_t)H * W) return;
    const int x = (int)(pix % (size_t)W), y = (int)(pix / (size_t)W);
    int v[9];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) v[3 * j + i] = in[(size_t)min(max(y + j - 1, 0), H - 1) * W + min(max(x + i - 1, 0), W - 1)];
#pragma unroll
    for (int a = 0; a < 5; ++a)                                  // five passes of a selection sort leave the median at v[4]
#pragma unroll
        for (int b = a + 1; b < 9; ++b) { const int lo = min(v[a], v[b]), hi = max(v[a], v[b]); v[a] = lo; v[b] = hi; }
    out[pix] = (int16_t)v[4];
}

// ---- the keypoint lift: a keypoint per thread --------------------------------------------------------------------------------
struct LiftArgs {
    int n;                           // keypoint count, or its bound when n_dev is given
    const int32_t* n_dev;            // device-resident count, clamped to [0, n]; may be NULL
    const float* xy;                 // [n][2]
    const float* xy_right_in;        // [n][2] or NULL: the right pixels are given, no disparity lookup
    const int16_t* disp;             // [H][W] sixteenths
    int H, W;
    double Pl[12], Pr[12];
    int have_P;
    float min_disp, max_disp;
    float* d_out; float* xy_right; double* X; uint8_t* mask;
};

__global__ __launch_bounds__(SG_T) void sg_lift_kernel(LiftArgs a) {
    const int n = a.n_dev ? min(max(a.n_dev[0], 0), a.n) : a.n;
    const int i = blockIdx.x * SG_T + threadIdx.x;
    if (i >= n) return;
    const float x = a.xy[2 * i], y = a.xy[2 * i + 1];
    const float nanf_ = __int_as_float(0x7fc00000);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    float d = nanf_, xr = nanf_;
    bool ok = false;
    if (a.xy_right_in) {
        xr = a.xy_right_in[2 * i];
        d = x - xr;
        ok = true;
    } else if (x > -1.0f && x < (float)a.W && y > -1.0f && y < (float)a.H) {      // int(): towards zero; a NaN compares false
        d = (float)a.disp[(size_t)(int)y * a.W + (int)x] / 16.0f;
        xr = x - d;
        ok = a.min_disp < d && d < a.max_disp;
    }
    double X[3] = {nan, nan, nan};
    if (ok && a.have_P) {
        double X4[4];
        sslam::dlt_null_vector(a.Pl, a.Pr, (double)x, (double)y, (double)xr, (double)(a.xy_right_in ? a.xy_right_in[2 * i + 1] : y), X4);
        const double w = X4[3];
        if (isfinite(w) && fabs(w) > 1e-12) { X[0] = X4[0] / w; X[1] = X4[1] / w; X[2] = X4[2] / w; }
        else ok = false;
    }
    if (a.d_out) a.d_out[i] = d;
    if (a.xy_right) { a.xy_right[2 * i] = xr; a.xy_right[2 * i + 1] = a.xy_right_in ? a.xy_right_in[2 * i + 1] : y; }
    if (a.X) { a.X[3 * i] = X[0]; a.X[3 * i + 1] = X[1]; a.X[3 * i + 2] = X[2]; }
    a.mask[i] = ok ? 1 : 0;
}

int sg_refuse(const char* who, const char* msg) {
    sslam::set_error("%s: %s", who, msg);
    return 2;
}

int sg_check_pair(const char* who, sslam_sgbm* g, const void* left, const void* right, int H, int W, int C, const void* out) {
    SSLAM_REQUIRE(g != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(left != nullptr && right != nullptr && out != nullptr, "%s: NULL argument", who);
    char msg[160];
    if (sslam::sgbm_check_image(W, H, C, g->max_w, g->max_h, msg, sizeof msg)) return sg_refuse(who, msg);
    return 0;
}

template <int DPL>
void sg_launch_paths(sslam_sgbm* g, int H, int W1, hipStream_t s) {
    const SgbmParams& p = g->p;
    for (int dir = 0; dir < sslam::SGBM_DIRECTIONS; ++dir)
        hipLaunchKernelGGL(sg_path_kernel<DPL>, dim3((unsigned)sslam::sgbm_path_blocks(dir, H, W1, p.D)), dim3(SG_T), 0, s, g->C, g->S, H, W1,
                           p.D, dir, p.P1, p.P2, dir == 0 ? 1 : 0);
}

int sg_enqueue(sslam_sgbm* g, const uint8_t* left, const uint8_t* right, int H, int W, int C, int16_t* out) {
    const SgbmParams& p = g->p;
    hipStream_t s = g->ctx->stream;
    const size_t npix = (size_t)H * W;
    const dim3 block(SG_T), per_pixel((unsigned)((npix + SG_T - 1) / SG_T));
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (C != 1) {
        hipLaunchKernelGGL(sg_grey_kernel, dim3(per_pixel.x, 2), block, 0, s, left, right, npix, C, g->grey[0], g->grey[1]);
        left = g->grey[0]; right = g->grey[1];
    }
    hipLaunchKernelGGL(sg_prefilter_kernel, dim3((unsigned)sslam::cdiv(W, 64), (unsigned)sslam::cdiv(H, 4), 2), block, 0, s, left, right, H, W,
                       p.ftzero, g->pf[0], g->pf[1]);
    const int W1 = W - p.maxD;
    if (W1 > 0) {
        const size_t cols = (size_t)W1 * p.D, vol = (size_t)H * cols;
        hipLaunchKernelGGL(sg_rowsum_kernel, dim3((unsigned)((vol + SG_T - 1) / SG_T)), block, 0, s, left, right, g->pf[0], g->pf[1], H, W, p, g->rows);
        hipLaunchKernelGGL(sg_colsum_kernel, dim3((unsigned)((cols + SG_T - 1) / SG_T), (unsigned)sslam::cdiv(H, SG_ROWS)), block, 0, s, g->rows, H, cols,
                           p.bs >> 1, g->C);
        switch (sslam::sgbm_d_per_lane(p.D)) {
        case 1: sg_launch_paths<1>(g, H, W1, s); break;
        case 2: sg_launch_paths<2>(g, H, W1, s); break;
        default: sg_launch_paths<4>(g, H, W1, s); break;
        }
    }
    hipLaunchKernelGGL(sg_select_kernel, dim3((unsigned)((npix + SG_T / SG_SEL_LANES - 1) / (SG_T / SG_SEL_LANES))), block, 0, s, g->S, H, W, p, g->raw,
                       g->key);
    hipLaunchKernelGGL(sg_right_kernel, per_pixel, block, 0, s, g->key, H, W, p, g->right);
    hipLaunchKernelGGL(sg_check_kernel, per_pixel, block, 0, s, g->raw, g->right, H, W, p, g->checked);
    hipLaunchKernelGGL(sg_median_kernel, per_pixel, block, 0, s, g->checked, H, W, out);
    SSLAM_HIP_CHECK(hipGetLastError());
    g->last_h = H; g->last_w = W;
    return 0;
}

int lift_fill(LiftArgs& a, const char* who, int n, int H, int W, const double* P_left12, const double* P_right12, double min_disp, double max_disp) {
    SSLAM_REQUIRE(n >= 0, "%s: n %d < 0", who, n);
    SSLAM_REQUIRE((P_left12 == nullptr) == (P_right12 == nullptr), "%s: one projection matrix without the other", who);
    a.n = n; a.H = H; a.W = W;
    a.have_P = P_left12 != nullptr;
    for (int i = 0; i < 12; ++i) { a.Pl[i] = a.have_P ? P_left12[i] : 0.0; a.Pr[i] = a.have_P ? P_right12[i] : 0.0; }
    a.min_disp = (float)min_disp; a.max_disp = (float)max_disp;
    return 0;
}

}  // namespace

extern "C" int sslam_sgbm_create(sslam_ctx* ctx, int max_w, int max_h, int minDisparity, int numDisparities, int blockSize, int P1, int P2,
                                 int disp12MaxDiff, int preFilterCap, int uniquenessRatio, int speckleWindowSize, int speckleRange, int mode,
                                 sslam_sgbm** out) {
    const char* who = "sslam_sgbm_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    char msg[200];
    if (sslam::sgbm_check_create(max_w, max_h, minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                                 speckleWindowSize, speckleRange, mode, msg, sizeof msg)) return sg_refuse(who, msg);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_sgbm> g(new sslam_sgbm);
    g->ctx = ctx; g->max_w = max_w; g->max_h = max_h;
    g->p = sslam::sgbm_normalise(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio);
    const sslam::SgbmExtents e = sslam::sgbm_extents(max_w, max_h, g->p.maxD, g->p.D);
    size_t measured = 0;
    if (int rc = g->slab.alloc(who, false, [&](sslam::Slab& S) {
            for (int i = 0; i < 2; ++i) g->stage[i] = S.take<uint8_t>((size_t)e.px * 4);
            for (int i = 0; i < 2; ++i) g->grey[i] = S.take<uint8_t>((size_t)e.px);
            for (int i = 0; i < 2; ++i) g->pf[i] = S.take<uint8_t>((size_t)e.px);
            g->rows = S.take<int16_t>((size_t)e.vol);
            g->C = S.take<int16_t>((size_t)e.vol);
            g->S = S.take<int16_t>((size_t)e.vol);
            g->key = S.take<int32_t>((size_t)max_h * (size_t)e.cols);
            g->raw = S.take<int16_t>((size_t)e.px);
            g->right = S.take<int16_t>((size_t)e.px);
            g->checked = S.take<int16_t>((size_t)e.px);
            g->fin = S.take<int16_t>((size_t)e.px);
            measured = S.bytes;
        })) return rc;
    SSLAM_REQUIRE(measured == (size_t)e.bytes, "%s: the slab took %zu bytes, the plan says %llu", who, measured, e.bytes);
    sslam::ctx_retain(ctx);
    *out = g.release();
    return 0;
}

extern "C" int sslam_sgbm_destroy(sslam_sgbm* g) {
    return sslam::destroy_instance(g);
}

extern "C" int sslam_sgbm_compute_dev(sslam_sgbm* g, const uint8_t* left_dev, const uint8_t* right_dev, int H, int W, int channels,
                                      int16_t* disp_dev) {
    const char* who = "sslam_sgbm_compute_dev";
    if (int rc = sg_check_pair(who, g, left_dev, right_dev, H, W, channels, disp_dev)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(g->ctx->device));
    return sg_enqueue(g, left_dev, right_dev, H, W, channels, disp_dev);
}

extern "C" int sslam_sgbm_compute_host(sslam_sgbm* g, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int16_t* disp) {
    const char* who = "sslam_sgbm_compute_host";
    if (int rc = sg_check_pair(who, g, left, right, H, W, channels, disp)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(g->ctx->device));
    hipStream_t s = g->ctx->stream;
    const size_t n = (size_t)H * W;
    SSLAM_HIP_CHECK(sslam::copy_up(s, g->stage[0], left, n * channels));
    SSLAM_HIP_CHECK(sslam::copy_up(s, g->stage[1], right, n * channels));
    if (int rc = sg_enqueue(g, g->stage[0], g->stage[1], H, W, channels, g->fin)) return rc;
    SSLAM_HIP_CHECK(sslam::copy_down(s, disp, g->fin, n));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_sgbm_stage_read(sslam_sgbm* g, int which, void* dst) {
    const char* who = "sslam_sgbm_stage_read";
    SSLAM_REQUIRE(g != nullptr && dst != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(g->last_h != 0, "%s: no compute yet", who);
    SSLAM_HIP_CHECK(hipSetDevice(g->ctx->device));
    const size_t npix = (size_t)g->last_h * g->last_w;
    const size_t vol = (size_t)g->last_h * (size_t)std::max(g->last_w - g->p.maxD, 0) * g->p.D;
    const void* from = nullptr;
    size_t bytes = 0;
    switch (which) {
    case sslam::SGBM_STAGE_PF_LEFT: from = g->pf[0]; bytes = npix; break;
    case sslam::SGBM_STAGE_PF_RIGHT: from = g->pf[1]; bytes = npix; break;
    case sslam::SGBM_STAGE_C: from = g->C; bytes = vol * sizeof(int16_t); break;
    case sslam::SGBM_STAGE_S: from = g->S; bytes = vol * sizeof(int16_t); break;
    case sslam::SGBM_STAGE_RAW: from = g->raw; bytes = npix * sizeof(int16_t); break;
    case sslam::SGBM_STAGE_RIGHT: from = g->right; bytes = npix * sizeof(int16_t); break;
    case sslam::SGBM_STAGE_CHECKED: from = g->checked; bytes = npix * sizeof(int16_t); break;
    default: SSLAM_REQUIRE(false, "%s: stage %d outside 0..6", who, which);
    }
    hipStream_t s = g->ctx->stream;
    if (bytes) SSLAM_HIP_CHECK(hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_stereo_lift_dev(sslam_ctx* ctx, int n_max, const int32_t* n_dev, const float* xy_dev, const float* xy_right_in_dev,
                                     const int16_t* disp_dev, int H, int W, const double* P_left12, const double* P_right12, double min_disp,
                                     double max_disp, float* d_out_dev, float* xy_right_out_dev, double* X_out_dev, uint8_t* mask_out_dev) {
    const char* who = "sslam_stereo_lift_dev";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n_max >= 1, "%s: n_max %d < 1", who, n_max);
    SSLAM_REQUIRE(xy_dev && mask_out_dev && (xy_right_in_dev || disp_dev), "%s: NULL argument", who);
    SSLAM_REQUIRE(xy_right_in_dev || (H >= 1 && W >= 1 && H <= sslam::SGBM_MAX_SIDE && W <= sslam::SGBM_MAX_SIDE), "%s: image size %dx%d outside 1..%d",
                  who, W, H, sslam::SGBM_MAX_SIDE);
    LiftArgs a{};
    if (int rc = lift_fill(a, who, n_max, H, W, P_left12, P_right12, min_disp, max_disp)) return rc;
    SSLAM_REQUIRE(X_out_dev == nullptr || a.have_P, "%s: X_out without projection matrices", who);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    a.n_dev = n_dev; a.xy = xy_dev; a.xy_right_in = xy_right_in_dev; a.disp = disp_dev;
    a.d_out = d_out_dev; a.xy_right = xy_right_out_dev; a.X = X_out_dev; a.mask = mask_out_dev;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sg_lift_kernel, dim3((unsigned)sslam::cdiv(n_max, SG_T)), dim3(SG_T), 0, ctx->stream, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sslam_stereo_lift_host(sslam_ctx* ctx, int n, const float* xy, const float* xy_right_in, const int16_t* disp, int H, int W,
                                      const double* P_left12, const double* P_right12, double min_disp, double max_disp, float* d_out,
                                      float* xy_right_out, double* X_out, uint8_t* mask_out) {
    const char* who = "sslam_stereo_lift_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    LiftArgs a{};
    if (int rc = lift_fill(a, who, n, H, W, P_left12, P_right12, min_disp, max_disp)) return rc;
    if (n == 0) return 0;
    SSLAM_REQUIRE(xy && mask_out && (xy_right_in || disp), "%s: NULL argument", who);
    SSLAM_REQUIRE(xy_right_in || (H >= 1 && W >= 1 && H <= sslam::SGBM_MAX_SIDE && W <= sslam::SGBM_MAX_SIDE), "%s: image size %dx%d outside 1..%d", who,
                  W, H, sslam::SGBM_MAX_SIDE);
    SSLAM_REQUIRE(X_out == nullptr || a.have_P, "%s: X_out without projection matrices", who);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n, npix = xy_right_in ? 0 : (size_t)H * W;
    float *xy_d = nullptr, *xr_in_d = nullptr, *d_d = nullptr, *xr_d = nullptr;
    int16_t* disp_d = nullptr;
    double* X_d = nullptr;
    uint8_t* mask_d = nullptr;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) {
            xy_d = sl.take<float>(N * 2); xr_in_d = sl.take<float>(N * 2); disp_d = sl.take<int16_t>(npix);
            d_d = sl.take<float>(N); xr_d = sl.take<float>(N * 2); X_d = sl.take<double>(N * 3); mask_d = sl.take<uint8_t>(N);
        })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, xy_d, xy, N * 2));
    if (xy_right_in) SSLAM_HIP_CHECK(sslam::copy_up(s, xr_in_d, xy_right_in, N * 2));
    else SSLAM_HIP_CHECK(sslam::copy_up(s, disp_d, disp, npix));
    a.xy = xy_d; a.xy_right_in = xy_right_in ? xr_in_d : nullptr; a.disp = disp_d;
    a.d_out = d_d; a.xy_right = xr_d; a.X = a.have_P ? X_d : nullptr; a.mask = mask_d;
    (void)hipGetLastError();
    hipLaunchKernelGGL(sg_lift_kernel, dim3((unsigned)sslam::cdiv(n, SG_T)), dim3(SG_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    if (d_out) SSLAM_HIP_CHECK(sslam::copy_down(s, d_out, d_d, N));
    if (xy_right_out) SSLAM_HIP_CHECK(sslam::copy_down(s, xy_right_out, xr_d, N * 2));
    if (X_out) SSLAM_HIP_CHECK(sslam::copy_down(s, X_out, X_d, N * 3));
    SSLAM_HIP_CHECK(sslam::copy_down(s, mask_out, mask_d, N));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
