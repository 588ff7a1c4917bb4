// triangulate_kernels.hip - two-view triangulation of a keyframe pair's matches with the reference's gates.
//
// Replaces the numeric body of `triangulate_between_kfs_2view` (slam/core/triangulation_utils.py:143-271): the
// `cv2.triangulatePoints` call (:152), the homogeneous test (:153-159), the world-frame parallax of
// `_angle_parallax_deg_batch` (:54-77), the depth / cheirality / reprojection gates (:189-249) and the selection of the
// matches that become landmarks, in match order.  Everything is fp64, one match per thread:
//   * P = K T[:3,:] for both views, the 4 x 4 DLT matrix of OpenCV 4.x's triangulate.cpp (rows x P[2] - P[0], y P[2] - P[1]
//     per view), its null vector from a ONE-SIDED (Hestenes) Jacobi SVD of A itself, as OpenCV's JacobiSVD does - never
//     from A^T A, whose condition number is the square (the low-parallax pairs are the ones the gates must judge);
//   * the sweep cap (30, OpenCV's) and the rotation order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) are fixed and a match's
//     arithmetic involves no other match, so a result does not depend on the launch shape (dlt_svd.hpp, shared with
//     relative_pose_kernels.hip);
//   * one reason per match, decided in the reference's order: invalid_w, low_parallax, bad_depth, behind_cam, high_reproj,
//     else kept (the reference's `continue`s).
// PARITY UNPINNED: cv2 is absent here; tests/triangulate_ref.py restates the reference with LAPACK's SVD.
//
// Two launches: a wide one (a match per thread: the Jacobi sweeps are a serial fp64 chain of a few thousand operations per
// match, 4096 of them on one CU would take four turns of a full workgroup) and a one-workgroup tail that compacts the kept
// matches in order (sslam::block_compact) and sums the reason counters.
#include "common.hpp"
#include "dlt_svd.hpp"
#include "geom_common.hpp"

#include <cfloat>
#include <cmath>

namespace {

constexpr int TR_T = 256;            // threads per workgroup of the per-match launch
constexpr int TR_TAIL_T = 1024;      // the compaction tail: one workgroup, 1024 matches per turn
constexpr int TR_REASONS = 6;

enum : int { TR_KEPT = 0, TR_INVALID_W = 1, TR_LOW_PARALLAX = 2, TR_BAD_DEPTH = 3, TR_BEHIND_CAM = 4, TR_HIGH_REPROJ = 5 };

struct TRArgs {
    int n;                                    // match count, or its bound when n_dev is given
    const int32_t* n_dev;                     // device-resident count, clamped to [0, n]; may be NULL
    const float* xy1; const float* xy2;       // ij == NULL: matched pixels [n][2]; else the keypoint arrays the pairs index
    const int32_t* ij;                        // [n][2] (query, train) or NULL
    const double* T1; const double* T2;       // device [16] row-major camera-from-world
    double K[9], Kinv[9];
    double min_d, max_d, par_min, reproj_max;
    int use_par;
    int32_t* reason;                          // [n]  (scratch, or the caller's diagnostics buffer)
    double* Xall;                             // [n][3] scratch: every valid match's point
    double* diag;                             // [n][5] parallax, z1, z2, e1, e2; may be NULL
    double* X_out; int32_t* idx_out; int32_t* ij_out; int32_t* info_out;
};

__device__ __forceinline__ int tr_n(const TRArgs& a) { return a.n_dev ? min(max(a.n_dev[0], 0), a.n) : a.n; }

// P = K T[:3,:] (row-major 3 x 4)
__device__ __forceinline__ void tr_projection(const double* K, const double* T, double* P) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) P[4 * r + c] = K[3 * r] * T[c] + K[3 * r + 1] * T[4 + c] + K[3 * r + 2] * T[8 + c];
}

// unit ray of pixel (u, v) in the world frame: R^T Kinv (u, v, 1), divided by (norm + 1e-12) as the reference does
__device__ __forceinline__ void tr_world_ray(const double* Kinv, const double* T, double u, double v, double* r) {
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = Kinv[3 * i] * u + Kinv[3 * i + 1] * v + Kinv[3 * i + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = T[i] * c[0] + T[4 + i] * c[1] + T[8 + i] * c[2];
    const double nrm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + 1e-12;
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] /= nrm;
}

// camera-frame point, and the reprojection error against (u, v) when it lies in front (else +inf): triangulation_utils.py:195-209
__device__ __forceinline__ void tr_view(const double* K, const double* T, const double* X, double u, double v, double& z, double& e) {
    const double xc = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
    const double yc = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
    z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
    e = INFINITY;
    if (z > 1e-6) {
        const double xn = xc / z, yn = yc / z;
        const double du = K[0] * xn + K[1] * yn + K[2] - u, dv = K[3] * xn + K[4] * yn + K[5] - v;
        e = sqrt(du * du + dv * dv);
    }
}

// ---- 1. a match per thread: triangulate, gate, one reason --------------------------------------------------------
__global__ __launch_bounds__(TR_T) void tr_match_kernel(TRArgs a) {
    const int n = tr_n(a);
    for (int i = blockIdx.x * TR_T + threadIdx.x; i < n; i += gridDim.x * TR_T) {
        int q = i, t = i;
        if (a.ij) { q = a.ij[2 * i]; t = a.ij[2 * i + 1]; }
        const double u1 = a.xy1[2 * q], v1 = a.xy1[2 * q + 1], u2 = a.xy2[2 * t], v2 = a.xy2[2 * t + 1];
        double P1[12], P2[12];
        tr_projection(a.K, a.T1, P1);
        tr_projection(a.K, a.T2, P2);
        double X4[4];
        sslam::dlt_null_vector(P1, P2, u1, v1, u2, v2, X4);
        const double w = X4[3];
        const bool valid_w = isfinite(w) && fabs(w) > 1e-12;
        double X[3] = {X4[0] / w, X4[1] / w, X4[2] / w};

        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        double par = nan;
        if (a.use_par) {
            double r1[3], r2[3];
            tr_world_ray(a.Kinv, a.T1, u1, v1, r1);
            tr_world_ray(a.Kinv, a.T2, u2, v2, r2);
            const double c = fmin(fmax(r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2], -1.0), 1.0);
            par = acos(c) * (180.0 / M_PI);
        }
        double z1 = nan, z2 = nan, e1 = nan, e2 = nan;
        int reason = TR_INVALID_W;
        if (valid_w) {
            tr_view(a.K, a.T1, X, u1, v1, z1, e1);
            tr_view(a.K, a.T2, X, u2, v2, z2, e2);
            if (a.use_par && par < a.par_min) reason = TR_LOW_PARALLAX;
            else if (!(a.min_d <= z1 && z1 <= a.max_d && a.min_d <= z2 && z2 <= a.max_d)) reason = TR_BAD_DEPTH;
            else if (!(z1 > 1e-6) || !(z2 > 1e-6)) reason = TR_BEHIND_CAM;
            else if (fmax(e1, e2) > a.reproj_max) reason = TR_HIGH_REPROJ;
            else reason = TR_KEPT;
        }
        a.reason[i] = reason;
        a.Xall[3 * i] = X[0]; a.Xall[3 * i + 1] = X[1]; a.Xall[3 * i + 2] = X[2];
        if (a.diag) {
            double* d = a.diag + 5 * (size_t)i;
            d[0] = par; d[1] = z1; d[2] = z2; d[3] = e1; d[4] = e2;
        }
    }
}

// ---- 2. the kept matches in match order, the counters (one workgroup) -------------------------------------------
__global__ __launch_bounds__(TR_TAIL_T) void tr_tail_kernel(TRArgs a) {
    __shared__ int wsum[TR_TAIL_T / 64], base;
    __shared__ int sh[TR_TAIL_T];
    __shared__ int totals[8];
    const int n = tr_n(a);
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    int cnt[TR_REASONS] = {0, 0, 0, 0, 0, 0};
    for (int i0 = 0; i0 < n; i0 += TR_TAIL_T) {
        const int i = i0 + threadIdx.x;
        const int reason = i < n ? a.reason[i] : -1;
#pragma unroll
        for (int r = 0; r < TR_REASONS; ++r) cnt[r] += reason == r;
        sslam::block_compact<TR_TAIL_T>(reason == TR_KEPT, wsum, base, [&](int o) {
            a.X_out[3 * o] = a.Xall[3 * i]; a.X_out[3 * o + 1] = a.Xall[3 * i + 1]; a.X_out[3 * o + 2] = a.Xall[3 * i + 2];
            if (a.idx_out) a.idx_out[o] = i;
            if (a.ij_out) {
                a.ij_out[2 * o] = a.ij ? a.ij[2 * i] : i;
                a.ij_out[2 * o + 1] = a.ij ? a.ij[2 * i + 1] : i;
            }
        });
    }
#pragma unroll
    for (int r = 0; r < TR_REASONS; ++r) {
        const int tot = sslam::block_sum<TR_TAIL_T>(cnt[r], sh);
        if ((int)threadIdx.x == r + 1) totals[r + 1] = tot;
    }
    if (threadIdx.x == 0) { totals[0] = base; totals[7] = n; }
    __syncthreads();
    if (threadIdx.x < 8) a.info_out[threadIdx.x] = totals[threadIdx.x];      // one lane per word
}

void tr_enqueue(hipStream_t s, const TRArgs& a) {
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (a.n > 0) hipLaunchKernelGGL(tr_match_kernel, dim3(sslam::cdiv(a.n, TR_T)), dim3(TR_T), 0, s, a);
    hipLaunchKernelGGL(tr_tail_kernel, dim3(1), dim3(TR_TAIL_T), 0, s, a);
}

// K^-1 by cofactors (the reference calls np.linalg.inv on the same 3 x 3)
bool tr_inverse3(const double* m, double* o) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    o[0] = c0 / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = c1 / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = c2 / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}

int tr_fill(TRArgs& a, const char* who, const double* K9, double min_depth, double max_depth, int use_parallax_gate,
            double parallax_min_deg, double reproj_px_max) {
    SSLAM_REQUIRE(K9 != nullptr, "%s: K9 is NULL", who);
    for (int i = 0; i < 9; ++i) a.K[i] = K9[i];
    SSLAM_REQUIRE(tr_inverse3(K9, a.Kinv), "%s: K is singular", who);
    a.min_d = min_depth; a.max_d = max_depth; a.use_par = use_parallax_gate != 0;
    a.par_min = parallax_min_deg; a.reproj_max = reproj_px_max;
    return 0;
}

// the slab-backed pointers of TRArgs, in slab order.  host: the inputs and outputs are the slab's too (T1: both poses, [32])
void tr_bind(sslam::Slab& sl, TRArgs& a, size_t N, bool host, bool diag) {
    a.reason = sl.take<int32_t>(N); a.Xall = sl.take<double>(N * 3);
    if (!host) return;
    a.xy1 = sl.take<float>(N * 2); a.xy2 = sl.take<float>(N * 2); a.T1 = sl.take<double>(32);
    a.X_out = sl.take<double>(N * 3); a.idx_out = sl.take<int32_t>(N); a.info_out = sl.take<int32_t>(8);
    if (diag) a.diag = sl.take<double>(N * 5);
}

}  // namespace

extern "C" int sslam_triangulate_2view_dev(sslam_ctx* ctx, int n_max, const int32_t* n_dev, const float* xy1_dev,
                                           const float* xy2_dev, const int32_t* ij_dev, const double* K9,
                                           const double* T1_dev, const double* T2_dev, double min_depth,
                                           double max_depth, int use_parallax_gate, double parallax_min_deg,
                                           double reproj_px_max, double* X_out_dev, int32_t* ij_out_dev,
                                           int32_t* info_out_dev, int32_t* reason_out_dev, double* diag_out_dev) {
    const char* who = "sslam_triangulate_2view_dev";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n_max >= 1, "%s: n_max %d < 1", who, n_max);
    SSLAM_REQUIRE(xy1_dev && xy2_dev && ij_dev && T1_dev && T2_dev && X_out_dev && info_out_dev, "%s: NULL argument", who);
    TRArgs a{};
    if (int rc = tr_fill(a, who, K9, min_depth, max_depth, use_parallax_gate, parallax_min_deg, reproj_px_max)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { tr_bind(sl, a, (size_t)n_max, false, false); })) return rc;
    a.n = n_max; a.n_dev = n_dev; a.xy1 = xy1_dev; a.xy2 = xy2_dev; a.ij = ij_dev; a.T1 = T1_dev; a.T2 = T2_dev;
    if (reason_out_dev) a.reason = reason_out_dev;
    a.diag = diag_out_dev; a.X_out = X_out_dev; a.ij_out = ij_out_dev; a.info_out = info_out_dev;
    tr_enqueue(ctx->stream, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sslam_triangulate_2view_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2,
                                            const double* K9, const double* T1_16, const double* T2_16,
                                            double min_depth, double max_depth, int use_parallax_gate,
                                            double parallax_min_deg, double reproj_px_max, double* X_out,
                                            int32_t* idx_out, int32_t* info_out, int32_t* reason_out,
                                            double* diag_out) {
    const char* who = "sslam_triangulate_2view_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= 0, "%s: n %d < 0", who, n);
    SSLAM_REQUIRE(T1_16 && T2_16 && info_out, "%s: NULL argument", who);
    SSLAM_REQUIRE(n == 0 || (pts1 && pts2 && X_out && idx_out), "%s: NULL argument", who);
    TRArgs a{};
    if (int rc = tr_fill(a, who, K9, min_depth, max_depth, use_parallax_gate, parallax_min_deg, reproj_px_max)) return rc;
    for (int i = 0; i < 8; ++i) info_out[i] = 0;
    if (n == 0) return 0;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    const bool want_diag = diag_out != nullptr;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { tr_bind(sl, a, N, true, want_diag); })) return rc;
    hipStream_t s = ctx->stream;
    double Ts[32];
    for (int i = 0; i < 16; ++i) { Ts[i] = T1_16[i]; Ts[16 + i] = T2_16[i]; }
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.xy1, pts1, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.xy2, pts2, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.T1, Ts, 32));
    a.n = n; a.T2 = a.T1 + 16;
    tr_enqueue(s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    SSLAM_HIP_CHECK(sslam::copy_down(s, info_out, a.info_out, 8));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));      // (Ts is a stack array: the copy above must have left it; the count sizes the rest)
    const size_t kept = (size_t)info_out[0];
    if (kept) {
        SSLAM_HIP_CHECK(sslam::copy_down(s, X_out, a.X_out, kept * 3));
        SSLAM_HIP_CHECK(sslam::copy_down(s, idx_out, a.idx_out, kept));
    }
    if (reason_out) SSLAM_HIP_CHECK(sslam::copy_down(s, reason_out, a.reason, N));
    if (want_diag) SSLAM_HIP_CHECK(sslam::copy_down(s, diag_out, a.diag, N * 5));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
