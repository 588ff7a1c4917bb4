// relative_pose_kernels.hip - two-view relative pose from an essential matrix, and the validation of such a pose.
//
// The F/E leg of the reference's map bootstrap (slam/core/two_view_bootstrap.py:127-220, :314-411) and of the
// tracking-lost fallback (slam/monocular/main_revamped.py:512-514):
//   * sslam_recover_pose_host restates OpenCV 4.x `recoverPose(E, points1, points2, cameraMatrix, R, t, distanceThresh,
//     mask)` (modules/calib3d/src/five-point.cpp): pixels widened to double and normalised (x - cx) / fx, (y - cy) / fy;
//     `decomposeEssentialMat` - the 3 x 3 SVD by the one-sided Jacobi of dlt_svd.hpp, singular values sorted descending,
//     U = -U / Vt = -Vt where a determinant is negative, R1 = U W Vt, R2 = U W^T Vt, t = U[:,2]; the four candidates
//     [R1|t] [R2|t] [R1|-t] [R2|-t] against [I|0], every match triangulated (the shared DLT) and judged by OpenCV's four
//     comparisons; the winner by OpenCV's own >= chain.
//   * sslam_two_view_metrics_host restates `triangulation_metrics` (:127-156) and `_triangulate_points_cv` (:314-326):
//     `cv2.undistortPoints` without distortion ((x - cx) * (1 / fx) in double, rounded to float32 as OpenCV does for
//     float32 input), the DLT against [I|0] and [R|t], X = Xh[:3] / (Xh[3] + 1e-12), the two depths, the angle between
//     the rays from the two camera centres, the fraction in front of both cameras and the median angle in degrees.
// PARITY UNPINNED: cv2 is absent here; tests/relative_pose_ref.py restates both and names what could not be confirmed.
//
// fp64 throughout and no fused multiply-add in this file: the restatement has separate operations.
//
// Launch chains (no host decision inside either; integer sums, so a result does not depend on the launch shape):
//   recover pose   head [one lane: the SVD, the four projection matrices, counters to zero] - wide [a thread per
//                  (match, candidate): DLT, the mask byte; a workgroup's count by block_sum, one integer atomic per
//                  workgroup] - tail [one workgroup: the winner, its mask copied, R / t / info]
//   metrics        head [one workgroup: the selected matches compacted in match order] - wide [a thread per selected
//                  match: X, depths, the angle; the in-front count as above] - tail [one workgroup: the exact median by
//                  a radix selection over the angles' bit patterns, the metrics]
#include "common.hpp"

#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)
#include "dlt_svd.hpp"
#include "geom_common.hpp"

namespace {

constexpr int RP_T = 256;            // threads per workgroup of the wide launches
constexpr int RP_TAIL_T = 1024;      // the one-workgroup launches
constexpr int RP_MAX_SELECTED = 16384;

struct RPArgs {
    int n;
    const float* p1; const float* p2;         // [n][2] pixels
    const unsigned char* mask_in;             // [n] or NULL
    double E[9];
    double fx, fy, cx, cy, thresh;
    double* P;                                // [4][12] the candidates' projection matrices; then R1[9], R2[9], t[3]
    unsigned char* masks;                     // [4][n]
    int32_t* counts;                          // [4]
    double* Rt_out;                           // R[9], t[3]
    unsigned char* mask_out;                  // [n]
    int32_t* info_out;                        // [8]
};

__device__ __forceinline__ double rp_det3(const double (&M)[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

// ---- recover pose 1: decomposeEssentialMat by one lane ----------------------------------------------------------
__global__ __launch_bounds__(64) void rp_head_kernel(RPArgs a) {
    if (threadIdx.x != 0) return;
    double A[3][3], V[3][3];                          // [column][row]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) A[c][r] = a.E[3 * r + c];
    sslam::jacobi_sweeps(A, V);
    double w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = sqrt(A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2]);
    // descending singular values, OpenCV's selection order (the first of equals stays first)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int j = i;
#pragma unroll
        for (int k = i + 1; k < 3; ++k) if (w[j] < w[k]) j = k;
        if (i != j) {
            const double tw = w[i]; w[i] = w[j]; w[j] = tw;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double ta = A[i][r]; A[i][r] = A[j][r]; A[j][r] = ta;
                const double tv = V[i][r]; V[i][r] = V[j][r]; V[j][r] = tv;
            }
        }
    }
    double U[3][3], Vt[3][3];                         // [row][column]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) { U[r][c] = A[c][r] / w[c]; Vt[c][r] = V[c][r]; }
    if (!(w[2] > DBL_MIN)) {
        // a singular value of exactly zero leaves no column to normalise (OpenCV completes the basis there): the third
        // left vector is the cross product of the first two, its sign immaterial below
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
    if (rp_det3(U) < 0)
#pragma unroll
        for (int i = 0; i < 9; ++i) U[i / 3][i % 3] = -U[i / 3][i % 3];
    if (rp_det3(Vt) < 0)
#pragma unroll
        for (int i = 0; i < 9; ++i) Vt[i / 3][i % 3] = -Vt[i / 3][i % 3];
    // U W = [-u1, u0, u2], U W^T = [u1, -u0, u2] (columns)
    double R[2][3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double uw0 = -U[r][1], uw1 = U[r][0], uw2 = U[r][2];
            R[0][r][c] = uw0 * Vt[0][c] + uw1 * Vt[1][c] + uw2 * Vt[2][c];
            R[1][r][c] = (-uw0) * Vt[0][c] + (-uw1) * Vt[1][c] + uw2 * Vt[2][c];
        }
    const double t[3] = {U[0][2], U[1][2], U[2][2]};
#pragma unroll
    for (int cand = 0; cand < 4; ++cand)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.P[12 * cand + 4 * r + c] = R[cand & 1][r][c];
            a.P[12 * cand + 4 * r + 3] = cand < 2 ? t[r] : -t[r];
        }
    double* Rt = a.P + 48;
#pragma unroll
    for (int i = 0; i < 9; ++i) { Rt[i] = R[0][i / 3][i % 3]; Rt[9 + i] = R[1][i / 3][i % 3]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) Rt[18 + i] = t[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) a.counts[i] = 0;
}

// ---- recover pose 2: a thread per (match, candidate) ------------------------------------------------------------
__global__ __launch_bounds__(RP_T) void rp_vote_kernel(RPArgs a) {
    __shared__ int sh[RP_T];
    const int cand = blockIdx.y;
    const int i = blockIdx.x * RP_T + threadIdx.x;
    int nz = 0;
    if (i < a.n) {
        const double x1 = ((double)a.p1[2 * i] - a.cx) / a.fx, y1 = ((double)a.p1[2 * i + 1] - a.cy) / a.fy;
        const double x2 = ((double)a.p2[2 * i] - a.cx) / a.fx, y2 = ((double)a.p2[2 * i + 1] - a.cy) / a.fy;
        const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        double P[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = a.P[12 * cand + k];
        double Q[4];
        sslam::dlt_null_vector(P0, P, x1, y1, x2, y2, Q);
        bool good = Q[2] * Q[3] > 0;
        const double q0 = Q[0] / Q[3], q1 = Q[1] / Q[3], q2 = Q[2] / Q[3], q3 = Q[3] / Q[3];
        good &= q2 < a.thresh;
        const double z = P[8] * q0 + P[9] * q1 + P[10] * q2 + P[11] * q3;
        good &= z > 0;
        good &= z < a.thresh;
        unsigned char m = good ? 255 : 0;
        if (a.mask_in) m &= a.mask_in[i];
        a.masks[(size_t)cand * a.n + i] = m;
        nz = m != 0;
    }
    const int tot = sslam::block_sum<RP_T>(nz, sh);
    if (threadIdx.x == 0 && tot) atomicAdd(a.counts + cand, tot);
}

// ---- recover pose 3: the winner (one workgroup) -----------------------------------------------------------------
__global__ __launch_bounds__(RP_TAIL_T) void rp_tail_kernel(RPArgs a) {
    const int g1 = a.counts[0], g2 = a.counts[1], g3 = a.counts[2], g4 = a.counts[3];
    int win;
    if (g1 >= g2 && g1 >= g3 && g1 >= g4) win = 0;
    else if (g2 >= g1 && g2 >= g3 && g2 >= g4) win = 1;
    else if (g3 >= g1 && g3 >= g2 && g3 >= g4) win = 2;
    else win = 3;
    for (int i = threadIdx.x; i < a.n; i += RP_TAIL_T) a.mask_out[i] = a.masks[(size_t)win * a.n + i];
    const double* Rt = a.P + 48;
    if (threadIdx.x < 9) a.Rt_out[threadIdx.x] = Rt[9 * (win & 1) + threadIdx.x];
    else if (threadIdx.x < 12) a.Rt_out[threadIdx.x] = win < 2 ? Rt[18 + threadIdx.x - 9] : -Rt[18 + threadIdx.x - 9];
    else if (threadIdx.x < 20) {
        const int k = threadIdx.x - 12;
        const int v[8] = {win == 0 ? g1 : win == 1 ? g2 : win == 2 ? g3 : g4, a.n, win, g1, g2, g3, g4, 0};
        a.info_out[k] = v[k];
    }
}

// the slab-backed pointers of RPArgs, in slab order
void rp_bind(sslam::Slab& sl, RPArgs& a, size_t N, bool with_mask) {
    a.p1 = sl.take<float>(N * 2); a.p2 = sl.take<float>(N * 2);
    if (with_mask) a.mask_in = sl.take<unsigned char>(N);
    a.P = sl.take<double>(48 + 21); a.masks = sl.take<unsigned char>(4 * N); a.counts = sl.take<int32_t>(4);
    a.Rt_out = sl.take<double>(12); a.mask_out = sl.take<unsigned char>(N); a.info_out = sl.take<int32_t>(8);
}

// =================================================================================================================
struct TVArgs {
    int n;
    const float* p1; const float* p2;         // [n][2] pixels
    const unsigned char* sel;                 // [n] or NULL: every match
    double ifx, ify, cx, cy;
    double R[9], t[3];
    int32_t* idx;                             // [n] the selected matches in order
    int32_t* cnt;                             // [2] selected, in front of both cameras
    double* ang;                              // [n] arccos of the clipped cosine, per selected match
    double* X;                                // [n][3]
    double* z;                                // [n][2]
    double* metrics_out;                      // [2]
    int32_t* info_out;                        // [4]
};

// ---- metrics 1: the selected matches in match order (one workgroup) ---------------------------------------------
__global__ __launch_bounds__(RP_TAIL_T) void tv_select_kernel(TVArgs a) {
    __shared__ int wsum[RP_TAIL_T / 64], base;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < a.n; i0 += RP_TAIL_T) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < a.n && (!a.sel || a.sel[i] != 0);
        sslam::block_compact<RP_TAIL_T>(keep, wsum, base, [&](int o) { a.idx[o] = i; });
    }
    if (threadIdx.x == 0) { a.cnt[0] = base; a.cnt[1] = 0; }
}

// ---- metrics 2: a thread per selected match ---------------------------------------------------------------------
__global__ __launch_bounds__(RP_T) void tv_point_kernel(TVArgs a) {
    __shared__ int sh[RP_T];
    const int N = a.cnt[0];
    const int o = blockIdx.x * RP_T + threadIdx.x;
    int front = 0;
    if (o < N) {
        const int i = a.idx[o];
        // cv2.undistortPoints on float32 input: double arithmetic, a float32 result
        const double x1 = (double)(float)(((double)a.p1[2 * i] - a.cx) * a.ifx), y1 = (double)(float)(((double)a.p1[2 * i + 1] - a.cy) * a.ify);
        const double x2 = (double)(float)(((double)a.p2[2 * i] - a.cx) * a.ifx), y2 = (double)(float)(((double)a.p2[2 * i + 1] - a.cy) * a.ify);
        const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const double* R = a.R;
        const double P[12] = {R[0], R[1], R[2], a.t[0], R[3], R[4], R[5], a.t[1], R[6], R[7], R[8], a.t[2]};
        double Q[4];
        sslam::dlt_null_vector(P0, P, x1, y1, x2, y2, Q);
        const double w = Q[3] + 1e-12;
        const double X[3] = {Q[0] / w, Q[1] / w, Q[2] / w};
        const double z1 = X[2];
        const double z2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + a.t[2];
        front = z1 > 0 && z2 > 0;
        // v1 = X - 0, v2 = X - (-R^T t)
        double v2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v2[k] = X[k] + (R[k] * a.t[0] + R[3 + k] * a.t[1] + R[6 + k] * a.t[2]);
        const double dot = X[0] * v2[0] + X[1] * v2[1] + X[2] * v2[2];
        const double n1 = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]), n2 = sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
        const double c = fmin(fmax(dot / (n1 * n2 + 1e-12), -1.0), 1.0);
        a.ang[o] = acos(c);
        a.X[3 * (size_t)o] = X[0]; a.X[3 * (size_t)o + 1] = X[1]; a.X[3 * (size_t)o + 2] = X[2];
        a.z[2 * (size_t)o] = z1; a.z[2 * (size_t)o + 1] = z2;
    }
    const int tot = sslam::block_sum<RP_T>(front, sh);
    if (threadIdx.x == 0 && tot) atomicAdd(a.cnt + 1, tot);
}

// a double as an unsigned key of the same order (-0 below +0)
__device__ __forceinline__ unsigned long long tv_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ULL;
}
__device__ __forceinline__ double tv_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k & 0x7fffffffffffffffULL : ~k;
    return __longlong_as_double((long long)b);
}

// The k-th smallest (0-based) of v[0..N) by a most-significant-digit radix selection on the keys, eight bits per pass:
// exact, no copy of the values, the same answer for any workgroup shape.  Every thread calls it and gets the value.
__device__ double tv_select_kth(const double* v, int N, int k, int* hist, unsigned long long* state) {
    unsigned long long prefix = 0, pmask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const unsigned long long key = tv_key(v[i]);
            if ((key & pmask) == prefix) atomicAdd(hist + (int)((key >> shift) & 255), 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int d = 0, below = 0;
            while (d < 255 && below + hist[d] <= k) { below += hist[d]; ++d; }
            state[0] = prefix | ((unsigned long long)d << shift);
            state[1] = (unsigned long long)(k - below);
        }
        __syncthreads();
        prefix = state[0]; k = (int)state[1];
        pmask |= 255ULL << shift;
        __syncthreads();
    }
    return tv_unkey(prefix);
}

// ---- metrics 3: the median angle and the two metrics (one workgroup) --------------------------------------------
__global__ __launch_bounds__(RP_TAIL_T) void tv_tail_kernel(TVArgs a) {
    __shared__ int hist[256];
    __shared__ unsigned long long state[2];
    const int N = a.cnt[0];
    double posdepth = 0, parallax = 0;
    if (N >= 2) {                                                     // (uniform over the workgroup)
        const double hi = tv_select_kth(a.ang, N, N / 2, hist, state);
        double med = hi;
        if ((N & 1) == 0) med = (tv_select_kth(a.ang, N, N / 2 - 1, hist, state) + hi) / 2;
        parallax = med * (180.0 / M_PI);
        posdepth = (double)a.cnt[1] / (double)N;
    }
    if (threadIdx.x == 0) {
        a.metrics_out[0] = posdepth; a.metrics_out[1] = parallax;
        a.info_out[0] = N >= 2 ? N : 0; a.info_out[1] = N >= 2 ? a.cnt[1] : 0; a.info_out[2] = 0; a.info_out[3] = 0;
    }
}

// the slab-backed pointers of TVArgs, in slab order
void tv_bind(sslam::Slab& sl, TVArgs& a, size_t N, bool with_sel) {
    a.p1 = sl.take<float>(N * 2); a.p2 = sl.take<float>(N * 2);
    if (with_sel) a.sel = sl.take<unsigned char>(N);
    a.idx = sl.take<int32_t>(N); a.cnt = sl.take<int32_t>(2); a.ang = sl.take<double>(N); a.X = sl.take<double>(N * 3);
    a.z = sl.take<double>(N * 2);
    a.metrics_out = sl.take<double>(2 + 2);     // metrics[2], then info[4] in the same piece: one read-back
    if (a.metrics_out) a.info_out = reinterpret_cast<int32_t*>(a.metrics_out + 2);
}

}  // namespace

extern "C" int sslam_recover_pose_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, const double* E9,
                                       const double* K9, double distance_thresh, const unsigned char* mask_in,
                                       double* R_out9, double* t_out3, unsigned char* mask_out, int32_t* info_out) {
    const char* who = "sslam_recover_pose_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= 0, "%s: n %d < 0", who, n);
    SSLAM_REQUIRE(E9 && K9 && R_out9 && t_out3 && info_out, "%s: NULL argument", who);
    SSLAM_REQUIRE(n == 0 || (pts1 && pts2 && mask_out), "%s: NULL argument", who);
    SSLAM_REQUIRE(K9[0] != 0 && K9[4] != 0 && std::isfinite(K9[0]) && std::isfinite(K9[4]), "%s: K has no focal length", who);
    RPArgs a{};
    for (int i = 0; i < 9; ++i) a.E[i] = E9[i];
    a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5]; a.thresh = distance_thresh;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    const bool with_mask = mask_in != nullptr && n > 0;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { rp_bind(sl, a, N, with_mask); })) return rc;
    hipStream_t s = ctx->stream;
    if (n) {
        SSLAM_HIP_CHECK(sslam::copy_up(s, a.p1, pts1, N * 2));
        SSLAM_HIP_CHECK(sslam::copy_up(s, a.p2, pts2, N * 2));
        if (with_mask) SSLAM_HIP_CHECK(sslam::copy_up(s, a.mask_in, mask_in, N));
    }
    a.n = n;
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    hipLaunchKernelGGL(rp_head_kernel, dim3(1), dim3(64), 0, s, a);
    if (n) hipLaunchKernelGGL(rp_vote_kernel, dim3(sslam::cdiv(n, RP_T), 4), dim3(RP_T), 0, s, a);
    hipLaunchKernelGGL(rp_tail_kernel, dim3(1), dim3(RP_TAIL_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    double Rt[12];
    SSLAM_HIP_CHECK(sslam::copy_down(s, Rt, a.Rt_out, 12));
    SSLAM_HIP_CHECK(sslam::copy_down(s, info_out, a.info_out, 8));
    if (n) SSLAM_HIP_CHECK(sslam::copy_down(s, mask_out, a.mask_out, N));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    for (int i = 0; i < 9; ++i) R_out9[i] = Rt[i];
    for (int i = 0; i < 3; ++i) t_out3[i] = Rt[9 + i];
    return 0;
}

extern "C" int sslam_two_view_metrics_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2,
                                           const unsigned char* sel, const double* K9, const double* R9,
                                           const double* t3, double* metrics_out, int32_t* info_out, double* X_out,
                                           double* z_out) {
    const char* who = "sslam_two_view_metrics_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= 0, "%s: n %d < 0", who, n);
    SSLAM_REQUIRE(K9 && R9 && t3 && metrics_out && info_out, "%s: NULL argument", who);
    SSLAM_REQUIRE(n == 0 || (pts1 && pts2), "%s: NULL argument", who);
    SSLAM_REQUIRE(K9[0] != 0 && K9[4] != 0 && std::isfinite(K9[0]) && std::isfinite(K9[4]), "%s: K has no focal length", who);
    size_t selected = (size_t)n;              // (sizes the read-back and the refusal below; the device compacts on its own)
    if (sel) {
        selected = 0;
        for (int i = 0; i < n; ++i) selected += sel[i] != 0;
    }
    SSLAM_REQUIRE(selected <= (size_t)RP_MAX_SELECTED, "%s: %zu selected matches, at most %d are supported", who, selected,
                  RP_MAX_SELECTED);
    metrics_out[0] = metrics_out[1] = 0;
    for (int i = 0; i < 4; ++i) info_out[i] = 0;
    if (n == 0) return 0;
    TVArgs a{};
    a.ifx = 1.0 / K9[0]; a.ify = 1.0 / K9[4]; a.cx = K9[2]; a.cy = K9[5];
    for (int i = 0; i < 9; ++i) a.R[i] = R9[i];
    for (int i = 0; i < 3; ++i) a.t[i] = t3[i];
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { tv_bind(sl, a, N, sel != nullptr); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p1, pts1, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p2, pts2, N * 2));
    if (sel) SSLAM_HIP_CHECK(sslam::copy_up(s, a.sel, sel, N));
    a.n = n;
    (void)hipGetLastError();
    hipLaunchKernelGGL(tv_select_kernel, dim3(1), dim3(RP_TAIL_T), 0, s, a);
    hipLaunchKernelGGL(tv_point_kernel, dim3(sslam::cdiv(n, RP_T)), dim3(RP_T), 0, s, a);
    hipLaunchKernelGGL(tv_tail_kernel, dim3(1), dim3(RP_TAIL_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    double out[4];
    SSLAM_HIP_CHECK(sslam::copy_down(s, out, a.metrics_out, 4));
    if (X_out && selected) SSLAM_HIP_CHECK(sslam::copy_down(s, X_out, a.X, selected * 3));
    if (z_out && selected) SSLAM_HIP_CHECK(sslam::copy_down(s, z_out, a.z, selected * 2));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    std::memcpy(metrics_out, out, 16);
    std::memcpy(info_out, out + 2, 16);
    return 0;
}
