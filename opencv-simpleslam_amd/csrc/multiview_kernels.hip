// multiview_kernels.hip - N-view triangulation of feature tracks with the gates of the reference's CLI, and the
// all-pairs-within-a-radius search under landmark fusion.
//
// The module the reference's own tests call (`slam.core.multi_view_utils`: `multi_view_triangulation`,
// `MultiViewTriangulator`) was lost upstream; its contract survives in those tests and in the drivers' knobs
// (`--mvt_rep_err`, `--merge_radius`, `--min_depth`, `--max_depth`).  include/sslam_hip.h states the definition used here.
// PARITY UNPINNED: there is no upstream implementation to compare with; tests/multiview_ref.py restates the definition.
//
// Tracks (fp64, one track per thread, 256 threads per workgroup as in triangulate_kernels.hip: the Jacobi sweeps are a
// serial fp64 chain of a few thousand operations):
//   * P = K Tcw[:3] once per view (mv_proj_kernel), not once per observation;
//   * the DLT matrix A [2V, 4] (rows u P[2] - P[0], v P[2] - P[1]) is never stored: each row is folded by four Givens
//     rotations into the 4 x 4 triangular factor R, which has A's singular values and right singular vectors - so a track
//     has no cap on its views and no memory of its own.  A^T A is never formed: its condition number is the square, and the
//     low-parallax tracks are the ones the gates must judge;
//   * R goes to the one-sided Jacobi of dlt_svd.hpp, the null vector is the column of V under R's column of smallest norm,
//     the first of equals, as `dlt_null_vector` selects it;
//   * a second pass over the track's observations gives the depths and the mean reprojection error;
//   * one reason per track: too_few_views, invalid_w, bad_depth, behind_cam, high_reproj, else kept.
// A track's arithmetic involves no other track and the rotation order is fixed, so a result does not depend on the launch
// shape.  A one-workgroup tail compacts the kept tracks in order (sslam::block_compact) and sums the reason counters.
//
// Pairs: a 2-D grid of 256-point tiles (bi, bj), the lower triangle exits at once; the bj tile sits in LDS (6 KB), each
// thread keeps one i point in registers and tests dx^2 + dy^2 + dz^2 <= r^2 against the tile.  A hit takes a slot from a
// device counter; a hit beyond the buffer is counted, not written, so the count is exact and the caller runs once more
// with a buffer of that size.  The order of the pairs in the buffer is the order of the atomics: the caller sorts.
//
// Multiply-adds do not fuse in this file: a pair's test must depend on its two points only, in either order of the
// operands, and the track arithmetic is then the one tests/multiview_ref.py ports.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)
#include "dlt_svd.hpp"
#include "geom_common.hpp"

namespace {

constexpr int MV_T = 256;            // threads per workgroup of the per-track launch
constexpr int MV_TAIL_T = 1024;      // the compaction tail: one workgroup, 1024 tracks per turn
constexpr int MV_REASONS = 6;
constexpr int CP_T = 256;            // points per tile of the pair search = threads per workgroup

enum : int { MV_KEPT = 0, MV_TOO_FEW_VIEWS = 1, MV_INVALID_W = 2, MV_BAD_DEPTH = 3, MV_BEHIND_CAM = 4, MV_HIGH_REPROJ = 5 };

struct MVArgs {
    int n, F;                                 // tracks, views
    const int32_t* off;                       // [n + 1] CSR offsets into the observations
    const int32_t* view;                      // [M] view of each observation, in [0, F)
    const float* uv;                          // [M][2] pixels
    const double* Tcw;                        // [F][16] row-major camera-from-world
    double* P;                                // [F][12] scratch: K Tcw[:3]
    double K[9];
    double min_d, max_d, err_max;
    int32_t* reason;                          // [n]
    double* Xall;                             // [n][3] scratch: every track's point
    double* diag;                             // [n][3] mean error, z min, z max; may be NULL
    double* X_out; int32_t* idx_out; int32_t* info_out;
};

// ---- 1. P = K Tcw[:3] per view ------------------------------------------------------------------------------------
__global__ __launch_bounds__(MV_T) void mv_proj_kernel(MVArgs a) {
    const int f = blockIdx.x * MV_T + threadIdx.x;
    if (f >= a.F) return;
    const double* T = a.Tcw + 16 * (size_t)f;
    double* P = a.P + 12 * (size_t)f;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) P[4 * r + c] = a.K[3 * r] * T[c] + a.K[3 * r + 1] * T[4 + c] + a.K[3 * r + 2] * T[8 + c];
}

// fold one row of A into the triangular factor R (row-major, upper): four Givens rotations, each zeroing one entry of the row
__device__ __forceinline__ void mv_fold_row(double (&R)[4][4], double (&row)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (row[k] != 0.0) {
            const double r = hypot(R[k][k], row[k]);
            const double c = R[k][k] / r, s = row[k] / r;
#pragma unroll
            for (int j = k; j < 4; ++j) {
                const double t = c * R[k][j] + s * row[j];
                row[j] = c * row[j] - s * R[k][j];
                R[k][j] = t;
            }
        }
    }
}

// ---- 2. a track per thread: triangulate, gate, one reason ----------------------------------------------------------
__global__ __launch_bounds__(MV_T) void mv_track_kernel(MVArgs a) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int i = blockIdx.x * MV_T + threadIdx.x; i < a.n; i += gridDim.x * MV_T) {
        const int o0 = a.off[i], o1 = a.off[i + 1];
        const int V = o1 - o0;
        int reason = MV_TOO_FEW_VIEWS;
        double X[3] = {nan, nan, nan};
        double mean = nan, zmin = nan, zmax = nan;
        if (V >= 2) {
            double R[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) R[r][c] = 0.0;
            for (int o = o0; o < o1; ++o) {
                const double* P = a.P + 12 * (size_t)a.view[o];
                const double u = a.uv[2 * (size_t)o], v = a.uv[2 * (size_t)o + 1];
                double ru[4], rv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { ru[k] = u * P[8 + k] - P[k]; rv[k] = v * P[8 + k] - P[4 + k]; }
                mv_fold_row(R, ru);
                mv_fold_row(R, rv);
            }
            double A[4][4], Vm[4][4];                  // [column][row], as dlt_svd.hpp holds them
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) A[c][r] = R[r][c];
            sslam::jacobi_sweeps(A, Vm);
            double best = 0, X4[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double s = A[k][0] * A[k][0] + A[k][1] * A[k][1] + A[k][2] * A[k][2] + A[k][3] * A[k][3];
                if (k == 0 || s < best) {
                    best = s;
#pragma unroll
                    for (int r = 0; r < 4; ++r) X4[r] = Vm[k][r];
                }
            }
            const double w = X4[3];
            reason = MV_INVALID_W;
            if (isfinite(w) && fabs(w) > 1e-12) {
                X[0] = X4[0] / w; X[1] = X4[1] / w; X[2] = X4[2] / w;
                bool in_window = true, in_front = true;
                double sum = 0;
                zmin = INFINITY; zmax = -INFINITY;
                for (int o = o0; o < o1; ++o) {
                    const double* T = a.Tcw + 16 * (size_t)a.view[o];
                    const double u = a.uv[2 * (size_t)o], v = a.uv[2 * (size_t)o + 1];
                    const double xc = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[3];
                    const double yc = T[4] * X[0] + T[5] * X[1] + T[6] * X[2] + T[7];
                    const double z = T[8] * X[0] + T[9] * X[1] + T[10] * X[2] + T[11];
                    in_window &= a.min_d <= z && z <= a.max_d;
                    zmin = fmin(zmin, z); zmax = fmax(zmax, z);
                    double e = INFINITY;
                    if (z > 1e-6) {
                        const double xn = xc / z, yn = yc / z;
                        const double du = a.K[0] * xn + a.K[1] * yn + a.K[2] - u, dv = a.K[3] * xn + a.K[4] * yn + a.K[5] - v;
                        e = sqrt(du * du + dv * dv);
                    } else {
                        in_front = false;
                    }
                    sum += e;
                }
                mean = sum / (double)V;
                if (!in_window) reason = MV_BAD_DEPTH;
                else if (!in_front) reason = MV_BEHIND_CAM;
                else if (mean > a.err_max) reason = MV_HIGH_REPROJ;
                else reason = MV_KEPT;
            }
        }
        a.reason[i] = reason;
        a.Xall[3 * (size_t)i] = X[0]; a.Xall[3 * (size_t)i + 1] = X[1]; a.Xall[3 * (size_t)i + 2] = X[2];
        if (a.diag) {
            double* d = a.diag + 3 * (size_t)i;
            d[0] = mean; d[1] = zmin; d[2] = zmax;
        }
    }
}

// ---- 3. the kept tracks in track order, the counters (one workgroup) -----------------------------------------------
__global__ __launch_bounds__(MV_TAIL_T) void mv_tail_kernel(MVArgs a) {
    __shared__ int wsum[MV_TAIL_T / 64], base;
    __shared__ int sh[MV_TAIL_T];
    __shared__ int totals[8];
    const int n = a.n;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    int cnt[MV_REASONS] = {0, 0, 0, 0, 0, 0};
    for (int i0 = 0; i0 < n; i0 += MV_TAIL_T) {
        const int i = i0 + threadIdx.x;
        const int reason = i < n ? a.reason[i] : -1;
#pragma unroll
        for (int r = 0; r < MV_REASONS; ++r) cnt[r] += reason == r;
        sslam::block_compact<MV_TAIL_T>(reason == MV_KEPT, wsum, base, [&](int o) {
            const size_t s = 3 * (size_t)i, d = 3 * (size_t)o;
            a.X_out[d] = a.Xall[s]; a.X_out[d + 1] = a.Xall[s + 1]; a.X_out[d + 2] = a.Xall[s + 2];
            a.idx_out[o] = i;
        });
    }
#pragma unroll
    for (int r = 0; r < MV_REASONS; ++r) {
        const int tot = sslam::block_sum<MV_TAIL_T>(cnt[r], sh);
        if ((int)threadIdx.x == r + 1) totals[r + 1] = tot;
    }
    if (threadIdx.x == 0) { totals[0] = base; totals[7] = n; }
    __syncthreads();
    if (threadIdx.x < 8) a.info_out[threadIdx.x] = totals[threadIdx.x];      // one lane per word
}

void mv_bind(sslam::Slab& sl, MVArgs& a, size_t N, size_t M, size_t F, bool diag) {
    a.off = sl.take<int32_t>(N + 1); a.view = sl.take<int32_t>(M); a.uv = sl.take<float>(M * 2);
    a.Tcw = sl.take<double>(F * 16); a.P = sl.take<double>(F * 12);
    a.reason = sl.take<int32_t>(N); a.Xall = sl.take<double>(N * 3);
    a.X_out = sl.take<double>(N * 3); a.idx_out = sl.take<int32_t>(N); a.info_out = sl.take<int32_t>(8);
    if (diag) a.diag = sl.take<double>(N * 3);
}

// ---- pairs within a radius -------------------------------------------------------------------------------------------
struct CPArgs {
    int n;
    const double* pos;                        // [n][3]
    double r2;
    unsigned long long cap;
    int32_t* pairs;                           // [cap][2]
    unsigned long long* count;                // every hit, written or not
};

__global__ __launch_bounds__(CP_T) void cp_pairs_kernel(CPArgs a) {
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj < bi) return;
    __shared__ double sx[CP_T], sy[CP_T], sz[CP_T];
    const int j_own = bj * CP_T + (int)threadIdx.x;
    if (j_own < a.n) {
        const double* p = a.pos + 3 * (size_t)j_own;
        sx[threadIdx.x] = p[0]; sy[threadIdx.x] = p[1]; sz[threadIdx.x] = p[2];
    }
    __syncthreads();
    const int i = bi * CP_T + (int)threadIdx.x;
    if (i >= a.n) return;
    const double xi = a.pos[3 * (size_t)i], yi = a.pos[3 * (size_t)i + 1], zi = a.pos[3 * (size_t)i + 2];
    const int jn = min(CP_T, a.n - bj * CP_T);
    for (int jj = bi == bj ? (int)threadIdx.x + 1 : 0; jj < jn; ++jj) {      // i < j inside a diagonal tile
        const double dx = xi - sx[jj], dy = yi - sy[jj], dz = zi - sz[jj];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 <= a.r2) {                      // (false for a NaN: a non-finite coordinate pairs with nothing)
            const unsigned long long o = atomicAdd(a.count, 1ull);
            if (o < a.cap) { a.pairs[2 * o] = i; a.pairs[2 * o + 1] = bj * CP_T + jj; }
        }
    }
}

void cp_bind(sslam::Slab& sl, CPArgs& a, size_t N, size_t cap, bool host) {
    a.count = sl.take<unsigned long long>(1); a.pairs = sl.take<int32_t>(cap * 2);
    if (host) a.pos = sl.take<double>(N * 3);
}

int cp_run(sslam_ctx* ctx, const char* who, int n, const double* pos_host, const double* pos_dev, double radius, int64_t cap,
           int32_t* pairs_out, int64_t* count_out) {
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= 0 && n <= 65535 * CP_T, "%s: n %d outside [0, %d]", who, n, 65535 * CP_T);
    SSLAM_REQUIRE(std::isfinite(radius) && radius >= 0, "%s: radius must be finite and >= 0", who);
    SSLAM_REQUIRE(cap >= 0 && cap <= ((int64_t)1 << 30), "%s: cap outside [0, 2^30]", who);
    SSLAM_REQUIRE(count_out != nullptr && (cap == 0 || pairs_out != nullptr), "%s: NULL argument", who);
    *count_out = 0;
    if (n < 2) return 0;
    SSLAM_REQUIRE(pos_host != nullptr || pos_dev != nullptr, "%s: NULL argument", who);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    CPArgs a{};
    const bool host = pos_host != nullptr;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { cp_bind(sl, a, (size_t)n, (size_t)cap, host); })) return rc;
    hipStream_t s = ctx->stream;
    if (host) SSLAM_HIP_CHECK(sslam::copy_up(s, a.pos, pos_host, (size_t)n * 3));
    else a.pos = pos_dev;
    a.n = n; a.r2 = radius * radius; a.cap = (unsigned long long)cap;
    SSLAM_HIP_CHECK(hipMemsetAsync(a.count, 0, sizeof(unsigned long long), s));
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    const int tiles = sslam::cdiv(n, CP_T);
    hipLaunchKernelGGL(cp_pairs_kernel, dim3(tiles, tiles), dim3(CP_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    unsigned long long count = 0;
    SSLAM_HIP_CHECK(sslam::copy_down(s, &count, a.count, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    *count_out = (int64_t)count;
    const size_t got = (size_t)std::min<unsigned long long>(count, (unsigned long long)cap);
    if (got) {
        SSLAM_HIP_CHECK(sslam::copy_down(s, pairs_out, a.pairs, got * 2));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    return 0;
}

}  // namespace

extern "C" int sslam_triangulate_tracks_host(sslam_ctx* ctx, int n_tracks, int n_views, const int32_t* track_off,
                                             const int32_t* obs_view, const float* obs_uv, const double* K9,
                                             const double* Tcw, double min_depth, double max_depth, double max_rep_err,
                                             double* X_out, int32_t* idx_out, int32_t* info_out, int32_t* reason_out,
                                             double* diag_out) {
    const char* who = "sslam_triangulate_tracks_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n_tracks >= 0 && n_views >= 0, "%s: negative count", who);
    SSLAM_REQUIRE(K9 != nullptr && info_out != nullptr, "%s: NULL argument", who);
    for (int i = 0; i < 8; ++i) info_out[i] = 0;
    if (n_tracks == 0) return 0;
    SSLAM_REQUIRE(track_off && X_out && idx_out, "%s: NULL argument", who);
    SSLAM_REQUIRE(track_off[0] == 0, "%s: track_off[0] is %d, not 0", who, track_off[0]);
    for (int i = 0; i < n_tracks; ++i)
        SSLAM_REQUIRE(track_off[i + 1] >= track_off[i], "%s: track_off decreases at track %d", who, i);
    const size_t N = (size_t)n_tracks, M = (size_t)track_off[n_tracks], F = (size_t)n_views;
    SSLAM_REQUIRE(M == 0 || (obs_view && obs_uv && Tcw), "%s: NULL argument", who);
    for (size_t o = 0; o < M; ++o)
        SSLAM_REQUIRE(obs_view[o] >= 0 && obs_view[o] < n_views, "%s: obs_view[%zu] = %d outside [0, %d)", who, o, obs_view[o], n_views);
    MVArgs a{};
    for (int i = 0; i < 9; ++i) a.K[i] = K9[i];
    a.min_d = min_depth; a.max_d = max_depth; a.err_max = max_rep_err;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const bool want_diag = diag_out != nullptr;
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { mv_bind(sl, a, N, M, F, want_diag); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.off, track_off, N + 1));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.view, obs_view, M));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.uv, obs_uv, M * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.Tcw, Tcw, F * 16));
    a.n = n_tracks; a.F = n_views;
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (F) hipLaunchKernelGGL(mv_proj_kernel, dim3(sslam::cdiv(n_views, MV_T)), dim3(MV_T), 0, s, a);
    hipLaunchKernelGGL(mv_track_kernel, dim3(sslam::cdiv(n_tracks, MV_T)), dim3(MV_T), 0, s, a);
    hipLaunchKernelGGL(mv_tail_kernel, dim3(1), dim3(MV_TAIL_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    SSLAM_HIP_CHECK(sslam::copy_down(s, info_out, a.info_out, 8));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));      // (the count sizes the rest)
    const size_t kept = (size_t)info_out[0];
    if (kept) {
        SSLAM_HIP_CHECK(sslam::copy_down(s, X_out, a.X_out, kept * 3));
        SSLAM_HIP_CHECK(sslam::copy_down(s, idx_out, a.idx_out, kept));
    }
    if (reason_out) SSLAM_HIP_CHECK(sslam::copy_down(s, reason_out, a.reason, N));
    if (want_diag) SSLAM_HIP_CHECK(sslam::copy_down(s, diag_out, a.diag, N * 3));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_close_pairs_host(sslam_ctx* ctx, int n, const double* pos, double radius, int64_t cap,
                                      int32_t* pairs_out, int64_t* count_out) {
    const char* who = "sslam_close_pairs_host";
    SSLAM_REQUIRE(n < 2 || pos != nullptr, "%s: NULL argument", who);
    return cp_run(ctx, who, n, pos, nullptr, radius, cap, pairs_out, count_out);
}

extern "C" int sslam_close_pairs_dev(sslam_ctx* ctx, int n, const double* pos_dev, double radius, int64_t cap,
                                     int32_t* pairs_out, int64_t* count_out) {
    const char* who = "sslam_close_pairs_dev";
    SSLAM_REQUIRE(n < 2 || pos_dev != nullptr, "%s: NULL argument", who);
    return cp_run(ctx, who, n, nullptr, pos_dev, radius, cap, pairs_out, count_out);
}
