// pnp_kernels.hip - PnP-RANSAC (EPnP samples, LM refinement) on the GPU.
//
// Replaces `cv2.solvePnPRansac(pts3d, pts2d, K, None, flags=cv2.SOLVEPNP_ITERATIVE, ...)` as called by
// `solve_pnp_ransac` (slam/core/pnp_utils.py:307-341; caller main_revamped.py:449-475, with Tcw_pred as the guess) and
// `refine_pose_pnp` (pnp_utils.py:200-221).
//
// The algorithm is OpenCV 4.x's classic (non-USAC) path, restated from its published source (solvepnp.cpp, epnp.cpp,
// calibration.cpp, compat_ptsetreg.cpp, ptsetreg.cpp); oracle/pnp_ref.py is the restatement in numpy, with every
// point that could not be confirmed named there:
//   * float32 correspondences; model_points 5, minimal solver EPnP on undistortPoints' float32 normalized points;
//     n == 5: one EPnP on all points, all inliers, no refinement;
//   * samples: cv::RNG (state 2^64-1), getSubset with duplicate re-draws (the PnP callback accepts every subset);
//   * score: projectPoints to float32 pixels, err = float ||ip - proj||^2, inlier iff err <= (float)(px^2), px a float;
//   * best = strictly larger inlier count than max(best, 4); budget RANSACUpdateNumIters after every new best;
//   * final: CvLevMarq (cvFindExtrinsicCameraParams2 with a guess) on the winner's inliers, 20 iterations or a relative
//     step below FLT_EPSILON; its start is the winner's model, or - when the caller passed a guess - the LAST evaluated
//     sample's EPnP pose (the callback writes every sample into solvePnPRansac's own rvec / tvec buffers);
//   * returned mask: the winner's.
// PARITY UNPINNED: cv2 is absent here.  Every eigen / singular vector comes from one cyclic Jacobi eigen-solver
// (jacobi_lds, the same operations in the same order as the restatement's `jacobi_eigen`), the beta least-squares
// from epnp's own qr_solve, the LM's 6 x 6 solve from Gaussian elimination.
//
// Like ransac_kernels.hip, the sequential loop depends on the data only through the running best / budget: one lane
// replays the sample stream chunk by chunk, a workgroup per sample solves EPnP (fp64, LDS) and scores the model against
// every correspondence, one lane replays the best / budget logic.  Eight launches per call, whatever the data: head
// [compaction of the association's output (device entry), control block, samples of chunk 0] - per chunk [solve +
// score] and [replay + samples of the next chunk] - tail [replay, the winner's mask, the LM start] - LM.  cv::RNG,
// RANSACUpdateNumIters, getSubset's draw and the workgroup reduction / compaction come from geom_common.hpp, shared with
// ransac_kernels.hip.
#include "common.hpp"

#include <algorithm>
#include <cfloat>

// bit-for-bit agreement with the restatement: no fused multiply-adds in this file (the shared helpers included)
#pragma clang fp contract(off)
#include "geom_common.hpp"

namespace {

constexpr int PN_MP = 5;                 // model points
constexpr int PN_MAX_ITERS = 100000;
constexpr int PN_T = 64;                 // solve + score: one wave per sample
constexpr int PN_HEAD_T = 1024;
constexpr int PN_LM_T = 256;
constexpr int PN_LM_MAX = 20;
constexpr int PN_JACOBI_SWEEPS = 50;
constexpr int PN_LDS_POINTS = 3072;      // LM: 3072 x 20 bytes = 60 KB of dynamic LDS at most

struct PNCtrl {
    int n;              // correspondences
    int mode;           // 0 RANSAC, 1 n == 5, 2 nothing to do (n < 5)
    int niters;         // iterations the sequential loop has run
    int n_subsets;      // samples drawn
    int budget;         // the loop's iteration budget
    int max_good;       // best inlier count so far
    int best_h;         // winning sample (-1: none)
    int lm_iters;
    unsigned long long rng_state;
};

struct PNArgs {
    int n_max;                                 // capacity (host entry: n; device entry: the map's point count)
    int max_iters, use_guess;
    int h0, h1;                                // sample range of this chunk
    double fx, fy, cx, cy;
    double confidence;
    float thresh2;                             // (float)(px * px), px = (float)reproj_px
    const int32_t* kp_of_point;                // device entry: association output [n_max]
    const double* map_xyz;                     // device entry: map points [n_max][3]
    const float* kp_xy;                        // device entry: keypoints [*][2]
    float* p3;                                 // [n_max][3] correspondences (compacted)
    float* p2;                                 // [n_max][2]
    int* subsets;                              // [max_iters][5]
    double* models;                            // [max_iters][6]  rvec, tvec
    int* counts;                               // [max_iters]
    unsigned char* mask;                       // [n_max]
    double* lm_start;                          // [6]
    double* Tcw_out;                           // [16]
    int32_t* n_out;                            // [1] (may be NULL)
    int32_t* info_out;                         // [4]
    PNCtrl* ctrl;
};

// samples [h0, h1) of the stream (one lane; the draws depend on n only)
__device__ void pn_draw(const PNArgs& a, int h0, int h1) {
    PNCtrl* c = a.ctrl;
    if (c->mode != 0 || h0 != c->niters || h0 >= c->budget) return;
    const int n = c->n, end = min(h1, c->budget);
    sslam::CvRng rng{c->rng_state};
    for (int it = h0; it < end; ++it) {
        int idx[PN_MP];
        sslam::draw_distinct<PN_MP>(rng, n, idx);
#pragma unroll
        for (int i = 0; i < PN_MP; ++i) a.subsets[it * PN_MP + i] = idx[i];
    }
    c->n_subsets = end;
    c->rng_state = rng.state;
}

// best / budget over the scored samples [h0, h1) (one lane)
__device__ void pn_select(const PNArgs& a, int h0, int h1) {
    PNCtrl* c = a.ctrl;
    if (c->mode != 0 || h0 != c->niters) return;
    const int n = c->n;
    int it = h0;
    for (; it < h1 && it < c->n_subsets && it < c->budget; ++it) {
        const int good = a.counts[it];
        if (good > max(c->max_good, PN_MP - 1)) {
            c->max_good = good;
            c->best_h = it;
            c->budget = sslam::update_num_iters(a.confidence, (double)(n - good) / n, PN_MP, c->budget);
        }
    }
    c->niters = it;
}

// ---- linear algebra in LDS (the restatement's operations, in its order) ----------------------------------------------
__device__ __forceinline__ double ieee_div(double a, double b) { return a / b; }

// Cyclic Jacobi on the symmetric n x n matrix A (LDS), all PN_T lanes of the workgroup: lanes r < n rotate row / column r
// of A, lanes n <= l < 2n row l - n of V.  Writes the eigenvectors as ROWS, by descending eigenvalue (ties by index), to
// `vec`, the eigenvalues to `val`.  A is destroyed, V is scratch (n x n).
__device__ void jacobi_lds(double* A, double* V, int n, double* vec, double* val) {
    const int lane = threadIdx.x;
    for (int i = lane; i < n * n; i += PN_T) V[i] = (i / n == i % n) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < PN_JACOBI_SWEEPS; ++sweep) {
        int nz = 0;
        for (int i = lane; i < n * n; i += PN_T) nz |= (i / n != i % n) && A[i] != 0.0;
        if (__syncthreads_or(nz) == 0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;                            // (uniform: every lane read the same value)
                const double app = A[p * n + p], aqq = A[q * n + q];
                const double g = 100.0 * fabs(apq);
                __syncthreads();                                     // every lane has read before anyone writes
                if (sweep >= 4 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
                    if (lane == 0) { A[p * n + q] = 0.0; A[q * n + p] = 0.0; }
                    __syncthreads();
                    continue;
                }
                const double h = aqq - app;
                double t;
                if (fabs(h) + g == fabs(h)) {
                    t = ieee_div(apq, h);
                } else {
                    const double theta = ieee_div(0.5 * h, apq);
                    t = ieee_div(1.0, fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) t = -t;
                }
                const double c = ieee_div(1.0, sqrt(1.0 + t * t));
                const double s = t * c;
                const double tau = ieee_div(s, 1.0 + c);
                if (lane < n) {
                    const int r = lane;
                    if (r != p && r != q) {
                        const double gp = A[r * n + p], hq = A[r * n + q];
                        const double np_ = gp - s * (hq + gp * tau), nq = hq + s * (gp - hq * tau);
                        A[r * n + p] = np_; A[p * n + r] = np_;
                        A[r * n + q] = nq; A[q * n + r] = nq;
                    }
                } else if (lane < 2 * n) {
                    const int r = lane - n;
                    const double gp = V[r * n + p], hq = V[r * n + q];
                    V[r * n + p] = gp - s * (hq + gp * tau);
                    V[r * n + q] = hq + s * (gp - hq * tau);
                }
                if (lane == 0) {
                    A[p * n + p] = app - t * apq;
                    A[q * n + q] = aqq + t * apq;
                    A[p * n + q] = 0.0; A[q * n + p] = 0.0;
                }
                __syncthreads();
            }
    }
    __syncthreads();
    if (lane == 0) {
        unsigned taken = 0;
        for (int k = 0; k < n; ++k) {
            int b = -1;
            for (int i = 0; i < n; ++i)
                if (!(taken >> i & 1u) && (b < 0 || A[i * n + i] > A[b * n + b])) b = i;
            taken |= 1u << b;
            val[k] = A[b * n + b];
            for (int j = 0; j < n; ++j) vec[k * n + j] = V[j * n + b];
        }
    }
    __syncthreads();
}

// U V^T of the SVD of the 3 x 3 `A` (LDS) as A (A^T A)^(-1/2) into R (LDS); all lanes.  w: 9 + 9 + 9 + 3 doubles of scratch
__device__ void polar3_lds(const double* A, double* R, double* w) {
    double* AtA = w; double* Vs = w + 9; double* vec = w + 18; double* val = w + 27;
    if (threadIdx.x == 0)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) AtA[i * 3 + j] = A[0 * 3 + i] * A[0 * 3 + j] + A[1 * 3 + i] * A[1 * 3 + j] + A[2 * 3 + i] * A[2 * 3 + j];
    __syncthreads();
    jacobi_lds(AtA, Vs, 3, vec, val);
    if (threadIdx.x == 0) {
        double S[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) acc += vec[k * 3 + i] * ieee_div(1.0, sqrt(fabs(val[k]))) * vec[k * 3 + j];
                S[i * 3 + j] = acc;
            }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = A[i * 3 + 0] * S[0 * 3 + j] + A[i * 3 + 1] * S[1 * 3 + j] + A[i * 3 + 2] * S[2 * 3 + j];
    }
    __syncthreads();
}

// epnp::qr_solve on LDS arrays (one lane): A [nr x nc] row-major and b are destroyed; false: singular (X untouched)
__device__ bool qr_solve(double* A, double* b, int nr, int nc, double* X, double* A1, double* A2) {
    for (int k = 0; k < nc; ++k) {
        double eta = fabs(A[k * nc + k]);
        for (int i = k + 1; i < nr; ++i) { const double e = fabs(A[i * nc + k]); if (eta < e) eta = e; }
        if (eta == 0) return false;
        const double inv_eta = ieee_div(1.0, eta);
        double sum2 = 0.0;
        for (int i = k; i < nr; ++i) { A[i * nc + k] *= inv_eta; sum2 += A[i * nc + k] * A[i * nc + k]; }
        double sigma = sqrt(sum2);
        if (A[k * nc + k] < 0) sigma = -sigma;
        A[k * nc + k] += sigma;
        A1[k] = sigma * A[k * nc + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s = 0.0;
            for (int i = k; i < nr; ++i) s += A[i * nc + k] * A[i * nc + j];
            const double tau = ieee_div(s, A1[k]);
            for (int i = k; i < nr; ++i) A[i * nc + j] -= tau * A[i * nc + k];
        }
    }
    for (int j = 0; j < nc; ++j) {
        double tau = 0.0;
        for (int i = j; i < nr; ++i) tau += A[i * nc + j] * b[i];
        tau = ieee_div(tau, A1[j]);
        for (int i = j; i < nr; ++i) b[i] -= tau * A[i * nc + j];
    }
    X[nc - 1] = ieee_div(b[nc - 1], A2[nc - 1]);
    for (int i = nc - 2; i >= 0; --i) {
        double s = 0.0;
        for (int j = i + 1; j < nc; ++j) s += A[i * nc + j] * X[j];
        X[i] = ieee_div(b[i] - s, A2[i]);
    }
    return true;
}

// cvRodrigues2, vector -> matrix (and dR/dr, 3 x 9, when J != NULL); one lane, pointers into LDS or registers
__device__ void rodrigues_r2R(const double* r, double* R, double* J) {
    double rx = r[0], ry = r[1], rz = r[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        if (J) for (int k = 0; k < 27; ++k) J[k] = 0.0;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c;
    const double itheta = ieee_div(1.0, theta);
    rx *= itheta; ry *= itheta; rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (c * I[k] + c1 * rrt[k]) + s * r_x[k];
    if (!J) return;
    const double drrt[27] = {rx + rx, ry, rz, ry, 0, 0, rz, 0, 0,
                             0, rx, 0, rx, ry + ry, rz, 0, rz, 0,
                             0, 0, rx, 0, 0, ry, rx, ry, rz + rz};
    const double d_r_x_[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0,
                               0, 0, 1, 0, 0, 0, -1, 0, 0,
                               0, -1, 0, 1, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double ri = i == 0 ? rx : i == 1 ? ry : rz;
        const double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
        const double a3 = (c - s * itheta) * ri, a4 = s * itheta;
#pragma unroll
        for (int k = 0; k < 9; ++k)
            J[i * 9 + k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * r_x[k] + a4 * d_r_x_[k];
    }
}

// ---- EPnP of one sample (workgroup of PN_T lanes; everything in LDS) ---------------------------------------------------
struct EpnpLds {
    double A12[144], V12[144], ut[144], d12[12];
    double A3[9], V3[9], uct[9], dc[3], pw3[30];
    double pws[15], us[10], alphas[20], cws[12], ci[9];
    double L[60], rho[6];
    double qa[30], qb[6], qx[5], q1[5], q2[5];
    double betas[4], ccs[12], pcs[15], abt[9], Rb[9], R[3][9], t[3][3], err[3];
    double model[6];
};

__device__ __forceinline__ double dot3(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// least squares of L[:, cols] x = rho (one lane); zeros where qr_solve finds a zero column
__device__ void ls_cols(EpnpLds& e, const int* cols, int nc, double* x) {
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j < nc; ++j) e.qa[i * nc + j] = e.L[i * 10 + cols[j]];
        e.qb[i] = e.rho[i];
    }
    for (int j = 0; j < nc; ++j) e.qx[j] = 0.0;
    qr_solve(e.qa, e.qb, 6, nc, e.qx, e.q1, e.q2);
    for (int j = 0; j < nc; ++j) x[j] = e.qx[j];
}

__device__ void gauss_newton(EpnpLds& e, double* betas) {
    double x[4] = {0, 0, 0, 0};
    for (int it = 0; it < 5; ++it) {
        const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
        for (int i = 0; i < 6; ++i) {
            const double* l = e.L + i * 10;
            e.qa[i * 4 + 0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
            e.qa[i * 4 + 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
            e.qa[i * 4 + 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
            e.qa[i * 4 + 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
            e.qb[i] = e.rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2
                                  + l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
        }
        if (qr_solve(e.qa, e.qb, 6, 4, e.qx, e.q1, e.q2))
            for (int i = 0; i < 4; ++i) x[i] = e.qx[i];
        for (int i = 0; i < 4; ++i) betas[i] = betas[i] + x[i];
    }
}

// the sample's pose as (rvec, tvec) in e.model; NaN when EPnP breaks down.  pw32 / ip32: the sample's points
__device__ void epnp_model(EpnpLds& e, const float* p3, const float* p2, const int* idx, int m, const PNArgs& a) {
    const int lane = threadIdx.x;
    const double fu = a.fx, fv = a.fy, uc = a.cx, vc = a.cy;
    if (lane == 0) {
        for (int i = 0; i < m; ++i) {
            const int id = idx[i];
            for (int j = 0; j < 3; ++j) e.pws[i * 3 + j] = (double)p3[id * 3 + j];
            const float xn = (float)(((double)p2[id * 2] - uc) * ieee_div(1.0, fu));
            const float yn = (float)(((double)p2[id * 2 + 1] - vc) * ieee_div(1.0, fv));
            e.us[i * 2] = (double)xn * fu + uc;
            e.us[i * 2 + 1] = (double)yn * fv + vc;
        }
        // choose_control_points: centroid, then PCA
        for (int j = 0; j < 3; ++j) e.cws[j] = 0.0;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < 3; ++j) e.cws[j] += e.pws[i * 3 + j];
        for (int j = 0; j < 3; ++j) e.cws[j] = ieee_div(e.cws[j], (double)m);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < 3; ++j) e.pw3[i * 3 + j] = e.pws[i * 3 + j] - e.cws[j];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double acc = 0.0;
                for (int i = 0; i < m; ++i) acc += e.pw3[i * 3 + r] * e.pw3[i * 3 + c];
                e.A3[r * 3 + c] = acc;
            }
    }
    __syncthreads();
    jacobi_lds(e.A3, e.V3, 3, e.uct, e.dc);
    if (lane == 0) {
        double ks[3];
        for (int i = 0; i < 3; ++i) ks[i] = sqrt(ieee_div(fabs(e.dc[i]), (double)m));
        for (int i = 1; i < 4; ++i)
            for (int j = 0; j < 3; ++j) e.cws[i * 3 + j] = e.cws[j] + ks[i - 1] * e.uct[(i - 1) * 3 + j];
        // compute_barycentric_coordinates: the pseudo-inverse of [k_j u_j] has rows u_j / k_j
        const double thr = 2 * DBL_EPSILON * (ks[0] + ks[1] + ks[2]);
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 3; ++c) e.ci[j * 3 + c] = ks[j] > thr ? ieee_div(e.uct[j * 3 + c], ks[j]) : 0.0;
        for (int i = 0; i < m; ++i) {
            const double d0 = e.pws[i * 3] - e.cws[0], d1 = e.pws[i * 3 + 1] - e.cws[1], d2 = e.pws[i * 3 + 2] - e.cws[2];
            double* al = e.alphas + 4 * i;
            for (int j = 0; j < 3; ++j) al[1 + j] = e.ci[j * 3] * d0 + e.ci[j * 3 + 1] * d1 + e.ci[j * 3 + 2] * d2;
            al[0] = 1.0 - al[1] - al[2] - al[3];
        }
    }
    __syncthreads();
    // MtM (12 x 12) from the 2m x 12 M of fill_M, built on the fly; lanes share the 144 entries
    for (int ab = lane; ab < 144; ab += PN_T) {
        const int ca = ab / 12, cb = ab % 12;
        double acc = 0.0;
        for (int r = 0; r < 2 * m; ++r) {
            const int i = r >> 1, odd = r & 1;
            double ma, mb;
            {
                const int j = ca / 3, k = ca % 3;
                const double al = e.alphas[4 * i + j];
                ma = odd ? (k == 0 ? 0.0 : k == 1 ? al * fv : al * (vc - e.us[2 * i + 1]))
                         : (k == 0 ? al * fu : k == 1 ? 0.0 : al * (uc - e.us[2 * i]));
            }
            {
                const int j = cb / 3, k = cb % 3;
                const double al = e.alphas[4 * i + j];
                mb = odd ? (k == 0 ? 0.0 : k == 1 ? al * fv : al * (vc - e.us[2 * i + 1]))
                         : (k == 0 ? al * fu : k == 1 ? 0.0 : al * (uc - e.us[2 * i]));
            }
            acc += ma * mb;
        }
        e.A12[ab] = acc;
    }
    __syncthreads();
    jacobi_lds(e.A12, e.V12, 12, e.ut, e.d12);
    if (lane == 0) {
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
        for (int i = 0; i < 6; ++i) {
            double dv[4][3];
            for (int vi = 0; vi < 4; ++vi) {
                const double* v = e.ut + 12 * (11 - vi);
                for (int k = 0; k < 3; ++k) dv[vi][k] = v[3 * pa[i] + k] - v[3 * pb[i] + k];
            }
            double* row = e.L + 10 * i;
            row[0] = dot3(dv[0], dv[0]);
            row[1] = 2.0 * dot3(dv[0], dv[1]);
            row[2] = dot3(dv[1], dv[1]);
            row[3] = 2.0 * dot3(dv[0], dv[2]);
            row[4] = 2.0 * dot3(dv[1], dv[2]);
            row[5] = dot3(dv[2], dv[2]);
            row[6] = 2.0 * dot3(dv[0], dv[3]);
            row[7] = 2.0 * dot3(dv[1], dv[3]);
            row[8] = 2.0 * dot3(dv[2], dv[3]);
            row[9] = dot3(dv[3], dv[3]);
            double d[3];
            for (int k = 0; k < 3; ++k) d[k] = e.cws[pa[i] * 3 + k] - e.cws[pb[i] * 3 + k];
            e.rho[i] = dot3(d, d);
        }
    }
    __syncthreads();
    for (int approx = 0; approx < 3; ++approx) {
        if (lane == 0) {
            double* B = e.betas;
            if (approx == 0) {
                const int cols[4] = {0, 1, 3, 6};
                double b4[4];
                ls_cols(e, cols, 4, b4);
                if (b4[0] < 0) {
                    B[0] = sqrt(-b4[0]);
                    B[1] = ieee_div(-b4[1], B[0]); B[2] = ieee_div(-b4[2], B[0]); B[3] = ieee_div(-b4[3], B[0]);
                } else {
                    B[0] = sqrt(b4[0]);
                    B[1] = ieee_div(b4[1], B[0]); B[2] = ieee_div(b4[2], B[0]); B[3] = ieee_div(b4[3], B[0]);
                }
            } else if (approx == 1) {
                const int cols[3] = {0, 1, 2};
                double b3[3];
                ls_cols(e, cols, 3, b3);
                if (b3[0] < 0) { B[0] = sqrt(-b3[0]); B[1] = b3[2] < 0 ? sqrt(-b3[2]) : 0.0; }
                else { B[0] = sqrt(b3[0]); B[1] = b3[2] > 0 ? sqrt(b3[2]) : 0.0; }
                if (b3[1] < 0) B[0] = -B[0];
                B[2] = 0.0; B[3] = 0.0;
            } else {
                const int cols[5] = {0, 1, 2, 3, 4};
                double b5[5];
                ls_cols(e, cols, 5, b5);
                if (b5[0] < 0) { B[0] = sqrt(-b5[0]); B[1] = b5[2] < 0 ? sqrt(-b5[2]) : 0.0; }
                else { B[0] = sqrt(b5[0]); B[1] = b5[2] > 0 ? sqrt(b5[2]) : 0.0; }
                if (b5[1] < 0) B[0] = -B[0];
                B[2] = ieee_div(b5[3], B[0]); B[3] = 0.0;
            }
            gauss_newton(e, B);
            // compute_ccs, compute_pcs, solve_for_sign
            for (int k = 0; k < 12; ++k) e.ccs[k] = 0.0;
            for (int i = 0; i < 4; ++i) {
                const double* v = e.ut + 12 * (11 - i);
                for (int j = 0; j < 4; ++j)
                    for (int k = 0; k < 3; ++k) e.ccs[j * 3 + k] += B[i] * v[3 * j + k];
            }
            for (int i = 0; i < m; ++i) {
                const double* al = e.alphas + 4 * i;
                for (int j = 0; j < 3; ++j)
                    e.pcs[i * 3 + j] = al[0] * e.ccs[j] + al[1] * e.ccs[3 + j] + al[2] * e.ccs[6 + j] + al[3] * e.ccs[9 + j];
            }
            if (e.pcs[2] < 0.0) {
                for (int k = 0; k < 12; ++k) e.ccs[k] = -e.ccs[k];
                for (int k = 0; k < 3 * m; ++k) e.pcs[k] = -e.pcs[k];
            }
            // estimate_R_and_t, part 1: centroids and ABt
            double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < 3; ++j) { pc0[j] += e.pcs[i * 3 + j]; pw0[j] += e.pws[i * 3 + j]; }
            for (int j = 0; j < 3; ++j) { pc0[j] = ieee_div(pc0[j], (double)m); pw0[j] = ieee_div(pw0[j], (double)m); }
            for (int k = 0; k < 9; ++k) e.abt[k] = 0.0;
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < 3; ++j)
                    for (int k = 0; k < 3; ++k) e.abt[j * 3 + k] += (e.pcs[i * 3 + j] - pc0[j]) * (e.pws[i * 3 + k] - pw0[k]);
            for (int j = 0; j < 3; ++j) { e.t[approx][j] = pc0[j]; e.q1[j] = pw0[j]; }     // (stashed for part 2)
        }
        __syncthreads();
        polar3_lds(e.abt, e.Rb, e.A12);                                                    // (A12 is free again)
        if (lane == 0) {
            double* R = e.R[approx];
            for (int k = 0; k < 9; ++k) R[k] = e.Rb[k];
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7]
                             - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            const double pw0[3] = {e.q1[0], e.q1[1], e.q1[2]};
            double* t = e.t[approx];
            for (int j = 0; j < 3; ++j) t[j] = t[j] - dot3(R + 3 * j, pw0);
            double sum2 = 0.0;
            for (int i = 0; i < m; ++i) {
                const double* pw = e.pws + 3 * i;
                const double Xc = dot3(R, pw) + t[0];
                const double Yc = dot3(R + 3, pw) + t[1];
                const double inv_Zc = ieee_div(1.0, dot3(R + 6, pw) + t[2]);
                const double ue = uc + fu * Xc * inv_Zc;
                const double ve = vc + fv * Yc * inv_Zc;
                const double u = e.us[2 * i], v = e.us[2 * i + 1];
                sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
            }
            e.err[approx] = ieee_div(sum2, (double)m);
        }
        __syncthreads();
    }
    // the best of the three, then Rodrigues (R -> r) of its polar factor
    int N = 0;
    if (e.err[1] < e.err[0]) N = 1;
    if (e.err[2] < e.err[N]) N = 2;
    polar3_lds(e.R[N], e.Rb, e.A12);
    if (lane == 0) {
        const double* t = e.t[N];
        bool finite = true;
        for (int k = 0; k < 9; ++k) finite &= isfinite(e.R[N][k]);
        for (int k = 0; k < 3; ++k) finite &= isfinite(t[k]);
        if (!finite) {
            for (int k = 0; k < 6; ++k) e.model[k] = __longlong_as_double(0x7ff8000000000000LL);
        } else {
            const double* R = e.Rb;
            double r[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
            const double s = sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25);
            double c = (R[0] + R[4] + R[8] - 1) * 0.5;
            c = c > 1. ? 1. : c < -1. ? -1. : c;
            double theta = acos(c);
            if (s < 1e-5) {
                if (c > 0) {
                    r[0] = r[1] = r[2] = 0.0;
                } else {
                    double tt = (R[0] + 1) * 0.5;
                    r[0] = sqrt(fmax(tt, 0.));
                    tt = (R[4] + 1) * 0.5;
                    r[1] = sqrt(fmax(tt, 0.)) * (R[1] < 0 ? -1. : 1.);
                    tt = (R[8] + 1) * 0.5;
                    r[2] = sqrt(fmax(tt, 0.)) * (R[2] < 0 ? -1. : 1.);
                    if (fabs(r[0]) < fabs(r[1]) && fabs(r[0]) < fabs(r[2]) && (R[5] > 0) != (r[1] * r[2] > 0)) r[2] = -r[2];
                    theta = ieee_div(theta, sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
                    for (int k = 0; k < 3; ++k) r[k] *= theta;
                }
            } else {
                double vth = ieee_div(1.0, 2.0 * s);
                vth *= theta;
                for (int k = 0; k < 3; ++k) r[k] *= vth;
            }
            for (int k = 0; k < 3; ++k) { e.model[k] = r[k]; e.model[3 + k] = t[k]; }
        }
    }
    __syncthreads();
}

// PnPRansacCallback::computeError of one correspondence against the pose (R row-major, t): float ||ip - proj||^2
__device__ __forceinline__ float pn_error(const double* R, const double* t, const PNArgs& a, float X, float Y, float Z,
                                          float u, float v) {
    const double Xd = X, Yd = Y, Zd = Z;
    const double x = R[0] * Xd + R[1] * Yd + R[2] * Zd + t[0];
    const double y = R[3] * Xd + R[4] * Yd + R[5] * Zd + t[1];
    const double z = R[6] * Xd + R[7] * Yd + R[8] * Zd + t[2];
    const double iz = z != 0 ? ieee_div(1.0, z) : 1.0;
    const float pu = (float)(x * iz * a.fx + a.cx);
    const float pv = (float)(y * iz * a.fy + a.cy);
    const float dx = __fsub_rn(u, pu), dy = __fsub_rn(v, pv);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}

// ---- solve sample h, score its model against every correspondence (workgroup / sample) ---------------------------------
__global__ __launch_bounds__(PN_T) void pn_models_score_kernel(PNArgs a) {
    __shared__ EpnpLds e;
    __shared__ double Rs[9];
    __shared__ int sh[PN_T];
    __shared__ int idx[PN_MP];
    const int h = a.h0 + blockIdx.x;
    const PNCtrl* c = a.ctrl;
    if (c->mode == 2 || h >= a.h1 || h >= c->n_subsets || a.h0 != c->niters) return;
    const int n = c->n;
    if (threadIdx.x < PN_MP) idx[threadIdx.x] = a.subsets[h * PN_MP + threadIdx.x];
    __syncthreads();
    epnp_model(e, a.p3, a.p2, idx, PN_MP, a);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) a.models[(size_t)h * 6 + k] = e.model[k];
        rodrigues_r2R(e.model, Rs, nullptr);
    }
    __syncthreads();
    if (c->mode == 1) return;                                      // n == 5: every point is an inlier, no scoring
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = Rs[k];
    for (int k = 0; k < 3; ++k) t[k] = e.model[3 + k];
    int good = 0;
    for (int i = threadIdx.x; i < n; i += PN_T)
        good += pn_error(R, t, a, a.p3[3 * i], a.p3[3 * i + 1], a.p3[3 * i + 2], a.p2[2 * i], a.p2[2 * i + 1]) <= a.thresh2;
    good = sslam::block_sum(good, sh);
    if (threadIdx.x == 0) a.counts[h] = good;
}

// ---- head: (device entry) the correspondences in map order, the control block, the samples of chunk 0 ----------------
__global__ __launch_bounds__(PN_HEAD_T) void pn_head_kernel(PNArgs a) {
    __shared__ int wsum[PN_HEAD_T / 64], base;
    PNCtrl* c = a.ctrl;
    int n = a.n_max;
    if (a.kp_of_point) {
        // order-preserving compaction of the association (the order of Matches2D3D), cast to float32 as the reference does
        if (threadIdx.x == 0) base = 0;
        __syncthreads();
        for (int q0 = 0; q0 < a.n_max; q0 += PN_HEAD_T) {
            const int q = q0 + threadIdx.x;
            const int kp = q < a.n_max ? a.kp_of_point[q] : -1;
            sslam::block_compact<PN_HEAD_T>(kp >= 0, wsum, base, [&](int o) {
                a.p3[3 * o] = (float)a.map_xyz[3 * (size_t)q];
                a.p3[3 * o + 1] = (float)a.map_xyz[3 * (size_t)q + 1];
                a.p3[3 * o + 2] = (float)a.map_xyz[3 * (size_t)q + 2];
                a.p2[2 * o] = a.kp_xy[2 * (size_t)kp];
                a.p2[2 * o + 1] = a.kp_xy[2 * (size_t)kp + 1];
            });
        }
        n = base;
    }
    if (threadIdx.x == 0) {
        c->n = n;
        c->mode = n > PN_MP ? 0 : n == PN_MP ? 1 : 2;
        c->niters = 0;
        c->n_subsets = 0;
        c->budget = max(a.max_iters, 1);
        c->max_good = 0;
        c->best_h = -1;
        c->lm_iters = 0;
        c->rng_state = 0xffffffffffffffffULL;
        if (a.n_out) a.n_out[0] = n;
        if (c->mode == 1) {                        // one EPnP on all five points, in order
            for (int i = 0; i < PN_MP; ++i) a.subsets[i] = i;
            c->n_subsets = 1;
        } else {
            pn_draw(a, a.h0, a.h1);
        }
    }
}

// ---- between chunks: the best / budget replay over the chunk just scored, then the samples of the next ---------------
__global__ void pn_step_kernel(PNArgs a, int h2) {
    pn_select(a, a.h0, a.h1);
    pn_draw(a, a.h1, h2);
}

// ---- tail: replay of the last chunk, the winner's mask (findInliers of its model), the LM's start ---------------------
__global__ __launch_bounds__(1024) void pn_tail_kernel(PNArgs a) {
    __shared__ double Rs[9], ts[3];
    __shared__ int have;
    PNCtrl* c = a.ctrl;
    if (threadIdx.x == 0) {
        pn_select(a, a.h0, a.h1);
        if (c->mode == 1) { c->best_h = 0; c->max_good = PN_MP; }
        have = c->mode != 2 && c->best_h >= 0;
        if (have) {
            const double* m = a.models + (size_t)c->best_h * 6;
            rodrigues_r2R(m, Rs, nullptr);
            for (int k = 0; k < 3; ++k) ts[k] = m[3 + k];
            // the LM starts at the winner, or (caller guess) at the last sample the loop evaluated
            const double* s = (a.use_guess && c->mode == 0) ? a.models + (size_t)(c->niters - 1) * 6 : m;
            for (int k = 0; k < 6; ++k) a.lm_start[k] = s[k];
        }
    }
    __syncthreads();
    const int n = c->n;
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = Rs[k];
    for (int k = 0; k < 3; ++k) t[k] = ts[k];
    for (int i = threadIdx.x; i < n; i += 1024) {
        int in = 0;
        if (have) in = c->mode == 1 ? 1 : pn_error(R, t, a, a.p3[3 * i], a.p3[3 * i + 1], a.p3[3 * i + 2], a.p2[2 * i], a.p2[2 * i + 1]) <= a.thresh2;
        a.mask[i] = (unsigned char)in;
    }
}

// ---- LM (CvLevMarq as cvFindExtrinsicCameraParams2 drives it), one workgroup -------------------------------------------
constexpr int PN_NACC = 28;              // JtJ upper triangle (21) + JtErr (6) + ||err||^2

struct LmLds {
    double acc[PN_NACC][PN_LM_T / 64];   // per-wave partial sums
    double R[9], dRdr[27];
    double param[6], prev[6], JtJ[36], JtErr[6], A[36], b[6], x[6];
    double err_norm, prev_err_norm;
    int k, iters, done, retry;
};

// sums over the inliers of the residual (proj - m) and, with jac, of JtJ / JtErr at s.param; fixed order (thread-strided
// partial sums, a fixed shuffle tree per wave, the waves in order)
__device__ void lm_eval(LmLds& s, const PNArgs& a, int n, const float* P3, const float* P2, const unsigned char* mask,
                        bool jac) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) rodrigues_r2R(s.param, s.R, jac ? s.dRdr : nullptr);
    __syncthreads();
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = s.R[k];
    for (int k = 0; k < 3; ++k) t[k] = s.param[3 + k];
    double acc[PN_NACC];
#pragma unroll
    for (int k = 0; k < PN_NACC; ++k) acc[k] = 0.0;
    const double fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
    for (int i = tid; i < n; i += PN_LM_T) {
        if (!mask[i]) continue;
        const double X = P3[3 * i], Y = P3[3 * i + 1], Z = P3[3 * i + 2];
        const double x0 = R[0] * X + R[1] * Y + R[2] * Z + t[0];
        const double y0 = R[3] * X + R[4] * Y + R[5] * Z + t[1];
        const double z0 = R[6] * X + R[7] * Y + R[8] * Z + t[2];
        const double z = z0 != 0 ? ieee_div(1.0, z0) : 1.0;
        const double x = x0 * z, y = y0 * z;
        const double ex = x * fx + cx - (double)P2[2 * i], ey = y * fy + cy - (double)P2[2 * i + 1];
        acc[27] += ex * ex + ey * ey;
        if (jac) {
            double jx[6], jy[6];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double* d = s.dRdr + j * 9;
                const double dx0 = X * d[0] + Y * d[1] + Z * d[2];
                const double dy0 = X * d[3] + Y * d[4] + Z * d[5];
                const double dz0 = X * d[6] + Y * d[7] + Z * d[8];
                jx[j] = fx * (z * (dx0 - x * dz0));
                jy[j] = fy * (z * (dy0 - y * dz0));
            }
            jx[3] = fx * z; jy[3] = 0.0;
            jx[4] = 0.0;    jy[4] = fy * z;
            jx[5] = fx * (-x * z); jy[5] = fy * (-y * z);
            int o = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c2 = r; c2 < 6; ++c2) acc[o++] += jx[r] * jx[c2] + jy[r] * jy[c2];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[21 + r] += jx[r] * ex + jy[r] * ey;
        }
    }
#pragma unroll
    for (int k = 0; k < PN_NACC; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) s.acc[k][w] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double tot[PN_NACC];
#pragma unroll
        for (int k = 0; k < PN_NACC; ++k) {
            double v = 0.0;
            for (int j = 0; j < PN_LM_T / 64; ++j) v += s.acc[k][j];
            tot[k] = v;
        }
        s.err_norm = sqrt(tot[27]);
        if (jac) {
            int o = 0;
            for (int r = 0; r < 6; ++r)
                for (int c2 = r; c2 < 6; ++c2) { s.JtJ[r * 6 + c2] = tot[o]; s.JtJ[c2 * 6 + r] = tot[o]; ++o; }
            for (int r = 0; r < 6; ++r) s.JtErr[r] = tot[21 + r];
        }
    }
    __syncthreads();
}

// CvLevMarq::step: param = prev - solve(JtJ with its diagonal x (1 + 10^k), JtErr) (one lane)
__device__ void lm_step(LmLds& s) {
    const double lambda = exp(s.k * log(10.));
    for (int i = 0; i < 36; ++i) s.A[i] = s.JtJ[i];
    for (int i = 0; i < 6; ++i) { s.A[i * 7] *= 1. + lambda; s.b[i] = s.JtErr[i]; }
    for (int k = 0; k < 6; ++k) {
        int p = k;
        for (int i = k + 1; i < 6; ++i) if (fabs(s.A[i * 6 + k]) > fabs(s.A[p * 6 + k])) p = i;
        if (p != k) {
            for (int j = 0; j < 6; ++j) { const double tmp = s.A[k * 6 + j]; s.A[k * 6 + j] = s.A[p * 6 + j]; s.A[p * 6 + j] = tmp; }
            const double tmp = s.b[k]; s.b[k] = s.b[p]; s.b[p] = tmp;
        }
        for (int i = k + 1; i < 6; ++i) {
            const double f = ieee_div(s.A[i * 6 + k], s.A[k * 6 + k]);
            for (int j = k; j < 6; ++j) s.A[i * 6 + j] -= f * s.A[k * 6 + j];
            s.b[i] -= f * s.b[k];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double v = s.b[i];
        for (int j = i + 1; j < 6; ++j) v -= s.A[i * 6 + j] * s.x[j];
        s.x[i] = ieee_div(v, s.A[i * 7]);
    }
    for (int i = 0; i < 6; ++i) s.param[i] = s.prev[i] - s.x[i];
}

__global__ __launch_bounds__(PN_LM_T) void pn_lm_kernel(PNArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lm_pts[];
    __shared__ LmLds s;
    PNCtrl* c = a.ctrl;
    const int n = c->n;
    const bool have = c->mode != 2 && c->best_h >= 0;
    const int tid = threadIdx.x;
    if (have && c->mode == 0) {
        // inliers' points into LDS when they fit (all n, so the mask indexes them as it is)
        const bool in_lds = n <= PN_LDS_POINTS;
        const float* P3 = a.p3;
        const float* P2 = a.p2;
        if (in_lds) {
            for (int i = tid; i < 3 * n; i += PN_LM_T) lm_pts[i] = a.p3[i];
            for (int i = tid; i < 2 * n; i += PN_LM_T) lm_pts[3 * n + i] = a.p2[i];
            P3 = lm_pts; P2 = lm_pts + 3 * n;
        }
        if (tid == 0) {
            for (int k = 0; k < 6; ++k) s.param[k] = a.lm_start[k];
            s.k = -3; s.iters = 0; s.done = 0;
        }
        __syncthreads();
        lm_eval(s, a, n, P3, P2, a.mask, true);
        if (tid == 0) s.prev_err_norm = s.err_norm;
        for (;;) {
            if (tid == 0) {
                for (int i = 0; i < 6; ++i) s.prev[i] = s.param[i];
                lm_step(s);
            }
            __syncthreads();
            for (;;) {
                lm_eval(s, a, n, P3, P2, a.mask, false);
                if (tid == 0) {
                    s.retry = 0;
                    if (s.err_norm > s.prev_err_norm && ++s.k <= 16) { lm_step(s); s.retry = 1; }
                }
                __syncthreads();
                if (!s.retry) break;
            }
            if (tid == 0) {
                s.k = max(s.k - 1, -16);
                ++s.iters;
                double dn = 0.0, pn = 0.0;
                for (int i = 0; i < 6; ++i) { const double d = s.param[i] - s.prev[i]; dn += d * d; pn += s.prev[i] * s.prev[i]; }
                s.done = s.iters >= PN_LM_MAX || ieee_div(sqrt(dn), sqrt(pn) + DBL_EPSILON) < FLT_EPSILON;
                if (!s.done) s.prev_err_norm = s.err_norm;
            }
            __syncthreads();
            if (s.done) break;
            lm_eval(s, a, n, P3, P2, a.mask, true);
        }
    } else if (tid == 0 && have) {
        for (int k = 0; k < 6; ++k) s.param[k] = a.models[k];       // n == 5: the EPnP pose as it is
        s.iters = 0;
    }
    __syncthreads();
    if (tid == 0) {
        double R[9];
        if (have) rodrigues_r2R(s.param, R, nullptr);
        for (int i = 0; i < 16; ++i) a.Tcw_out[i] = (i % 5 == 0) ? 1.0 : 0.0;
        if (have) {
            for (int r = 0; r < 3; ++r) {
                for (int k = 0; k < 3; ++k) a.Tcw_out[r * 4 + k] = R[r * 3 + k];
                a.Tcw_out[r * 4 + 3] = s.param[3 + r];
            }
        }
        c->lm_iters = have ? s.iters : 0;
        a.info_out[0] = have ? c->max_good : -1;
        a.info_out[1] = c->mode == 0 ? c->niters : 0;
        a.info_out[2] = c->mode == 0 ? c->best_h : -1;
        a.info_out[3] = c->lm_iters;
    }
}

// the whole call (shared by the two entries): 8 launches - head, per chunk [solve + score] and [replay + next samples],
// tail, LM.  A chunk whose first sample lies beyond the (shrinking) budget is an early-exit launch; the result does not
// depend on the chunking.
void pn_enqueue(hipStream_t s, PNArgs a) {
    const auto bounds = sslam::ransac_chunk_bounds(a.max_iters, 64);     // (the schedule: geom_slab.hpp)
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    {
        PNArgs h = a; h.h0 = bounds[0]; h.h1 = bounds[1];
        hipLaunchKernelGGL(pn_head_kernel, dim3(1), dim3(PN_HEAD_T), 0, s, h);
    }
    for (int ci = 0; ci < 3; ++ci) {
        a.h0 = bounds[ci]; a.h1 = bounds[ci + 1];
        // (chunk 0 always launches: the n == 5 branch solves its one sample there)
        hipLaunchKernelGGL(pn_models_score_kernel, dim3(std::max(a.h1 - a.h0, 1)), dim3(PN_T), 0, s, a);
        if (ci < 2) hipLaunchKernelGGL(pn_step_kernel, dim3(1), dim3(1), 0, s, a, bounds[ci + 2]);
    }
    hipLaunchKernelGGL(pn_tail_kernel, dim3(1), dim3(1024), 0, s, a);          // (a.h0, a.h1: the last chunk)
    const size_t lds = (size_t)std::min(a.n_max, PN_LDS_POINTS) * 20;
    hipLaunchKernelGGL(pn_lm_kernel, dim3(1), dim3(PN_LM_T), lds, s, a);
}

// the slab-backed pointers of PNArgs, in slab order
void pn_bind(sslam::Slab& sl, PNArgs& a, size_t N, size_t H) {
    a.p3 = sl.take<float>(N * 3); a.p2 = sl.take<float>(N * 2); a.subsets = sl.take<int>(H * PN_MP);
    a.models = sl.take<double>(H * 6); a.counts = sl.take<int>(H); a.mask = sl.take<unsigned char>(N);
    a.lm_start = sl.take<double>(6); a.Tcw_out = sl.take<double>(16); a.info_out = sl.take<int32_t>(4);
    a.n_out = sl.take<int32_t>(1); a.ctrl = sl.take<PNCtrl>(1);
}

int pn_args(sslam_ctx* ctx, int n_max, const double* K9, int use_guess, double reproj_px, double confidence,
            int max_iters, PNArgs& a) {
    SSLAM_REQUIRE(K9 != nullptr, "PnP: K9 is NULL");
    SSLAM_REQUIRE(max_iters >= 0 && max_iters <= PN_MAX_ITERS, "PnP: max_iters %d outside [0, %d]", max_iters, PN_MAX_ITERS);
    SSLAM_REQUIRE(confidence > 0 && confidence < 1, "PnP: confidence %g outside (0, 1)", confidence);
    max_iters = std::max(max_iters, 1);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    a = PNArgs{};
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { pn_bind(sl, a, (size_t)std::max(n_max, 1), (size_t)max_iters); }))
        return rc;
    a.n_max = n_max; a.max_iters = max_iters; a.use_guess = use_guess;
    a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5];
    a.confidence = confidence;
    const double px = (double)(float)reproj_px;            // solvePnPRansac's `float reprojectionError`
    a.thresh2 = (float)(px * px);
    return 0;
}

}  // namespace

extern "C" int sslam_pnp_ransac_dev(sslam_ctx* ctx, int n_points, const int32_t* kp_of_point_dev, const double* pts3d_dev,
                                    const float* kp_xy_dev, const double* K9, const double* Tcw_init16, double reproj_px,
                                    double confidence, int max_iters, unsigned char* mask_out_dev, double* Tcw_out_dev,
                                    int32_t* n_out_dev, int32_t* info_out_dev) {
    SSLAM_REQUIRE(ctx != nullptr, "sslam_pnp_ransac_dev: ctx is NULL");
    SSLAM_REQUIRE(n_points >= 1, "sslam_pnp_ransac_dev: n_points %d < 1", n_points);
    SSLAM_REQUIRE(kp_of_point_dev && pts3d_dev && kp_xy_dev && Tcw_out_dev && info_out_dev,
                  "sslam_pnp_ransac_dev: NULL argument");
    PNArgs a;
    if (int rc = pn_args(ctx, n_points, K9, Tcw_init16 != nullptr, reproj_px, confidence, max_iters, a)) return rc;
    a.kp_of_point = kp_of_point_dev; a.map_xyz = pts3d_dev; a.kp_xy = kp_xy_dev;
    if (mask_out_dev) a.mask = mask_out_dev;
    a.Tcw_out = Tcw_out_dev; a.info_out = info_out_dev;
    if (n_out_dev) a.n_out = n_out_dev;
    pn_enqueue(ctx->stream, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int sslam_pnp_ransac_host(sslam_ctx* ctx, int n, const float* pts3d, const float* pts2d, const double* K9,
                                     const double* Tcw_init16, double reproj_px, double confidence, int max_iters,
                                     unsigned char* mask_out, double* Tcw_out, int* info_out) {
    SSLAM_REQUIRE(ctx != nullptr, "sslam_pnp_ransac_host: ctx is NULL");
    SSLAM_REQUIRE(n >= 5, "sslam_pnp_ransac_host: %d correspondences, need >= 5 (4: OpenCV's P3P branch, not covered)", n);
    SSLAM_REQUIRE(pts3d && pts2d && mask_out && Tcw_out, "sslam_pnp_ransac_host: NULL argument");
    PNArgs a;
    if (int rc = pn_args(ctx, n, K9, Tcw_init16 != nullptr, reproj_px, confidence, max_iters, a)) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p3, pts3d, (size_t)n * 3));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p2, pts2d, (size_t)n * 2));
    pn_enqueue(s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    int info[4];
    SSLAM_HIP_CHECK(sslam::copy_down(s, info, a.info_out, 4));
    SSLAM_HIP_CHECK(sslam::copy_down(s, Tcw_out, a.Tcw_out, 16));
    SSLAM_HIP_CHECK(sslam::copy_down(s, mask_out, a.mask, (size_t)n));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (info_out) for (int i = 0; i < 4; ++i) info_out[i] = info[i];
    return 0;
}
