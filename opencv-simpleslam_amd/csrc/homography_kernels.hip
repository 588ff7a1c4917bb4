// homography_kernels.hip - homography RANSAC on the GPU: the H leg of the reference's two-view gate.
//
// Replaces `cv2.findHomography(pts_ref, pts_cur, cv2.RANSAC, px)` as `evaluate_two_view_bootstrap` calls it
// (slam/core/two_view_bootstrap.py:230, :294) and the tracking fallbacks do (slam/monocular/main.py:409, main4.py:458).
//
// The algorithm is OpenCV 4.x's classic (non-USAC) path, restated (fundam.cpp, ptsetreg.cpp, the LM solver):
//   * 4 matches: one normalised DLT on them, mask all ones, no refinement;
//   * more: RANSAC with cv::RNG (state 2^64-1); getSubset draws 4 distinct indices and throws a draw away when its last point
//     is collinear with an earlier pair in either point set, or when the orientation test fails (the signs of
//     det[[x,y,1]...] of the four triples, source times destination: 0 or 4 negatives pass), up to 10000 attempts;
//     runKernel = the normalised DLT (centroids, mean absolute deviations, LtL accumulated on its upper triangle, the
//     eigenvector of its smallest eigenvalue, denormalised, divided by H[8]); error in float on H cast to float, inlier iff
//     err <= (float)(thresh^2); best = count strictly above max(best so far, 3); the budget re-estimated after every
//     improvement;
//   * after the loop the mask stays the loop's; H is refitted by one runKernel on the inliers and polished by the
//     Levenberg-Marquardt solver (at most 10 iterations) on its first eight entries.
// PARITY UNPINNED: cv2 and its sources are absent here.  Restated from memory and NOT confirmed against a real cv2:
//   * cv::eigen's pivot order (OpenCV takes the largest off-diagonal element of a row; the pairs are cyclic here) - both end
//     at the same eigenvector, whose sign cancels in H / H[8];
//   * the whole schedule of LMSolverImpl::run: lambda = 1, lc = 0.75, Rlo / Rhi = 0.25 / 0.75, the nu clamp to [2, 10], the
//     damping A + lambda diag(A) on the CURRENT A, both stopping thresholds at DBL_EPSILON, the |d.v| > DBL_EPSILON guard;
//   * solve / invert(DECOMP_EIG) inside it: Gaussian elimination with partial pivoting here;
//   * the division by H[8] (OpenCV multiplies by the reciprocal) and the order of the sums over the points.
// tests/homography_ref.py restates the same and says the same.
//
// fp64 with no fused multiply-add in this file (the error is float, as in OpenCV): the restatement has separate operations.
//
// Launches, laid out like ransac_kernels.hip: head [control block, the samples of chunk 0: one lane replays the RNG] - per
// chunk [workgroup per sample: lane 0 solves the 4-point DLT, 9 x 9 Jacobi in LDS, then the workgroup scores the model against
// every match] and [one lane replays best / budget over the stored counts, then draws the next chunk's samples] - tail [one
// workgroup of 1024: the last replay, the winner's mask, the inliers compacted, the refit (4 + 4 + 45 sums) and the whole LM
// polish (36 + 8 + 1 sums per evaluation): fixed-order block sums, the 9 x 9 Jacobi and the 8 x 8 solves on one lane].  The
// polish is a chain of dependent reductions - latency, not work - so it stays inside one launch.  Chunks {8, 128, the
// rest}: a budget that collapses after the first good sample costs four early-exit launches.  The result does not depend
// on the chunking: a chunk only computes what the sequential loop would have looked at.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)
#include "geom_common.hpp"

namespace {

constexpr int HG_MAX_ITERS = 2000;       // cv::findHomography default maxIters (and OpenCV's clamp)
constexpr int HG_MP = 4;                 // model points
constexpr int HG_T = 256;                // the scoring workgroup
constexpr int HG_TAIL_T = 1024;          // the one-workgroup tail
constexpr int HG_SUBSET_ATTEMPTS = 10000;
constexpr int HG_MAX_N = 16384;
constexpr int HG_JACOBI_SWEEPS = 30;
constexpr int HG_LM_ITERS = 10;
constexpr int HG_NSUM = 45;              // LtL's upper triangle; also JtJ's (36) + Jtr (8) + the squared residual

struct HGCtrl {
    int n_subsets;      // samples drawn so far
    int niters;         // iterations the sequential loop has run
    int best_h;         // winning sample (-1: none)
    int best_count;     // its inliers
    int budget;         // the loop's current iteration budget
    int max_good;
    int exhausted;      // getSubset failed: the loop ended
    int lm_iters;
    unsigned long long rng_state;
    double H[9];
};

struct HGArgs {
    int n, max_iters;
    int direct;                               // n == 4: one runKernel on the four matches, no loop
    int h0, h1;                               // sample range of this chunk
    double thresh, confidence;
    const float* p1; const float* p2;         // [n][2] source / destination
    int* subsets;                             // [max_iters][4]
    double* models;                           // [max_iters][9]
    int* nmodels;                             // [max_iters]
    int* counts;                              // [max_iters]
    unsigned char* mask;                      // [n]
    int* inl;                                 // [n] the inliers' indices, in match order
    HGCtrl* ctrl;
};

// det [[x, y, 1] ...] of three points, cv::Matx33d's expansion
__device__ __forceinline__ double hg_det_ones(const float* p, const int* idx, int i0, int i1, int i2) {
    const double a = p[2 * idx[i0]], b = p[2 * idx[i0] + 1], c = p[2 * idx[i1]], d = p[2 * idx[i1] + 1];
    const double e = p[2 * idx[i2]], f = p[2 * idx[i2] + 1];
    return a * (d * 1.0 - f * 1.0) - b * (c * 1.0 - e * 1.0) + 1.0 * (c * f - e * d);
}

// HomographyEstimatorCallback::checkSubset on four points
__device__ bool hg_check_subset(const float* p1, const float* p2, const int* idx) {
    if (sslam::last_point_collinear(p1, idx, HG_MP) || sslam::last_point_collinear(p2, idx, HG_MP)) return false;
    const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        negative += hg_det_ones(p1, idx, tt[i][0], tt[i][1], tt[i][2]) * hg_det_ones(p2, idx, tt[i][0], tt[i][1], tt[i][2]) < 0;
    return negative == 0 || negative == 4;
}

// ---- 1. replay the sample stream for samples [h0, h1) (one lane) ---------------------------------------------------
__device__ void hg_subsets_step(const HGArgs& a, int h0, int h1) {
    HGCtrl* c = a.ctrl;
    if (c->exhausted || !(h0 < min(h1, c->budget)) || h0 != c->niters) return;
    sslam::CvRng rng{c->rng_state};
    const int end = min(h1, c->budget);
    int made = c->n_subsets;
    for (int it = h0; it < end; ++it) {
        int idx[HG_MP];
        int attempts = 0;
        for (; attempts < HG_SUBSET_ATTEMPTS; ++attempts) {
            sslam::draw_distinct<HG_MP>(rng, a.n, idx);
            if (hg_check_subset(a.p1, a.p2, idx)) break;
        }
        if (attempts == HG_SUBSET_ATTEMPTS) { c->exhausted = 1; break; }      // getSubset failed: the loop ends here
#pragma unroll
        for (int i = 0; i < HG_MP; ++i) a.subsets[it * HG_MP + i] = idx[i];
        ++made;
    }
    c->n_subsets = made;
    c->rng_state = rng.state;
}

// ---- 2. the small dense solvers, one lane, matrices in LDS (run-time indices) ---------------------------------------
// Cyclic Jacobi on the symmetric 9 x 9 A (destroyed): the pairs (p, q), p < q, row by row; a pair is left alone when
// |a_pq| <= 1e-18 trace; at most 30 sweeps.  V's columns become the eigenvectors; returns the column of the smallest
// eigenvalue (the first of equals).
__device__ int hg_jacobi9(double* A, double* V) {
    double tr = 0;
    for (int i = 0; i < 9; ++i) {
        for (int j = 0; j < 9; ++j) V[i * 9 + j] = i == j ? 1.0 : 0.0;
        tr += A[i * 9 + i];
    }
    const double thr = 1e-18 * tr;
    for (int sweep = 0; sweep < HG_JACOBI_SWEEPS; ++sweep) {
        bool changed = false;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[p * 9 + q];
                if (!(fabs(apq) > thr)) continue;
                changed = true;
                const double theta = (A[q * 9 + q] - A[p * 9 + p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
                for (int k = 0; k < 9; ++k) {
                    const double mp = A[k * 9 + p], mq = A[k * 9 + q];
                    A[k * 9 + p] = c * mp - s * mq;
                    A[k * 9 + q] = s * mp + c * mq;
                    const double vp = V[k * 9 + p], vq = V[k * 9 + q];
                    V[k * 9 + p] = c * vp - s * vq;
                    V[k * 9 + q] = s * vp + c * vq;
                }
                for (int k = 0; k < 9; ++k) {
                    const double rp = A[p * 9 + k], rq = A[q * 9 + k];
                    A[p * 9 + k] = c * rp - s * rq;
                    A[q * 9 + k] = s * rp + c * rq;
                }
            }
        if (!changed) break;
    }
    int best = 0;
    for (int i = 1; i < 9; ++i)
        if (A[i * 9 + i] < A[best * 9 + best]) best = i;
    return best;
}

// The normalisation of runKernel: centroids and count / (sum of absolute deviations) of both point sets.
struct HGNorm { double cMx, cMy, cmx, cmy, sMx, sMy, smx, smy; };

// LtL's upper triangle (row by row, 45 entries) of one match, normalised: added to acc
__device__ __forceinline__ void hg_ltl_add(const HGNorm& N, float Xf, float Yf, float xf, float yf, double (&acc)[HG_NSUM]) {
    const double x = ((double)xf - N.cmx) * N.smx, y = ((double)yf - N.cmy) * N.smy;
    const double X = ((double)Xf - N.cMx) * N.sMx, Y = ((double)Yf - N.cMy) * N.sMy;
    const double Lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
    const double Ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
    int o = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k) acc[o++] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
}

// The rest of runKernel by one lane: LtL from its upper triangle `tri`, its smallest eigenvector, H = invHnorm H0 Hnorm2,
// divided by H[8].  A, V: 81 doubles of LDS each.
__device__ void hg_dlt_finish(const double* tri, const HGNorm& N, double* A, double* V, double* H) {
    int o = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k) { A[j * 9 + k] = tri[o]; A[k * 9 + j] = tri[o]; ++o; }
    const int col = hg_jacobi9(A, V);
    double h0[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) h0[i] = V[i * 9 + col];
    const double inv[9] = {1.0 / N.smx, 0, N.cmx, 0, 1.0 / N.smy, N.cmy, 0, 0, 1};
    const double nrm[9] = {N.sMx, 0, -N.cMx * N.sMx, 0, N.sMy, -N.cMy * N.sMy, 0, 0, 1};
    double T[9], R[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[3 * r + c] = (inv[3 * r] * h0[c] + inv[3 * r + 1] * h0[3 + c]) + inv[3 * r + 2] * h0[6 + c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (T[3 * r] * nrm[c] + T[3 * r + 1] * nrm[3 + c]) + T[3 * r + 2] * nrm[6 + c];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = R[i] / R[8];
}

// runKernel on the four matches idx[0..4) by one lane; returns the number of models (0 or 1)
__device__ int hg_solve4(const HGArgs& a, const int* idx, double* tri, double* A, double* V, double* H) {
    double Xs[4], Ys[4], xs[4], ys[4];
    HGNorm N{};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        Xs[i] = a.p1[2 * idx[i]]; Ys[i] = a.p1[2 * idx[i] + 1]; xs[i] = a.p2[2 * idx[i]]; ys[i] = a.p2[2 * idx[i] + 1];
        N.cMx += Xs[i]; N.cMy += Ys[i]; N.cmx += xs[i]; N.cmy += ys[i];
    }
    N.cMx /= 4; N.cMy /= 4; N.cmx /= 4; N.cmy /= 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        N.sMx += fabs(Xs[i] - N.cMx); N.sMy += fabs(Ys[i] - N.cMy); N.smx += fabs(xs[i] - N.cmx); N.smy += fabs(ys[i] - N.cmy);
    }
    if (N.sMx < DBL_EPSILON || N.sMy < DBL_EPSILON || N.smx < DBL_EPSILON || N.smy < DBL_EPSILON) return 0;
    N.sMx = 4 / N.sMx; N.sMy = 4 / N.sMy; N.smx = 4 / N.smx; N.smy = 4 / N.smy;
    double acc[HG_NSUM];
#pragma unroll
    for (int i = 0; i < HG_NSUM; ++i) acc[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) hg_ltl_add(N, (float)Xs[i], (float)Ys[i], (float)xs[i], (float)ys[i], acc);
#pragma unroll
    for (int i = 0; i < HG_NSUM; ++i) tri[i] = acc[i];
    hg_dlt_finish(tri, N, A, V, H);
    return 1;
}

// HomographyEstimatorCallback::computeError of one match: float throughout
__device__ __forceinline__ float hg_error(const float* Hf, float X, float Y, float x, float y) {
    const float ww = 1.f / ((Hf[6] * X + Hf[7] * Y) + 1.f);
    const float dx = ((Hf[0] * X + Hf[1] * Y) + Hf[2]) * ww - x;
    const float dy = ((Hf[3] * X + Hf[4] * Y) + Hf[5]) * ww - y;
    return dx * dx + dy * dy;
}

// ---- 2 + 3. solve sample h and score its model against every match (workgroup / sample) ----------------------------
__global__ __launch_bounds__(HG_T) void hg_models_score_kernel(HGArgs a) {
    __shared__ double sA[81], sV[81], sTri[HG_NSUM], sH[9];
    __shared__ float Hf[9];
    __shared__ int sh[HG_T];
    __shared__ int s_nm;
    const int h = a.h0 + blockIdx.x;
    const HGCtrl* c = a.ctrl;
    if (h >= a.h1 || h >= c->n_subsets || a.h0 != c->niters) return;     // (beyond the samples drawn / the loop ended before this chunk)
    if (threadIdx.x == 0) {
        int idx[HG_MP];
#pragma unroll
        for (int i = 0; i < HG_MP; ++i) idx[i] = a.subsets[h * HG_MP + i];
        const int nm = hg_solve4(a, idx, sTri, sA, sV, sH);
        for (int i = 0; i < 9; ++i) { a.models[(size_t)h * 9 + i] = nm ? sH[i] : 0.0; Hf[i] = nm ? (float)sH[i] : 0.f; }
        a.nmodels[h] = nm;
        s_nm = nm;
    }
    __syncthreads();
    if (!s_nm || a.direct) {                                            // (uniform; the four-match path does not score)
        if (threadIdx.x == 0) a.counts[h] = 0;
        return;
    }
    const float t = (float)(a.thresh * a.thresh);
    int good = 0;
    for (int i = threadIdx.x; i < a.n; i += HG_T)
        good += hg_error(Hf, a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1]) <= t;
    good = sslam::block_sum<HG_T>(good, sh);
    if (threadIdx.x == 0) a.counts[h] = good;
}

// ---- 4. replay the sequential best / budget logic over samples [h0, h1) (one lane) ---------------------------------
__device__ void hg_select_step(const HGArgs& a, int h0, int h1) {
    HGCtrl* c = a.ctrl;
    int it = h0;
    if (it != c->niters) return;                       // the loop already ended before this chunk
    for (; it < h1 && it < c->n_subsets && it < c->budget; ++it) {
        if (!a.nmodels[it]) continue;
        const int good = a.counts[it];
        if (good > max(c->max_good, HG_MP - 1)) {
            c->max_good = good;
            c->best_h = it;
            c->budget = sslam::update_num_iters(a.confidence, (double)(a.n - good) / a.n, HG_MP, c->budget);
        }
    }
    c->niters = it;
}

// ---- first launch: the control block and the samples of the first chunk --------------------------------------------
__global__ __launch_bounds__(64) void hg_head_kernel(HGArgs a) {
    if (threadIdx.x != 0) return;
    HGCtrl* c = a.ctrl;
    c->budget = a.max_iters;
    c->rng_state = 0xffffffffffffffffULL;
    c->n_subsets = 0; c->exhausted = 0; c->best_h = -1; c->best_count = 0; c->niters = 0; c->max_good = 0; c->lm_iters = 0;
    for (int i = 0; i < 9; ++i) c->H[i] = 0;
    if (a.direct) {
        for (int i = 0; i < HG_MP; ++i) a.subsets[i] = i;
        c->n_subsets = 1;
        return;
    }
    hg_subsets_step(a, a.h0, a.h1);
}

// ---- between chunks: the replay over the chunk just scored [h0, h1), then the samples of the next [h1, h2) ----------
__global__ __launch_bounds__(64) void hg_step_kernel(HGArgs a, int h2) {
    if (threadIdx.x != 0) return;
    hg_select_step(a, a.h0, a.h1);
    hg_subsets_step(a, a.h1, h2);
}

// ---- the polish's pieces --------------------------------------------------------------------------------------------
// A x = b (8 x 8) by Gaussian elimination with partial pivoting (the first of equal pivots) on W = [A | b] (8 x 9, LDS,
// destroyed); false when a pivot is zero or not finite
__device__ bool hg_gauss8(double* W, double* x) {
    for (int k = 0; k < 8; ++k) {
        int piv = k;
        for (int i = k + 1; i < 8; ++i)
            if (fabs(W[i * 9 + k]) > fabs(W[piv * 9 + k])) piv = i;
        const double pv = W[piv * 9 + k];
        if (pv == 0 || !(fabs(pv) <= DBL_MAX)) return false;
        if (piv != k)
            for (int j = 0; j < 9; ++j) { const double tmp = W[k * 9 + j]; W[k * 9 + j] = W[piv * 9 + j]; W[piv * 9 + j] = tmp; }
        for (int i = k + 1; i < 8; ++i) {
            const double f = W[i * 9 + k] / W[k * 9 + k];
            for (int j = k; j < 8; ++j) W[i * 9 + j] = W[i * 9 + j] - f * W[k * 9 + j];
            W[i * 9 + 8] = W[i * 9 + 8] - f * W[k * 9 + 8];
        }
    }
    for (int i = 7; i >= 0; --i) {
        double acc = W[i * 9 + 8];
        for (int j = i + 1; j < 8; ++j) acc = acc - W[i * 9 + j] * x[j];
        x[i] = acc / W[i * 9 + i];
    }
    return true;
}

// The residuals of HomographyRefineCallback at h (8 entries) over this thread's inliers: the upper triangle of JtJ
// (acc[0 .. 36)), Jtr (acc[36 .. 44)), the squared residual (acc[44]); returns the largest |residual|
__device__ __forceinline__ double hg_lm_accumulate(const HGArgs& a, int m, const double* h, double (&acc)[HG_NSUM]) {
#pragma unroll
    for (int i = 0; i < HG_NSUM; ++i) acc[i] = 0;
    double rmax = 0;
    const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7];
    for (int o = threadIdx.x; o < m; o += HG_TAIL_T) {
        const int i = a.inl[o];
        const double X = a.p1[2 * i], Y = a.p1[2 * i + 1], mx = a.p2[2 * i], my = a.p2[2 * i + 1];
        const double den = (h6 * X + h7 * Y) + 1.0;
        const double ww = fabs(den) < DBL_EPSILON ? 0.0 : 1.0 / den;
        const double xi = ((h0 * X + h1 * Y) + h2) * ww, yi = ((h3 * X + h4 * Y) + h5) * ww;
        const double rx = xi - mx, ry = yi - my;
        const double Jx[8] = {X * ww, Y * ww, ww, 0, 0, 0, -X * ww * xi, -Y * ww * xi};
        const double Jy[8] = {0, 0, 0, X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi};
        int k = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int l = j; l < 8; ++l) acc[k++] += Jx[j] * Jx[l] + Jy[j] * Jy[l];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[36 + j] += Jx[j] * rx + Jy[j] * ry;
        acc[44] += rx * rx + ry * ry;
        rmax = fmax(rmax, fmax(fabs(rx), fabs(ry)));
    }
    return rmax;
}

// sums[45] of hg_lm_accumulate -> A (8 x 8, mirrored), v (8); returns the squared residual (one lane)
__device__ double hg_lm_unpack(const double* sums, double* A, double* v) {
    int k = 0;
    for (int j = 0; j < 8; ++j)
        for (int l = j; l < 8; ++l) { A[j * 8 + l] = sums[k]; A[l * 8 + j] = sums[k]; ++k; }
    for (int j = 0; j < 8; ++j) v[j] = sums[36 + j];
    return sums[44];
}

// ---- last launch: the replay over the last chunk, the winner and the loop's mask; then the refit on the inliers and
// the LM polish, all in this workgroup --------------------------------------------------------------------------------
__global__ __launch_bounds__(HG_TAIL_T) void hg_tail_kernel(HGArgs a) {
    __shared__ double part[(HG_TAIL_T / 64) * HG_NSUM], sums[HG_NSUM], smax[HG_TAIL_T];
    __shared__ double sA[81], sV[81], sH[9];
    __shared__ double lA[64], lv[8], lx[8], lxd[8], ld[8], lW[72], lAinv[8];
    __shared__ float Hf[9];
    __shared__ int wsum[HG_TAIL_T / 64], base, s_flag;
    __shared__ HGNorm sN;
    HGCtrl* c = a.ctrl;
    const int n = a.n;
    if (threadIdx.x == 0) {
        if (a.direct) c->best_h = a.nmodels[0] ? 0 : -1;
        else hg_select_step(a, a.h0, a.h1);
        if (c->best_h >= 0)
            for (int i = 0; i < 9; ++i) { sH[i] = a.models[(size_t)c->best_h * 9 + i]; Hf[i] = (float)sH[i]; }
        base = 0;
    }
    __syncthreads();
    const bool have = c->best_h >= 0;
    const float t = (float)(a.thresh * a.thresh);
    // the loop's mask (four matches: all ones) and the inliers' indices in match order, 1024 matches per turn
    for (int i0 = 0; i0 < n; i0 += HG_TAIL_T) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < n && have && (a.direct || hg_error(Hf, a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1]) <= t);
        if (i < n) a.mask[i] = (unsigned char)keep;
        sslam::block_compact<HG_TAIL_T>(keep, wsum, base, [&](int o) { a.inl[o] = i; });
    }
    const int m = base;
    if (!have || a.direct) {                             // (uniform) no model, or the four-match path: nothing to refine
        if (threadIdx.x == 0) {
            c->best_count = m;
            if (have) for (int i = 0; i < 9; ++i) c->H[i] = sH[i];
        }
        return;
    }
    // ---- the refit: runKernel on the inliers (a.inl is read by the threads that wrote it and by others: barriers above)
    {
        double s4[4] = {0, 0, 0, 0};
        for (int o = threadIdx.x; o < m; o += HG_TAIL_T) {
            const int i = a.inl[o];
            s4[0] += a.p1[2 * i]; s4[1] += a.p1[2 * i + 1]; s4[2] += a.p2[2 * i]; s4[3] += a.p2[2 * i + 1];
        }
        sslam::block_sum_n<HG_TAIL_T, 4>(s4, part, sums);
        const double cMx = sums[0] / m, cMy = sums[1] / m, cmx = sums[2] / m, cmy = sums[3] / m;
        double d4[4] = {0, 0, 0, 0};
        for (int o = threadIdx.x; o < m; o += HG_TAIL_T) {
            const int i = a.inl[o];
            d4[0] += fabs(a.p1[2 * i] - cMx); d4[1] += fabs(a.p1[2 * i + 1] - cMy);
            d4[2] += fabs(a.p2[2 * i] - cmx); d4[3] += fabs(a.p2[2 * i + 1] - cmy);
        }
        sslam::block_sum_n<HG_TAIL_T, 4>(d4, part, sums);
        const bool ok = !(sums[0] < DBL_EPSILON || sums[1] < DBL_EPSILON || sums[2] < DBL_EPSILON || sums[3] < DBL_EPSILON);
        HGNorm N{cMx, cMy, cmx, cmy, m / sums[0], m / sums[1], m / sums[2], m / sums[3]};
        if (ok) {                                        // (uniform: every thread holds the same sums)
            double acc[HG_NSUM];
#pragma unroll
            for (int i = 0; i < HG_NSUM; ++i) acc[i] = 0;
            for (int o = threadIdx.x; o < m; o += HG_TAIL_T) {
                const int i = a.inl[o];
                hg_ltl_add(N, a.p1[2 * i], a.p1[2 * i + 1], a.p2[2 * i], a.p2[2 * i + 1], acc);
            }
            sslam::block_sum_n<HG_TAIL_T, HG_NSUM>(acc, part, sums);
            if (threadIdx.x == 0) hg_dlt_finish(sums, N, sA, sV, sH);          // a return of 0 leaves H as it was
        }
    }
    // ---- the polish: LMSolver on H's first eight entries
    __syncthreads();                                     // (thread 0 is done with `sums`; sH is final)
    if (threadIdx.x == 0)
        for (int i = 0; i < 8; ++i) lx[i] = sH[i];
    __syncthreads();
    double acc[HG_NSUM];
    double rmax = hg_lm_accumulate(a, m, lx, acc);
    sslam::block_sum_n<HG_TAIL_T, HG_NSUM>(acc, part, sums);
    double r_inf = sslam::block_max<HG_TAIL_T>(rmax, smax);
    double S = 0, lambda = 1.0, lc = 0.75;               // (thread 0's own)
    int iter = 0;
    if (threadIdx.x == 0) S = hg_lm_unpack(sums, lA, lv);
    for (;;) {
        if (threadIdx.x == 0) {
            for (int i = 0; i < 8; ++i) {
                for (int j = 0; j < 8; ++j) lW[i * 9 + j] = lA[i * 8 + j];
                lW[i * 9 + i] = lA[i * 8 + i] + lambda * lA[i * 8 + i];
                lW[i * 9 + 8] = lv[i];
            }
            const bool ok = hg_gauss8(lW, ld);
            bool finite = ok;
            if (ok) for (int i = 0; i < 8; ++i) finite = finite && fabs(ld[i]) <= DBL_MAX;
            if (finite) for (int i = 0; i < 8; ++i) lxd[i] = lx[i] - ld[i];
            s_flag = finite ? 0 : 1;
        }
        __syncthreads();
        if (s_flag) break;                               // (uniform) the step could not be solved
        rmax = hg_lm_accumulate(a, m, lxd, acc);
        sslam::block_sum_n<HG_TAIL_T, HG_NSUM>(acc, part, sums);
        const double rd_inf = sslam::block_max<HG_TAIL_T>(rmax, smax);
        if (threadIdx.x == 0) {
            const double Sd = sums[44];
            double dS = 0, dv = 0, dmax = 0;
            for (int i = 0; i < 8; ++i) {
                double Ad = 0;
                for (int j = 0; j < 8; ++j) Ad += lA[i * 8 + j] * ld[j];
                dS += ld[i] * (2.0 * lv[i] - Ad);
                dv += ld[i] * lv[i];
                dmax = fmax(dmax, fabs(ld[i]));
            }
            const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1.0);
            if (R > 0.75) {
                lambda *= 0.5;
                if (lambda < lc) lambda = 0;
            } else if (R < 0.25) {
                double nu = (Sd - S) / (fabs(dv) > DBL_EPSILON ? dv : 1.0) + 2.0;
                nu = fmin(fmax(nu, 2.0), 10.0);
                if (lambda == 0) {
                    double maxval = DBL_EPSILON;
                    bool ok = true;
                    for (int k = 0; k < 8 && ok; ++k) {        // diag(A^-1), a column at a time
                        for (int i = 0; i < 8; ++i) {
                            for (int j = 0; j < 8; ++j) lW[i * 9 + j] = lA[i * 8 + j];
                            lW[i * 9 + 8] = i == k ? 1.0 : 0.0;
                        }
                        ok = hg_gauss8(lW, lAinv);
                        if (ok) maxval = fmax(maxval, fabs(lAinv[k]));
                    }
                    if (!ok) maxval = DBL_EPSILON;
                    lambda = lc = 1.0 / maxval;
                    nu *= 0.5;
                }
                lambda *= nu;
            }
            if (Sd < S) {
                for (int i = 0; i < 8; ++i) lx[i] = lxd[i];
                S = hg_lm_unpack(sums, lA, lv);
                r_inf = rd_inf;
            }
            ++iter;
            s_flag = !(iter < HG_LM_ITERS && dmax >= DBL_EPSILON && r_inf >= DBL_EPSILON);
        }
        __syncthreads();
        if (s_flag) break;
        __syncthreads();                                 // (s_flag is written again at the top of the next turn)
    }
    if (threadIdx.x == 0) {
        c->best_count = m;
        c->lm_iters = iter;
        for (int i = 0; i < 8; ++i) c->H[i] = lx[i];
        c->H[8] = 1.0;
    }
}

// the slab-backed pointers of HGArgs, in slab order
void hg_bind(sslam::Slab& sl, HGArgs& a, size_t N, size_t H) {
    a.p1 = sl.take<float>(N * 2); a.p2 = sl.take<float>(N * 2); a.subsets = sl.take<int>(H * HG_MP);
    a.models = sl.take<double>(H * 9); a.nmodels = sl.take<int>(H); a.counts = sl.take<int>(H);
    a.mask = sl.take<unsigned char>(N); a.inl = sl.take<int>(N); a.ctrl = sl.take<HGCtrl>(1);
}

}  // namespace

extern "C" int sslam_homography_ransac_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, double thresh,
                                            double confidence, int max_iters, unsigned char* mask_out, double* H_out,
                                            int32_t* info_out) {
    const char* who = "sslam_homography_ransac_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= HG_MP, "%s: %d matches, a homography needs at least %d", who, n, HG_MP);
    SSLAM_REQUIRE(n <= HG_MAX_N, "%s: %d matches, at most %d are supported", who, n, HG_MAX_N);
    SSLAM_REQUIRE(pts1 && pts2 && mask_out, "%s: NULL argument", who);
    // cv::findHomography's own defaulting of bad parameters
    if (thresh <= 0) thresh = 3;
    if (!(confidence > 0 && confidence < 1)) confidence = 0.995;
    max_iters = std::min(std::max(max_iters, 1), HG_MAX_ITERS);
    const bool direct = n == HG_MP;
    if (direct) max_iters = 1;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    HGArgs a{};
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { hg_bind(sl, a, N, (size_t)max_iters); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p1, pts1, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p2, pts2, N * 2));
    a.n = n; a.max_iters = max_iters; a.direct = direct; a.thresh = thresh; a.confidence = confidence;
    const auto bounds = sslam::ransac_chunk_bounds(max_iters, 128);     // (the schedule: geom_slab.hpp)
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    a.h0 = bounds[0]; a.h1 = bounds[1];
    hipLaunchKernelGGL(hg_head_kernel, dim3(1), dim3(64), 0, s, a);
    for (int ci = 0; ci < 3; ++ci) {
        a.h0 = bounds[ci]; a.h1 = bounds[ci + 1];
        if (a.h1 > a.h0) hipLaunchKernelGGL(hg_models_score_kernel, dim3(a.h1 - a.h0), dim3(HG_T), 0, s, a);
        if (ci < 2) hipLaunchKernelGGL(hg_step_kernel, dim3(1), dim3(64), 0, s, a, bounds[ci + 2]);
    }
    hipLaunchKernelGGL(hg_tail_kernel, dim3(1), dim3(HG_TAIL_T), 0, s, a);       // (a.h0, a.h1: the last chunk)
    SSLAM_HIP_CHECK(hipGetLastError());
    HGCtrl h{};
    SSLAM_HIP_CHECK(sslam::copy_down(s, &h, a.ctrl, 1));
    SSLAM_HIP_CHECK(sslam::copy_down(s, mask_out, a.mask, N));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (H_out) for (int i = 0; i < 9; ++i) H_out[i] = h.best_h >= 0 ? h.H[i] : 0.0;
    if (info_out) {
        info_out[0] = h.best_h >= 0 ? h.best_count : -1;      // -1: no model (cv2 returns (None, None))
        info_out[1] = direct ? 0 : h.niters;
        info_out[2] = 0;
        info_out[3] = h.best_h;
    }
    return 0;
}
