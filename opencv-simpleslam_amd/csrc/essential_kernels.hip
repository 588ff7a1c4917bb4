// essential_kernels.hip - essential-matrix RANSAC on the GPU: the five-point leg of the reference's tracking-lost fallback.
//
// Replaces `cv2.findEssentialMat(pts0, pts1, K, cv2.RANSAC, 0.999, thresh)` as the frame loops call it when tracking is
// lost (slam/monocular/main_revamped.py:512, main.py:402, main4.py:457); `sslam_recover_pose_host` takes its E and mask.
//
// The algorithm is OpenCV 4.x's classic (non-USAC) path, restated (five-point.cpp, ptsetreg.cpp):
//   * points widened to double and normalised (x - cx) / fx, (y - cy) / fy; the threshold divided by (fx + fy) / 2;
//   * 5 matches: one runKernel on them, mask all ones, E = every model stacked;
//   * more: RANSAC with cv::RNG (state 2^64-1); getSubset draws 5 distinct indices, no checkSubset; runKernel = Nister's
//     five-point solver, up to ten models; every model scored in order by the Sampson distance in double stored as float,
//     inlier iff err <= (float)(t^2); best = count strictly above max(best so far, 4); the budget re-estimated after
//     every improvement; no refit and no polish after the loop.
//   * runKernel: the 5 x 9 epipolar matrix, its four-dimensional right null space e0..e3, the ten cubic constraints on
//     E = x e0 + y e1 + z e2 + e3 as a 10 x 20 matrix, elimination of its left 10 x 10 block, the tenth-degree polynomial in
//     z, its real roots, per root (x, y) from the null vector of a 3 x 3 matrix, E divided by its Frobenius norm.
// PARITY UNPINNED: cv2 and its sources are absent here.  Restated from memory and NOT confirmed against a real cv2:
//   * the null-space basis: a one-sided Jacobi on the five rows, then rows 5..8 filled the way OpenCV's own JacobiSVD fills
//     them for FULL_UV (+-1/9 vectors from cv::RNG(0x12345678), `next() & 256` the sign, two Gram-Schmidt passes with an L1
//     rescale after every projection); a cv2 built on LAPACK returns another basis of the same space;
//   * getCoeffMat: here det E and the nine entries of (E E' - tr(E E') / 2) E, columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2
//     xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1 - the same ideal, other rows than OpenCV's generated ones;
//   * the elimination: Gauss-Jordan with partial pivoting for OpenCV's LU solve;
//   * solvePoly: Durand-Kerner from the start values (1 + i)^k, at most 300 iterations - but all ten roots updated at once,
//     not in place, stopping once every step is within 1e-14 (1 + |re| + |im|); a zero leading coefficient gives no model;
//   * the two 1e-10 tests (|imag| of a kept root; the last entry of the unit null vector, found here as the largest cross
//     product of two rows and not by an SVD);
//   * whether E is normalised (it is here) and the order of the models (the order of the root finder's slots).
// A different basis changes the order and the rounding of a sample's models, not their set; any converged root finder
// finds the same real roots.  tests/essential_ref.py restates the same and says the same.
//
// fp64 with no fused multiply-add in this file (only the stored error is float): the restatement has separate operations
// in the same order.
//
// Launches, laid out like homography_kernels.hip: normalise [thread per match] - head [control block, the samples of chunk
// 0: one lane replays the RNG] - per chunk [workgroup per sample: lane 0 runs the five-point solve with every run-time
// indexed matrix in LDS, then the workgroup scores all of the sample's models in ONE pass over the matches, ten counts
// reduced together] and [one lane replays best / budget over the stored counts, sample by sample and model by model, then
// draws the next chunk's samples] - tail [one workgroup of 1024: the last replay, the winner's E read back from the stored
// models, its mask and count].  Chunks {8, 128, the rest}.  The result does not depend on the chunking: a chunk only computes
// what the sequential loop would have looked at.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>

#pragma clang fp contract(off)
#include "geom_common.hpp"

namespace {

constexpr int EM_DEFAULT_ITERS = 1000;   // cv::findEssentialMat default maxIters
constexpr int EM_MAX_ITERS = 2000;       // the clamp: the slab holds max_iters x 10 models
constexpr int EM_MP = 5;                 // model points
constexpr int EM_MAXM = 10;              // models per sample
constexpr int EM_T = 256;                // the scoring workgroup
constexpr int EM_TAIL_T = 1024;          // the one-workgroup tail
constexpr int EM_MAX_N = 16384;
constexpr int EM_JACOBI_SWEEPS = 30;
constexpr int EM_POLY_ITERS = 300;
constexpr double EM_POLY_TOL = 1e-14;

struct EMCtrl {
    int n_subsets;      // samples drawn so far
    int niters;         // iterations the sequential loop has run
    int best_h;         // winning sample (-1: none)
    int best_m;         // the winner's index within its sample (five matches: the number of models)
    int best_count;     // its inliers
    int budget;         // the loop's current iteration budget
    int max_good;
    int pad;
    unsigned long long rng_state;
    double E[EM_MAXM * 9];
};

struct EMArgs {
    int n, max_iters;
    int direct;                               // n == 5: one runKernel on the five matches, no loop
    int h0, h1;                               // sample range of this chunk
    float t;                                  // the squared, normalised threshold
    double prob, fx, fy, cx, cy;
    const float* p1; const float* p2;         // [n][2] pixels
    double* xn;                               // [n][4] normalised x1 y1 x2 y2
    int* subsets;                             // [max_iters][5]
    double* models;                           // [max_iters][10][9]
    int* nmodels;                             // [max_iters]
    int* counts;                              // [max_iters][10]
    unsigned char* mask;                      // [n]
    EMCtrl* ctrl;
};

// monomials of x, y, z.  linear: x y z 1; quadratic: x^2 xy xz x y^2 yz y z^2 z 1; cubic: the 20 columns named above
__constant__ int EM_T12[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
__constant__ int EM_T23[10][4] = {{0, 2, 4, 5},    {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},   {3, 1, 6, 7},
                                  {8, 6, 13, 14},  {9, 7, 14, 15},   {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// LDS of the one-lane solve: everything indexed at run time lives here
struct EMSolve {
    double V[81];        // rows 0..4: the epipolar rows, orthogonalised; rows 5..8: e0..e3
    double Q[90];        // E E' (3 x 3 quadratics), then E E' - tr / 2
    double tr[10];
    double M[200];       // the 10 x 20 constraints
    double Mn[30];       // the three minors of det E
    double B[39];        // three rows of kx[4] ky[4] k1[5], ascending in z
    double cof[24];      // cx[8] cy[8] c1[7]
    double pq[16];
    double det[11], tmp[33];
    double a[10], zr[10], zi[10], nr[10], ni[10];
};

// ---- 1. replay the sample stream for samples [h0, h1) (one lane) ---------------------------------------------------
__device__ void em_subsets_step(const EMArgs& a, int h0, int h1) {
    EMCtrl* c = a.ctrl;
    if (!(h0 < min(h1, c->budget)) || h0 != c->niters) return;
    sslam::CvRng rng{c->rng_state};
    const int end = min(h1, c->budget);
    for (int it = h0; it < end; ++it) {
        int idx[EM_MP];
        sslam::draw_distinct<EM_MP>(rng, a.n, idx);
#pragma unroll
        for (int i = 0; i < EM_MP; ++i) a.subsets[it * EM_MP + i] = idx[i];
    }
    c->n_subsets = end;
    c->rng_state = rng.state;
}

// ---- 2. the five-point solve, one lane --------------------------------------------------------------------------------
// One-sided Jacobi on rows 0..4 of V (pairs (i, j), i < j; a pair is left alone when |p| <= 10 eps sqrt(a b); at most 30
// sweeps), the rows scaled to unit length; rows 5..8 filled the way OpenCV's JacobiSVD completes a basis.
__device__ void em_null_space(double* V) {
    const double eps = DBL_EPSILON * 10;
    for (int sweep = 0; sweep < EM_JACOBI_SWEEPS; ++sweep) {
        bool changed = false;
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 5; ++j) {
                double aa = 0, bb = 0, p = 0;
                for (int k = 0; k < 9; ++k) {
                    const double ai = V[i * 9 + k], aj = V[j * 9 + k];
                    aa += ai * ai; bb += aj * aj; p += ai * aj;
                }
                if (fabs(p) <= eps * sqrt(aa * bb)) continue;
                changed = true;
                p *= 2;
                const double beta = aa - bb, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    s = sqrt((gamma - beta) * 0.5 / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                for (int k = 0; k < 9; ++k) {
                    const double ai = V[i * 9 + k], aj = V[j * 9 + k];
                    V[i * 9 + k] = c * ai + s * aj;
                    V[j * 9 + k] = c * aj - s * ai;
                }
            }
        if (!changed) break;
    }
    sslam::CvRng rng{0x12345678ULL};
    for (int i = 0; i < 9; ++i) {
        double sd = 0;
        if (i < 5) {
            for (int k = 0; k < 9; ++k) sd += V[i * 9 + k] * V[i * 9 + k];
            sd = sqrt(sd);
        }
        for (int tries = 0; tries < 100 && sd <= DBL_MIN; ++tries) {
            for (int k = 0; k < 9; ++k) V[i * 9 + k] = (rng.next() & 256) != 0 ? 1.0 / 9 : -(1.0 / 9);
            for (int pass = 0; pass < 2; ++pass)
                for (int j = 0; j < i; ++j) {
                    double d = 0;
                    for (int k = 0; k < 9; ++k) d += V[i * 9 + k] * V[j * 9 + k];
                    double asum = 0;
                    for (int k = 0; k < 9; ++k) {
                        const double t = V[i * 9 + k] - d * V[j * 9 + k];
                        V[i * 9 + k] = t;
                        asum += fabs(t);
                    }
                    asum = asum > eps * 100 ? 1.0 / asum : 0.0;
                    for (int k = 0; k < 9; ++k) V[i * 9 + k] = V[i * 9 + k] * asum;
                }
            sd = 0;
            for (int k = 0; k < 9; ++k) sd += V[i * 9 + k] * V[i * 9 + k];
            sd = sqrt(sd);
        }
        const double s = sd > DBL_MIN ? 1.0 / sd : 0.0;
        for (int k = 0; k < 9; ++k) V[i * 9 + k] = V[i * 9 + k] * s;
    }
}

// entry (r, c) of E as a linear polynomial: coefficient i (x y z 1) is e_i[r][c]
#define EM_L(S, r, c, i) (S).V[(5 + (i)) * 9 + (r) * 3 + (c)]

// the 10 x 20 matrix: row 0 = det E, rows 1..9 = (E E' - tr(E E') / 2) E; every sum in the restatement's order
__device__ void em_coeff_matrix(EMSolve& S) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double* q = S.Q + (r * 3 + c) * 10;
            for (int o = 0; o < 10; ++o) q[o] = 0;
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j) q[EM_T12[i][j]] += EM_L(S, r, k, i) * EM_L(S, c, k, j);
        }
    for (int o = 0; o < 10; ++o) S.tr[o] = (S.Q[o] + S.Q[40 + o]) + S.Q[80 + o];
    for (int d = 0; d < 3; ++d)
        for (int o = 0; o < 10; ++o) S.Q[d * 40 + o] = S.Q[d * 40 + o] - 0.5 * S.tr[o];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double* m = S.M + (1 + r * 3 + c) * 20;
            for (int o = 0; o < 20; ++o) m[o] = 0;
            for (int k = 0; k < 3; ++k)
                for (int q = 0; q < 10; ++q)
                    for (int i = 0; i < 4; ++i) m[EM_T23[q][i]] += S.Q[(r * 3 + k) * 10 + q] * EM_L(S, k, c, i);
        }
    for (int cc = 0; cc < 3; ++cc) {
        const int c1 = (cc + 1) % 3, c2 = (cc + 2) % 3;
        double* mn = S.Mn + cc * 10;
        for (int o = 0; o < 10; ++o) mn[o] = 0;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                const int o = EM_T12[i][j];
                mn[o] += EM_L(S, 1, c1, i) * EM_L(S, 2, c2, j);
                mn[o] -= EM_L(S, 1, c2, i) * EM_L(S, 2, c1, j);
            }
    }
    for (int o = 0; o < 20; ++o) S.M[o] = 0;
    for (int cc = 0; cc < 3; ++cc)
        for (int q = 0; q < 10; ++q)
            for (int i = 0; i < 4; ++i) S.M[EM_T23[q][i]] += S.Mn[cc * 10 + q] * EM_L(S, 0, cc, i);
}

// Gauss-Jordan with partial pivoting (the first of equal pivots) on the 10 x 20 M; false when a pivot is zero or not finite
__device__ bool em_eliminate(double* M) {
    for (int k = 0; k < 10; ++k) {
        int piv = k;
        for (int i = k + 1; i < 10; ++i)
            if (fabs(M[i * 20 + k]) > fabs(M[piv * 20 + k])) piv = i;
        const double pv = M[piv * 20 + k];
        if (pv == 0 || !(fabs(pv) <= DBL_MAX)) return false;
        if (piv != k)
            for (int j = 0; j < 20; ++j) { const double t = M[k * 20 + j]; M[k * 20 + j] = M[piv * 20 + j]; M[piv * 20 + j] = t; }
        for (int j = k; j < 20; ++j) M[k * 20 + j] = M[k * 20 + j] / pv;
        for (int i = 0; i < 10; ++i) {
            if (i == k) continue;
            const double f = M[i * 20 + k];
            for (int j = k; j < 20; ++j) M[i * 20 + j] = M[i * 20 + j] - f * M[k * 20 + j];
        }
    }
    return true;
}

// out[i + j] += a[i] b[j], i outermost (out: na + nb - 1 coefficients, ascending)
__device__ void em_conv(const double* a, int na, const double* b, int nb, double* out) {
    for (int o = 0; o < na + nb - 1; ++o) out[o] = 0;
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) out[i + j] += a[i] * b[j];
}

// a b - c d of polynomials into out (p, q: LDS temporaries)
__device__ void em_conv_diff(const double* a, int na, const double* b, int nb, const double* c, int nc, const double* d, int nd,
                             double* p, double* q, double* out) {
    em_conv(a, na, b, nb, p);
    em_conv(c, nc, d, nd, q);
    for (int o = 0; o < na + nb - 1; ++o) out[o] = p[o] - q[o];
}

// the 3 x 3 matrix of polynomials in z from the eliminated rows (x^2z, x^2), (y^2z, y^2), (xyz, xy), and its determinant
__device__ void em_z_polynomials(EMSolve& S) {
    for (int r = 0; r < 3; ++r) {
        const double* e = S.M + (4 + 2 * r) * 20 + 10;
        const double* f = S.M + (5 + 2 * r) * 20 + 10;
        double* row = S.B + r * 13;
        for (int h = 0; h < 2; ++h) {
            const int o = 3 * h;
            row[4 * h + 0] = e[o + 2];
            row[4 * h + 1] = e[o + 1] - f[o + 2];
            row[4 * h + 2] = e[o] - f[o + 1];
            row[4 * h + 3] = -f[o];
        }
        row[8] = e[9]; row[9] = e[8] - f[9]; row[10] = e[7] - f[8]; row[11] = e[6] - f[7]; row[12] = -f[6];
    }
    const double *kx = S.B, *ky = S.B + 4, *k1 = S.B + 8, *lx = S.B + 13, *ly = S.B + 17, *l1 = S.B + 21;
    const double *mx = S.B + 26, *my = S.B + 30, *m1 = S.B + 34;
    double *cx = S.cof, *cy = S.cof + 8, *c1 = S.cof + 16;
    em_conv_diff(ky, 4, l1, 5, k1, 5, ly, 4, S.pq, S.pq + 8, cx);
    em_conv_diff(k1, 5, lx, 4, kx, 4, l1, 5, S.pq, S.pq + 8, cy);
    em_conv_diff(kx, 4, ly, 4, ky, 4, lx, 4, S.pq, S.pq + 8, c1);
    em_conv(mx, 4, cx, 8, S.tmp);
    em_conv(my, 4, cy, 8, S.tmp + 11);
    em_conv(m1, 5, c1, 7, S.tmp + 22);
    for (int o = 0; o < 11; ++o) S.det[o] = (S.tmp[o] + S.tmp[11 + o]) + S.tmp[22 + o];
}

// Durand-Kerner on det / det[10], all ten slots updated at once; false when the polynomial or an iterate is not finite
__device__ bool em_roots(EMSolve& S) {
    const double lead = S.det[10];
    bool finite = lead != 0;
    for (int o = 0; o < 11; ++o) finite = finite && fabs(S.det[o]) <= DBL_MAX;
    if (!finite) return false;
    for (int o = 0; o < 10; ++o) S.a[o] = S.det[o] / lead;
    double pr = 1, pi = 0;
    for (int k = 0; k < 10; ++k) {
        S.zr[k] = pr; S.zi[k] = pi;
        const double nr = pr - pi, ni = pr + pi;
        pr = nr; pi = ni;
    }
    for (int it = 0; it < EM_POLY_ITERS; ++it) {
        bool done = true;
        for (int i = 0; i < 10; ++i) {
            const double zr = S.zr[i], zi = S.zi[i];
            double vr = zr + S.a[9], vi = zi;
            for (int k = 8; k >= 0; --k) {
                const double tr = (vr * zr - vi * zi) + S.a[k], ti = vr * zi + vi * zr;
                vr = tr; vi = ti;
            }
            double dr = 1, di = 0;
            for (int j = 0; j < 10; ++j) {
                if (j == i) continue;
                const double fr = zr - S.zr[j], fi = zi - S.zi[j];
                const double tr = dr * fr - di * fi, ti = dr * fi + di * fr;
                dr = tr; di = ti;
            }
            const double den = dr * dr + di * di;
            const double qr = (vr * dr + vi * di) / den, qi = (vi * dr - vr * di) / den;
            const double nzr = zr - qr, nzi = zi - qi;
            S.nr[i] = nzr; S.ni[i] = nzi;
            finite = finite && fabs(nzr) <= DBL_MAX && fabs(nzi) <= DBL_MAX;
            done = done && (fabs(qr) + fabs(qi)) <= EM_POLY_TOL * ((1.0 + fabs(nzr)) + fabs(nzi));
        }
        if (!finite) return false;
        for (int i = 0; i < 10; ++i) { S.zr[i] = S.nr[i]; S.zi[i] = S.ni[i]; }
        if (done) break;
    }
    return true;
}

__device__ __forceinline__ double em_horner(const double* p, int np, double z) {
    double v = p[np - 1];
    for (int k = np - 2; k >= 0; --k) v = v * z + p[k];
    return v;
}

__device__ __forceinline__ void em_cross_best(const double (&u)[3], const double (&w)[3], double (&best)[3], double& bn) {
    const double v0 = u[1] * w[2] - u[2] * w[1], v1 = u[2] * w[0] - u[0] * w[2], v2 = u[0] * w[1] - u[1] * w[0];
    const double nn = (v0 * v0 + v1 * v1) + v2 * v2;
    if (nn > bn) { best[0] = v0; best[1] = v1; best[2] = v2; bn = nn; }
}

// runKernel on the five normalised matches idx[0..5) by one lane: up to ten unit-norm models into `models`; returns how many
__device__ int em_solve5(const EMArgs& a, const int* idx, EMSolve& S, double* models) {
    for (int i = 0; i < EM_MP; ++i) {
        const double* x = a.xn + (size_t)idx[i] * 4;
        const double x1 = x[0], y1 = x[1], x2 = x[2], y2 = x[3];
        double* r = S.V + i * 9;
        r[0] = x2 * x1; r[1] = x2 * y1; r[2] = x2; r[3] = y2 * x1; r[4] = y2 * y1; r[5] = y2; r[6] = x1; r[7] = y1; r[8] = 1.0;
    }
    em_null_space(S.V);
    em_coeff_matrix(S);
    if (!em_eliminate(S.M)) return 0;
    em_z_polynomials(S);
    if (!em_roots(S)) return 0;
    int nm = 0;
    for (int k = 0; k < 10; ++k) {
        if (!(fabs(S.zi[k]) < 1e-10)) continue;
        const double z = S.zr[k];
        double B0[3], B1[3], B2[3];
        B0[0] = em_horner(S.B, 4, z);      B0[1] = em_horner(S.B + 4, 4, z);  B0[2] = em_horner(S.B + 8, 5, z);
        B1[0] = em_horner(S.B + 13, 4, z); B1[1] = em_horner(S.B + 17, 4, z); B1[2] = em_horner(S.B + 21, 5, z);
        B2[0] = em_horner(S.B + 26, 4, z); B2[1] = em_horner(S.B + 30, 4, z); B2[2] = em_horner(S.B + 34, 5, z);
        double v[3] = {0, 0, 0}, bn = -1.0;
        em_cross_best(B0, B1, v, bn);
        em_cross_best(B0, B2, v, bn);
        em_cross_best(B1, B2, v, bn);
        if (!(bn > 0) || !(bn <= DBL_MAX)) continue;
        const double nv = sqrt(bn);
        const double v0 = v[0] / nv, v1 = v[1] / nv, v2 = v[2] / nv;
        if (fabs(v2) < 1e-10) continue;
        const double x = v0 / v2, y = v1 / v2;
        double* E = models + nm * 9;
        double nn = 0;
        for (int o = 0; o < 9; ++o) {
            const double e = ((x * S.V[45 + o] + y * S.V[54 + o]) + z * S.V[63 + o]) + S.V[72 + o];
            E[o] = e;
            nn += e * e;
        }
        const double nrm = sqrt(nn);
        bool finite = true;
        for (int o = 0; o < 9; ++o) {
            E[o] = E[o] / nrm;
            finite = finite && fabs(E[o]) <= DBL_MAX;
        }
        if (finite) ++nm;
    }
    return nm;
}

// EMEstimatorCallback::computeError of one match: the Sampson distance in double, stored as float
__device__ __forceinline__ float em_error(const double* e, double x1, double y1, double x2, double y2) {
    const double Ex0 = (e[0] * x1 + e[1] * y1) + e[2];
    const double Ex1 = (e[3] * x1 + e[4] * y1) + e[5];
    const double Ex2 = (e[6] * x1 + e[7] * y1) + e[8];
    const double Et0 = (e[0] * x2 + e[3] * y2) + e[6];
    const double Et1 = (e[1] * x2 + e[4] * y2) + e[7];
    const double num = (x2 * Ex0 + y2 * Ex1) + Ex2;
    const double den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1;
    return (float)(num * num / den);
}

// ---- 0. the normalised points -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void em_normalize_kernel(EMArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double* x = a.xn + (size_t)i * 4;
    x[0] = ((double)a.p1[2 * i] - a.cx) / a.fx;
    x[1] = ((double)a.p1[2 * i + 1] - a.cy) / a.fy;
    x[2] = ((double)a.p2[2 * i] - a.cx) / a.fx;
    x[3] = ((double)a.p2[2 * i + 1] - a.cy) / a.fy;
}

// ---- 2 + 3. solve sample h and score all of its models against every match (workgroup / sample) --------------------
__global__ __launch_bounds__(EM_T) void em_models_score_kernel(EMArgs a) {
    __shared__ EMSolve S;
    __shared__ double sE[EM_MAXM * 9], part[(EM_T / 64) * EM_MAXM], sums[EM_MAXM];
    __shared__ int s_nm;
    const int h = a.h0 + blockIdx.x;
    const EMCtrl* c = a.ctrl;
    if (h >= a.h1 || h >= c->n_subsets || a.h0 != c->niters) return;     // (beyond the samples drawn / the loop ended before this chunk)
    if (threadIdx.x == 0) {
        int idx[EM_MP];
#pragma unroll
        for (int i = 0; i < EM_MP; ++i) idx[i] = a.subsets[h * EM_MP + i];
        const int nm = em_solve5(a, idx, S, sE);
        for (int i = 0; i < nm * 9; ++i) a.models[(size_t)h * (EM_MAXM * 9) + i] = sE[i];
        a.nmodels[h] = nm;
        s_nm = nm;
    }
    __syncthreads();
    const int nm = s_nm;
    if (!nm || a.direct) {                                              // (uniform; the five-match path does not score)
        if (threadIdx.x < EM_MAXM) a.counts[h * EM_MAXM + threadIdx.x] = 0;
        return;
    }
    double good[EM_MAXM];
#pragma unroll
    for (int m = 0; m < EM_MAXM; ++m) good[m] = 0;
    for (int i = threadIdx.x; i < a.n; i += EM_T) {
        const double* x = a.xn + (size_t)i * 4;
        const double x1 = x[0], y1 = x[1], x2 = x[2], y2 = x[3];
#pragma unroll
        for (int m = 0; m < EM_MAXM; ++m)
            if (m < nm) good[m] += em_error(sE + m * 9, x1, y1, x2, y2) <= a.t ? 1.0 : 0.0;
    }
    sslam::block_sum_n<EM_T, EM_MAXM>(good, part, sums);                 // (counts: exact in double)
    if (threadIdx.x < EM_MAXM) a.counts[h * EM_MAXM + threadIdx.x] = (int)sums[threadIdx.x];
}

// ---- 4. replay the sequential best / budget logic over samples [h0, h1) (one lane) ---------------------------------
__device__ void em_select_step(const EMArgs& a, int h0, int h1) {
    EMCtrl* c = a.ctrl;
    int it = h0;
    if (it != c->niters) return;                       // the loop already ended before this chunk
    for (; it < h1 && it < c->n_subsets && it < c->budget; ++it) {
        const int nm = a.nmodels[it];
        for (int m = 0; m < nm; ++m) {
            const int good = a.counts[it * EM_MAXM + m];
            if (good > max(c->max_good, EM_MP - 1)) {
                c->max_good = good;
                c->best_h = it;
                c->best_m = m;
                c->budget = sslam::update_num_iters(a.prob, (double)(a.n - good) / a.n, EM_MP, c->budget);
            }
        }
    }
    c->niters = it;
}

// ---- first launch after the normalisation: the control block and the samples of the first chunk -------------------
__global__ __launch_bounds__(64) void em_head_kernel(EMArgs a) {
    if (threadIdx.x != 0) return;
    EMCtrl* c = a.ctrl;
    c->budget = a.max_iters;
    c->rng_state = 0xffffffffffffffffULL;
    c->n_subsets = 0; c->best_h = -1; c->best_m = 0; c->best_count = 0; c->niters = 0; c->max_good = 0; c->pad = 0;
    for (int i = 0; i < EM_MAXM * 9; ++i) c->E[i] = 0;
    if (a.direct) {
        for (int i = 0; i < EM_MP; ++i) a.subsets[i] = i;
        c->n_subsets = 1;
        return;
    }
    em_subsets_step(a, a.h0, a.h1);
}

// ---- between chunks: the replay over the chunk just scored [h0, h1), then the samples of the next [h1, h2) ----------
__global__ __launch_bounds__(64) void em_step_kernel(EMArgs a, int h2) {
    if (threadIdx.x != 0) return;
    em_select_step(a, a.h0, a.h1);
    em_subsets_step(a, a.h1, h2);
}

// ---- last launch: the replay over the last chunk, the winner's E read back, its mask and count ---------------------
__global__ __launch_bounds__(EM_TAIL_T) void em_tail_kernel(EMArgs a) {
    __shared__ double sE[9];
    __shared__ int sh[EM_TAIL_T];
    EMCtrl* c = a.ctrl;
    if (threadIdx.x == 0) {
        if (a.direct) {
            const int nm = a.nmodels[0];
            c->best_h = nm ? 0 : -1;
            c->best_m = nm;
            for (int i = 0; i < nm * 9; ++i) c->E[i] = a.models[i];
        } else {
            em_select_step(a, a.h0, a.h1);
            if (c->best_h >= 0)
                for (int i = 0; i < 9; ++i) {
                    sE[i] = a.models[(size_t)c->best_h * (EM_MAXM * 9) + c->best_m * 9 + i];
                    c->E[i] = sE[i];
                }
        }
    }
    __syncthreads();
    const bool have = c->best_h >= 0;
    int good = 0;
    for (int i = threadIdx.x; i < a.n; i += EM_TAIL_T) {
        const double* x = a.xn + (size_t)i * 4;
        const bool keep = have && (a.direct || em_error(sE, x[0], x[1], x[2], x[3]) <= a.t);
        a.mask[i] = (unsigned char)keep;
        good += keep;
    }
    good = sslam::block_sum<EM_TAIL_T>(good, sh);
    if (threadIdx.x == 0) c->best_count = good;
}

// the slab-backed pointers of EMArgs, in slab order
void em_bind(sslam::Slab& sl, EMArgs& a, size_t N, size_t H) {
    a.p1 = sl.take<float>(N * 2); a.p2 = sl.take<float>(N * 2); a.xn = sl.take<double>(N * 4);
    a.subsets = sl.take<int>(H * EM_MP); a.models = sl.take<double>(H * EM_MAXM * 9); a.nmodels = sl.take<int>(H);
    a.counts = sl.take<int>(H * EM_MAXM); a.mask = sl.take<unsigned char>(N); a.ctrl = sl.take<EMCtrl>(1);
}

}  // namespace

extern "C" int sslam_essential_ransac_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, const double* K9,
                                           double prob, double thresh, int max_iters, unsigned char* mask_out,
                                           double* E_out, int32_t* info_out) {
    const char* who = "sslam_essential_ransac_host";
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(n >= EM_MP, "%s: %d matches, an essential matrix needs at least %d", who, n, EM_MP);
    SSLAM_REQUIRE(n <= EM_MAX_N, "%s: %d matches, at most %d are supported", who, n, EM_MAX_N);
    SSLAM_REQUIRE(pts1 && pts2 && K9 && mask_out, "%s: NULL argument", who);
    // cv::findEssentialMat's defaults for bad parameters; max_iters is clamped to what the slab is laid out for
    if (!(prob > 0 && prob < 1)) prob = 0.999;
    if (!(thresh > 0)) thresh = 1.0;
    max_iters = max_iters <= 0 ? EM_DEFAULT_ITERS : std::min(max_iters, EM_MAX_ITERS);
    const bool direct = n == EM_MP;
    if (direct) max_iters = 1;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    EMArgs a{};
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { em_bind(sl, a, N, (size_t)max_iters); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p1, pts1, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.p2, pts2, N * 2));
    a.n = n; a.max_iters = max_iters; a.direct = direct; a.prob = prob;
    a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5];
    const double th = thresh / ((a.fx + a.fy) / 2);
    a.t = (float)(th * th);
    const auto bounds = sslam::ransac_chunk_bounds(max_iters, 128);     // (the schedule: geom_slab.hpp)
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    a.h0 = bounds[0]; a.h1 = bounds[1];
    hipLaunchKernelGGL(em_normalize_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(em_head_kernel, dim3(1), dim3(64), 0, s, a);
    for (int ci = 0; ci < 3; ++ci) {
        a.h0 = bounds[ci]; a.h1 = bounds[ci + 1];
        if (a.h1 > a.h0) hipLaunchKernelGGL(em_models_score_kernel, dim3(a.h1 - a.h0), dim3(EM_T), 0, s, a);
        if (ci < 2) hipLaunchKernelGGL(em_step_kernel, dim3(1), dim3(64), 0, s, a, bounds[ci + 2]);
    }
    hipLaunchKernelGGL(em_tail_kernel, dim3(1), dim3(EM_TAIL_T), 0, s, a);       // (a.h0, a.h1: the last chunk)
    SSLAM_HIP_CHECK(hipGetLastError());
    EMCtrl h{};
    SSLAM_HIP_CHECK(sslam::copy_down(s, &h, a.ctrl, 1));
    SSLAM_HIP_CHECK(sslam::copy_down(s, mask_out, a.mask, N));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (E_out) for (int i = 0; i < EM_MAXM * 9; ++i) E_out[i] = h.best_h >= 0 ? h.E[i] : 0.0;
    if (info_out) {
        info_out[0] = h.best_h >= 0 ? h.best_count : -1;      // -1: no model (cv2 returns (None, None))
        info_out[1] = direct ? 0 : h.niters;
        info_out[2] = h.best_m;
        info_out[3] = h.best_h;
    }
    return 0;
}
