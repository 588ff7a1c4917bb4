// dlt_svd.hpp - the per-thread DLT of `cv2.triangulatePoints` and the one-sided (Hestenes) Jacobi SVD under it, shared by
// triangulate_kernels.hip and relative_pose_kernels.hip.
//
// OpenCV 4.x's triangulate.cpp builds, per match, the 4 x 4 matrix with rows x P[2] - P[0], y P[2] - P[1] of each view and
// takes the right singular vector of its smallest singular value; its JacobiSVD rotates the COLUMNS of the matrix itself
// (never A^T A, whose condition number is the square).  Here one lane does the same: the sweep cap (30, OpenCV's), the
// rotation order (0,1) (0,2) ... (N-2,N-1) and the stopping rule (a pair is left alone when |p| <= 10 eps sqrt(a b)) are
// fixed, so a result depends on nothing but its own matrix.  The same rotations on a 3 x 3 matrix give the full SVD that
// `decomposeEssentialMat` needs: the stopping rule is RELATIVE, so the column of a vanishing singular value still ends up
// orthogonal to the others and its direction is a left singular vector.
//
// The multiply-adds here are contractible: each including file's own `fp contract` setting decides whether they fuse
// (triangulate_kernels.hip leaves the compiler's default, relative_pose_kernels.hip turns fusing off).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace sslam {

constexpr int JACOBI_SWEEPS = 30;        // OpenCV's JacobiSVD iteration cap for these sizes

// One Jacobi rotation of columns I, J of A (stored column-major: A[col][row]) and of V; false when they are already orthogonal.
template <int I, int J, int N>
__device__ __forceinline__ bool jacobi_rotate(double (&A)[N][N], double (&V)[N][N]) {
    double a = 0, b = 0, p = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) { a += A[I][k] * A[I][k]; b += A[J][k] * A[J][k]; p += A[I][k] * A[J][k]; }
    if (fabs(p) <= (DBL_EPSILON * 10) * sqrt(a * b)) return false;
    p *= 2;
    const double beta = a - b, gamma = hypot(p, beta);
    double c, s;
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = sqrt(delta / gamma);
        c = p / (gamma * s * 2);
    } else {
        c = sqrt((gamma + beta) / (gamma * 2));
        s = p / (gamma * c * 2);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double t0 = c * A[I][k] + s * A[J][k], t1 = c * A[J][k] - s * A[I][k];
        A[I][k] = t0; A[J][k] = t1;
        const double v0 = c * V[I][k] + s * V[J][k], v1 = c * V[J][k] - s * V[I][k];
        V[I][k] = v0; V[J][k] = v1;
    }
    return true;
}

// V = I, then sweeps until one changes nothing: the columns of A become U S, those of V the right singular vectors
__device__ __forceinline__ void jacobi_sweeps(double (&A)[4][4], double (&V)[4][4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) V[k][r] = k == r ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        bool changed = jacobi_rotate<0, 1>(A, V);
        changed |= jacobi_rotate<0, 2>(A, V);
        changed |= jacobi_rotate<0, 3>(A, V);
        changed |= jacobi_rotate<1, 2>(A, V);
        changed |= jacobi_rotate<1, 3>(A, V);
        changed |= jacobi_rotate<2, 3>(A, V);
        if (!changed) break;
    }
}

__device__ __forceinline__ void jacobi_sweeps(double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) V[k][r] = k == r ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        bool changed = jacobi_rotate<0, 1>(A, V);
        changed |= jacobi_rotate<0, 2>(A, V);
        changed |= jacobi_rotate<1, 2>(A, V);
        if (!changed) break;
    }
}

// cv2.triangulatePoints for one match: P1, P2 row-major 3 x 4, (u1, v1) / (u2, v2) the match in the two views; X4 = the
// homogeneous point (unit norm, sign arbitrary) - the column of V under the column of A of smallest norm, the first of equals
__device__ __forceinline__ void dlt_null_vector(const double* P1, const double* P2, double u1, double v1, double u2, double v2,
                                                double* X4) {
    double A[4][4], V[4][4];                       // [column][row]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        A[k][0] = u1 * P1[8 + k] - P1[k];
        A[k][1] = v1 * P1[8 + k] - P1[4 + k];
        A[k][2] = u2 * P2[8 + k] - P2[k];
        A[k][3] = v2 * P2[8 + k] - P2[4 + k];
    }
    jacobi_sweeps(A, V);
    double best = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = A[k][0] * A[k][0] + A[k][1] * A[k][1] + A[k][2] * A[k][2] + A[k][3] * A[k][3];
        if (k == 0 || s < best) {
            best = s;
#pragma unroll
            for (int r = 0; r < 4; ++r) X4[r] = V[k][r];
        }
    }
}

}  // namespace sslam
