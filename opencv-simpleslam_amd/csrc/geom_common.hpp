// geom_common.hpp - device helpers shared by the geometry kernels (ransac_kernels.hip, homography_kernels.hip,
// essential_kernels.hip, pnp_kernels.hip, triangulate_kernels.hip, relative_pose_kernels.hip, ba_lm.hip).  Their host side
// - the scratch slab's layout and the RANSAC chunk bounds - is geom_slab.hpp.
//
// The RANSAC pieces restate OpenCV 4.x's classic ptsetreg.cpp; both RANSAC files must stay bit-exact with the numpy
// restatements under oracle/, so they share one copy.  Nothing here holds a contractible multiply-add: pnp_kernels.hip
// compiles with `fp contract(off)` and the other files do not, and both must see the same arithmetic.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

namespace sslam {

// cv::RNG: multiply-with-carry on a 64-bit state
struct CvRng {
    unsigned long long state;
    __device__ __forceinline__ unsigned next() {
        state = (unsigned long long)(unsigned)state * 4164903690ULL + (unsigned)(state >> 32);
        return (unsigned)state;
    }
    __device__ __forceinline__ int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};

// RANSACUpdateNumIters(p, ep, modelPoints, maxIters)
__device__ __forceinline__ int update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = fmax(p, 0.0); p = fmin(p, 1.0);
    ep = fmax(ep, 0.0); ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, DBL_MIN);
    double denom = 1.0 - pow(1.0 - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

// getSubset's draw: MP distinct indices in [0, n), a duplicate is drawn again
template <int MP>
__device__ __forceinline__ void draw_distinct(CvRng& rng, int n, int* idx) {
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        int v;
        bool dup;
        do {
            v = rng.uniform(0, n);
            dup = false;
#pragma unroll
            for (int j = 0; j < i; ++j) dup |= idx[j] == v;
        } while (dup);
        idx[i] = v;
    }
}

// haveCollinearPoints(m, count) of fundam.cpp: the LAST point of the subset against every earlier pair, on points p [.][2]
__device__ inline bool last_point_collinear(const float* p, const int* idx, int count) {
    const int i = count - 1;
    const float xi = p[2 * idx[i]], yi = p[2 * idx[i] + 1];
    for (int j = 0; j < i; ++j) {
        const double dx1 = p[2 * idx[j]] - xi, dy1 = p[2 * idx[j] + 1] - yi;
        for (int k = 0; k < j; ++k) {
            const double dx2 = p[2 * idx[k]] - xi, dy2 = p[2 * idx[k] + 1] - yi;
            if (fabs(dx2 * dy1 - dy2 * dx1) <= (double)FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2)))
                return true;
        }
    }
    return false;
}

// Fixed-order tree reduction in LDS over a power-of-two workgroup: NT threads when the launch fixes it, else blockDim.x.
// Every thread calls it and gets the result; `sh` holds one element per thread.
// `op(acc, v)` folds v into acc in place.
template <int NT = 0, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, T* sh, Op op) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = (NT ? NT : (int)blockDim.x) >> 1; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

template <int NT = 0, typename T>
__device__ __forceinline__ T block_sum(T v, T* sh) { return block_reduce<NT>(v, sh, [](T& acc, T x) { acc += x; }); }

template <int NT = 0>
__device__ __forceinline__ double block_max(double v, double* sh) {
    return block_reduce<NT>(v, sh, [](double& acc, double x) { acc = fmax(acc, x); });
}

// N sums at once over a workgroup of NT threads (a multiple of 64; every thread calls it), two barriers for all of them: a
// wave's lanes by xor-shuffles, then thread k adds sum k of the waves in wave order - a fixed order.  `part` (NT / 64 x N
// doubles) and `out` (N doubles, the result, valid for every thread on return) are LDS.
template <int NT, int N>
__device__ __forceinline__ void block_sum_n(const double (&acc)[N], double* part, double* out) {
    static_assert(N <= NT, "one thread per sum");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) part[w * N + k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        double s = 0;
        for (int j = 0; j < NT / 64; ++j) s += part[j * N + threadIdx.x];
        out[threadIdx.x] = s;
    }
    __syncthreads();
}

// One turn of an order-preserving compaction over a workgroup of NT threads (a multiple of 64; every thread calls it):
// a thread whose `keep` is set gets emit(o), o = the number of items kept before its own - in earlier turns, then by
// lower threads of this one.  `wsum` (NT / 64 ints) and `base` (the running count, 0 before the first turn) are LDS.
template <int NT, typename Emit>
__device__ __forceinline__ void block_compact(bool keep, int* wsum, int& base, Emit emit) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int o = base;
    for (int j = 0; j < w; ++j) o += wsum[j];
    o += __popcll(bal & ((1ull << lane) - 1));
    if (keep) emit(o);
    __syncthreads();
    if (threadIdx.x == NT - 1) base = o + keep;           // the last thread's rank + its own item: the new running count
    __syncthreads();
}

}  // namespace sslam
