// feat_device.hpp - the device helpers that orb_kernels.hip, sift_kernels.hip, akaze_kernels.hip and klt_kernels.hip share, written
// ONCE: the outputs of SIFT and AKAZE are defined bit for bit and ORB's keypoints against the restatements under tests/, so a
// fix to one of these must reach every detector.  All are __forceinline__: a kernel compiled under
// __attribute__((target("no-packed-fp32-ops"))) inlines them and compiles them under its own attribute.  An expression here is
// one IEEE operation at a time: the pragma below turns contraction off from here to the end of the translation unit, whatever
// the order of the includes (every including file says the same before its own kernels).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "feat_plan.hpp"

#pragma clang fp contract(off)

namespace sslam {

// BORDER_REFLECT_101 of any i into 0 .. n - 1 (as many folds as it takes)
__device__ __forceinline__ int reflect101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// the grey value of a pixel of C channels: the first (C == 1) or BGR2GRAY in 15 fractional bits (an alpha channel is ignored)
__device__ __forceinline__ int bgr_to_grey(const uint8_t* __restrict__ s, int C) {
    return C == 1 ? (int)s[0] : ((int)s[0] * 3735 + (int)s[1] * 19235 + (int)s[2] * 9798 + (1 << 14)) >> 15;
}

// the sum over the wavefront's 64 lanes, on every lane (integers: exact, the order does not matter)
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// cv::fastAtan2 in degrees, 0 .. 360: float32, one operation at a time
__device__ __forceinline__ float fast_atan2_deg(const FastAtan& k, float fy, float fx) {
    const float ax = fabsf(fx), ay = fabsf(fy);
    float ang;
    if (ax >= ay) {
        const float q = ay / (ax + k.eps), q2 = q * q;
        float t = k.p7 * q2; t = t + k.p5; t = t * q2; t = t + k.p3; t = t * q2; t = t + k.p1;
        ang = t * q;
    } else {
        const float q = ax / (ay + k.eps), q2 = q * q;
        float t = k.p7 * q2; t = t + k.p5; t = t * q2; t = t + k.p3; t = t * q2; t = t + k.p1;
        t = t * q;
        ang = 90.f - t;
    }
    if (fx < 0.f) ang = 180.f - ang;
    if (fy < 0.f) ang = 360.f - ang;
    return ang;
}

// a float32 as a 64-bit integer at scale 2^LOG2 (truncated; `Int` unsigned: v >= 0) and back: the order-free sums of the histograms
template <int LOG2, class Int = long long>
__device__ __forceinline__ Int to_fixed(float v) { return (Int)((double)v * (double)(1ull << LOG2)); }
template <int LOG2>
__device__ __forceinline__ float from_fixed(long long s) { return (float)((double)s / (double)(1ull << LOG2)); }

// a frame whose candidates or keypoints exceed their list is voided (count 0, the sticky word), never truncated.  `a`: the
// kernel arguments of a detector with such lists - the capacities cand_cap, kp_cap and `ctl`, the control block in device memory
// with the counters ncand, nkp.  (It takes the arguments, not the four numbers: the keypoint counter is then read only when the
// candidates fit, and the kernels' code stays what it was.)
template <class Args>
__device__ __forceinline__ bool feat_voided(const Args& a) { return a.ctl->ncand > a.cand_cap || a.ctl->nkp > a.kp_cap; }

}  // namespace sslam
