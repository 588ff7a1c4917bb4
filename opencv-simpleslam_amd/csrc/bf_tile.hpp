// bf_tile.hpp - what the brute-force matcher's kernels share: the limits, the two norms, the staging of a 64 x 64 tile of
// pairs through LDS and its 4 x 4 register tile.  bf_match_kernels.hip (one nearest neighbour) and bf_knn_kernels.hip (the k
// nearest) both run bf_tile_distances, so a pair's distance is ONE arithmetic chain by construction: the bits of `match`
// and of `knnMatch` can only differ in what is kept, never in what is compared.
//
// The arithmetic is the contract (tests/bf_ref.py): NORM_HAMMING is the popcount of the XOR over all D bytes, exact;
// NORM_L2 is, per pair, one float32 accumulator, k ascending, diff = a_k - b_k, acc = fmaf(diff, diff, acc), and a
// correctly rounded root.  Plain fp32 VALU on purpose, no matrix core.
#pragma once
#include "common.hpp"

#include <cfloat>

namespace sslam {
namespace bf {

constexpr int BF_NORM_L2 = 4, BF_NORM_HAMMING = 6;      // cv2's values
constexpr int BF_MAX_ROWS = 65536;
constexpr int BF_MAX_D_HAMMING = 256, BF_MAX_D_L2 = 512;
constexpr int BF_T = 256;                // the distance workgroup: 16 x 16 threads, 4 x 4 pairs each
constexpr int BF_TILE = 64;              // rows of a tile, both sides
constexpr int BF_KC = 32;                // elements of a row per staged chunk
constexpr int BF_LD = BF_TILE + 4;       // leading dimension of a staged chunk [k][row]: rows of 272 bytes (16-byte aligned)
constexpr unsigned long long BF_NONE = ~0ull;

// the two descriptor sets of a call, as every kernel of the matcher takes them
struct BFRows {
    int D;                                    // bytes (Hamming) or floats (L2) per row
    int M, N;                                 // row bounds
    const int32_t* m_dev; const int32_t* n_dev;   // device counts, clamped to [0, bound]; may be NULL
    const void* q; const void* t;             // [M][D], [N][D]
    int words_ok;                             // Hamming: D % 4 == 0 and both bases 4-byte aligned: rows are read as words
};

__device__ __forceinline__ int bf_count(const int32_t* dev, int bound) { return dev ? min(max(dev[0], 0), bound) : bound; }

struct HammingNorm {
    using Elem = uint32_t;                    // a staged element: 4 bytes of the row, zero beyond D
    static __device__ __forceinline__ int elems(int D) { return (D + 3) >> 2; }
    static __device__ __forceinline__ Elem load(const BFRows& a, const void* base, int row, int k) {
        if (a.words_ok) return reinterpret_cast<const uint32_t*>(base)[(size_t)row * (a.D >> 2) + k];
        const uint8_t* p = reinterpret_cast<const uint8_t*>(base) + (size_t)row * a.D;
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4 * k + b < a.D) w |= (uint32_t)p[4 * k + b] << (8 * b);
        return w;
    }
    static __device__ __forceinline__ void step(Elem& acc, Elem x, Elem y) { acc += __popc(x ^ y); }
    static __device__ __forceinline__ float finish(Elem acc) { return (float)acc; }
};

struct L2Norm {
    using Elem = float;
    static __device__ __forceinline__ int elems(int D) { return D; }
    static __device__ __forceinline__ Elem load(const BFRows& a, const void* base, int row, int k) {
        return reinterpret_cast<const float*>(base)[(size_t)row * a.D + k];
    }
    static __device__ __forceinline__ void step(Elem& acc, Elem x, Elem y) {
        const float diff = x - y;
        acc = __builtin_fmaf(diff, diff, acc);
    }
    static __device__ __forceinline__ float finish(Elem acc) { return __fsqrt_rn(acc); }
};

template <class E>
struct alignas(16) BFVec4 { E v[4]; };

constexpr int BF_STAGE_VEC4 = BF_KC * BF_LD / 4;        // BFVec4 elements of one side's staged chunk

__device__ __forceinline__ unsigned long long bf_min(unsigned long long x, unsigned long long y) { return x < y ? x : y; }
__device__ __forceinline__ unsigned long long bf_max(unsigned long long x, unsigned long long y) { return x < y ? y : x; }

// the key of a pair: distances are non-negative, so bit order is value order, and the lower index wins a tie
__device__ __forceinline__ unsigned long long bf_key(float d, int other) {
    return (unsigned long long)__float_as_uint(d) << 32 | (unsigned)other;
}

// The accumulators of the 64 x 64 tile of pairs at (q0, t0), every thread of the workgroup of BF_T: thread (ty, tx) =
// (tid >> 4, tid & 15) leaves in acc[i][j] the un-finished sum of query row q0 + 4 ty + i and train row t0 + 4 tx + j.
// Both tiles are staged through sq4 / st4 (BF_STAGE_VEC4 each) in chunks of BF_KC elements, TRANSPOSED (k-major), so that a
// thread's fragment of one k is two 16-byte LDS reads, the query one a broadcast over 16 lanes.  Rows at and beyond m / n
// are staged as zeros and never read from memory; the caller leaves their pairs out.  Ends with a barrier: the staging
// buffers are free again when it returns.
template <class Norm>
__device__ __forceinline__ void bf_tile_distances(const BFRows& a, int q0, int t0, int m, int n,
                                                  BFVec4<typename Norm::Elem>* sq4, BFVec4<typename Norm::Elem>* st4,
                                                  typename Norm::Elem (&acc)[4][4]) {
    using Elem = typename Norm::Elem;
    Elem* sq = &sq4[0].v[0];
    Elem* st = &st4[0].v[0];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;

    const int E = Norm::elems(a.D);
    for (int k0 = 0; k0 < E; k0 += BF_KC) {
        const int kn = min(BF_KC, E - k0);
        // stage [kn][64] of both sides: a turn covers 8 k x 32 rows, 8 lanes along k (32 contiguous bytes of a row) and a
        // 32-lane group on 32 different banks (bank = 4 k + row).  Rows beyond the counts are zeros and are left out below.
#pragma unroll
        for (int s = 0; s < BF_TILE * BF_KC / BF_T; ++s) {
            const int k = (tid & 7) + 8 * (s & 3), r = (tid >> 3) + 32 * (s >> 2);
            if (8 * (s & 3) >= kn) continue;
            Elem x = 0, y = 0;
            if (k < kn) {
                if (q0 + r < m) x = Norm::load(a, a.q, q0 + r, k0 + k);
                if (t0 + r < n) y = Norm::load(a, a.t, t0 + r, k0 + k);
            }
            sq[k * BF_LD + r] = x;
            st[k * BF_LD + r] = y;
        }
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            const BFVec4<Elem> x = sq4[(k * BF_LD + 4 * ty) / 4], y = st4[(k * BF_LD + 4 * tx) / 4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) Norm::step(acc[i][j], x.v[i], y.v[j]);
        }
        __syncthreads();
    }
}

// every refusal of the matcher's entries that needs no device, in the order of the arguments
inline int bf_check(const char* who, sslam_ctx* ctx, int norm, int D, int M, int N) {
    SSLAM_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(norm == BF_NORM_L2 || norm == BF_NORM_HAMMING,
                  "%s: norm %d is neither NORM_L2 (4) nor NORM_HAMMING (6)", who, norm);
    const int dmax = norm == BF_NORM_HAMMING ? BF_MAX_D_HAMMING : BF_MAX_D_L2;
    SSLAM_REQUIRE(D >= 1 && D <= dmax, "%s: D %d outside 1..%d (%s)", who, D, dmax,
                  norm == BF_NORM_HAMMING ? "bytes per row, NORM_HAMMING" : "floats per row, NORM_L2");
    SSLAM_REQUIRE(M >= 0 && M <= BF_MAX_ROWS, "%s: M %d outside 0..%d", who, M, BF_MAX_ROWS);
    SSLAM_REQUIRE(N >= 0 && N <= BF_MAX_ROWS, "%s: N %d outside 0..%d", who, N, BF_MAX_ROWS);
    return 0;
}

inline size_t bf_row_bytes(int norm, int D) { return norm == BF_NORM_HAMMING ? (size_t)D : (size_t)D * sizeof(float); }

}  // namespace bf
}  // namespace sslam
