// bf_knn_kernels.hip - the k nearest train rows of every query row: `cv2.BFMatcher(norm).knnMatch(des0, des1, k)`, k = 1..8,
// and Lowe's ratio test on the two nearest as a device stage that feeds the F-matrix filter.
//
// Semantics (tests/bf_knn_ref.py restates them and lists what could not be confirmed against a real cv2):
//   * the distance of a pair is that of `match`, bit for bit: the norms, the staging and the 4 x 4 register tile are
//     bf_tile.hpp's, shared with bf_match_kernels.hip; a pair is valid iff d < FLT_MAX (a NaN never is);
//   * the neighbours of query row i are its valid train rows in ascending order of the key (float32 d, train index) - for L2
//     the float AFTER the root, the lower index first on a tie -, the first min(k, number of valid rows) of them.  The order is
//     total, so the result does not depend on how the work is split;
//   * idx [M][k] int32 is padded with -1, dist [M][k] float32 with +inf, cnt [M] int32 is the number of neighbours;
//   * the ratio test keeps row i iff cnt[i] >= 2 and (double)d1 < ratio * (double)d2, ONE fp64 multiply - Python's
//     `m.distance < ratio * n.distance` on DMatch floats -, and gives (i, idx1, d1) in query order.
//
// Two launches (three for the ratio form), no memset, no atomics:
//   1. bf_knn_partial_kernel<Norm, K>, grid (S, ceil(M / 64)), a workgroup of 256 per row tile and column split (the host
//      plan, bf_knn_plan.hpp, chooses K = 2 / 4 / 8 and S).  The workgroup walks the train tiles of its split; a thread keeps,
//      for each of its 4 query rows, the K smallest keys (float bits of d) << 32 | train index it has seen, ascending, in
//      registers: an insertion is an unrolled compare-exchange chain (compile-time indices only, no per-thread array that is
//      indexed at run time), skipped when the key is not below the list's last.  After the last tile the 16 adjacent lanes that
//      share a row merge their lists in 4 butterfly steps: the partner's list arrives by shuffles, min(own[c], partner[K-1-c])
//      are the K smallest of the 2 K as a bitonic sequence, and log2 K compare-exchange stages sort it.  The row's K keys go
//      through LDS to scratch [S][K][M], so that adjacent rows are adjacent lanes of one store.  Rows at and beyond the device
//      count m are neither computed nor written; a split beyond the device count n writes empty lists.
//   2. bf_knn_finish_kernel<K>, a thread per query row: merges the row's S lists (coalesced reads) by the same insertion and
//      writes idx / dist / cnt for rows < m and info = {m, n, k, S};  or, the ratio form, bf_ratio_reduce_kernel - the same merge
//      at K = 2, a thread per row, folded into split 0's lists in place (skipped when S is 1) - and bf_ratio_finish_kernel, one
//      workgroup of 1 024: the ratio test on the row's two keys and the compaction in query order (sslam::block_compact) into
//      the layout sslam_bf_match_dev leaves - ij [M][2], dist [M], info {K, m, n, 0} - which sslam_fmat_ransac_dev reads as it
//      is.  (One workgroup reading 2 S keys per row one after the other was measured at 24 - 43 us; two keys are one round.)
// A minimum over a total order does not depend on the order of arrival: the outputs are bitwise the same from run to run and
// for every S.  Scratch: 8 S M K bytes of the context's slab.
#include "bf_knn_plan.hpp"
#include "bf_tile.hpp"
#include "geom_common.hpp"

#include <cmath>

namespace {

using namespace sslam::bf;

static_assert(sslam::BFK_TILE == BF_TILE, "the plan and the kernels tile the train rows alike");

constexpr int BFK_FIN_T = 256;           // the k-NN finish: a thread per query row
constexpr int BFK_RATIO_T = 1024;        // the ratio finish: one workgroup, compaction turns of 1 024 rows

struct BFKArgs : BFRows {
    int k, K, S, tiles;                       // the plan: neighbours asked for, list length, column splits, ceil(N / 64)
    double ratio;
    unsigned long long* lists;                // [S][K][M] keys, ascending along K; ~0 = none
    int32_t* idx_out; float* dist_out; int32_t* cnt_out; int32_t* info_out;   // k-NN form: [M][k], [M][k], [M], [4]
    int32_t* ij_out;                          // ratio form: [M][2] (with dist_out [M] and info_out)
};

// x into the ascending list L; the largest of the K + 1 falls out
template <int K>
__device__ __forceinline__ void bfk_insert(unsigned long long (&L)[K], unsigned long long x) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const unsigned long long lo = bf_min(L[c], x);
        x = bf_max(L[c], x);
        L[c] = lo;
    }
}

// L, P ascending -> L = the K smallest of both, ascending (a bitonic merge: the half-cleaner, then log2 K stages)
template <int K>
__device__ __forceinline__ void bfk_merge(unsigned long long (&L)[K], const unsigned long long (&P)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) L[c] = bf_min(L[c], P[K - 1 - c]);
#pragma unroll
    for (int s = K / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int c = 0; c < K; ++c)
            if ((c & s) == 0) {
                const unsigned long long lo = bf_min(L[c], L[c + s]), hi = bf_max(L[c], L[c + s]);
                L[c] = lo;
                L[c + s] = hi;
            }
}

// ---- 1. a row tile and a column split per workgroup: the K smallest keys of every row over the split's train tiles ----------
template <class Norm, int K>
__global__ __launch_bounds__(BF_T) void bf_knn_partial_kernel(BFKArgs a) {
    using Elem = typename Norm::Elem;
    __shared__ BFVec4<Elem> sq4[BF_STAGE_VEC4], st4[BF_STAGE_VEC4];
    __shared__ unsigned long long s_out[K][BF_TILE];
    const int m = bf_count(a.m_dev, a.M), n = bf_count(a.n_dev, a.N);
    const int q0 = blockIdx.y * BF_TILE, split = blockIdx.x;
    if (q0 >= m) return;                     // (the whole workgroup: the counts are uniform)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int tile0 = (int)((long long)split * a.tiles / a.S), tile1 = (int)((long long)(split + 1) * a.tiles / a.S);

    unsigned long long L[4][K];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < K; ++c) L[i][c] = BF_NONE;

    for (int tile = tile0; tile < tile1; ++tile) {
        const int t0 = tile * BF_TILE;
        if (t0 >= n) break;                  // (uniform; this split's lists stay empty from here)
        Elem acc[4][4];
        bf_tile_distances<Norm>(a, q0, t0, m, n, sq4, st4, acc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = Norm::finish(acc[i][j]);
                const int qi = q0 + 4 * ty + i, tj = t0 + 4 * tx + j;
                if (qi < m && tj < n && d < FLT_MAX) {                      // (NaN fails the comparison)
                    const unsigned long long key = bf_key(d, tj);
                    if (key < L[i][K - 1]) bfk_insert<K>(L[i], key);
                }
            }
    }
    // a row's 16 threads are 16 adjacent lanes: after the 4 steps every one of them holds the row's list
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            unsigned long long P[K];
#pragma unroll
            for (int c = 0; c < K; ++c) P[c] = __shfl_xor(L[i][c], o);
            bfk_merge<K>(L[i], P);
        }
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < K; ++c) s_out[c][4 * ty + i] = L[i][c];
    }
    __syncthreads();
    for (int e = tid; e < K * BF_TILE; e += BF_T) {
        const int c = e / BF_TILE, r = e % BF_TILE;
        if (q0 + r < m) a.lists[((size_t)split * K + c) * (size_t)a.M + (size_t)(q0 + r)] = s_out[c][r];
    }
}

// the K smallest keys of a row over its S lists
template <int K>
__device__ __forceinline__ void bfk_row_list(const BFKArgs& a, int row, unsigned long long (&R)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) R[c] = BF_NONE;
    for (int s = 0; s < a.S; ++s) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const unsigned long long x = a.lists[((size_t)s * K + c) * (size_t)a.M + (size_t)row];
            if (x < R[K - 1]) bfk_insert<K>(R, x);
        }
    }
}

// ---- 2a. the k-NN form: a thread per query row --------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(BFK_FIN_T) void bf_knn_finish_kernel(BFKArgs a) {
    const int m = bf_count(a.m_dev, a.M), n = bf_count(a.n_dev, a.N);
    const int row = blockIdx.x * BFK_FIN_T + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4)
        a.info_out[threadIdx.x] = threadIdx.x == 0 ? m : threadIdx.x == 1 ? n : threadIdx.x == 2 ? a.k : a.S;
    if (row >= m) return;
    unsigned long long R[K];
    bfk_row_list<K>(a, row, R);
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < K; ++c)
        if (c < a.k) {
            const bool valid = R[c] != BF_NONE;
            cnt += valid;
            a.idx_out[(size_t)row * a.k + c] = valid ? (int32_t)(uint32_t)R[c] : -1;
            a.dist_out[(size_t)row * a.k + c] = valid ? __uint_as_float((uint32_t)(R[c] >> 32)) : INFINITY;
        }
    a.cnt_out[row] = cnt;
}

// ---- 2b. the ratio form: a thread per query row folds the row's S lists into split 0's, in place (only this thread reads or
// writes the row's entries), so that the one workgroup below reads two keys per row instead of 2 S one after the other ----------
__global__ __launch_bounds__(BFK_FIN_T) void bf_ratio_reduce_kernel(BFKArgs a) {
    const int m = bf_count(a.m_dev, a.M);
    const int row = blockIdx.x * BFK_FIN_T + threadIdx.x;
    if (row >= m) return;
    unsigned long long R[2];
    bfk_row_list<2>(a, row, R);
    a.lists[(size_t)row] = R[0];
    a.lists[(size_t)a.M + (size_t)row] = R[1];
}

// ---- 2c. the test on the two nearest, the kept rows in query order (one workgroup) ------------------------------------------
__global__ __launch_bounds__(BFK_RATIO_T) void bf_ratio_finish_kernel(BFKArgs a) {
    __shared__ int wsum[BFK_RATIO_T / 64], base;
    const int m = bf_count(a.m_dev, a.M), n = bf_count(a.n_dev, a.N);
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += BFK_RATIO_T) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        int j = 0;
        float d = 0.f;
        if (i < m && a.S > 0) {                                             // (S == 0: no train row, no list)
            const unsigned long long r0 = a.lists[(size_t)i], r1 = a.lists[(size_t)a.M + (size_t)i];       // split 0: the row's two nearest
            if (r1 != BF_NONE) {                                            // two neighbours
                d = __uint_as_float((uint32_t)(r0 >> 32));
                const double d2 = (double)__uint_as_float((uint32_t)(r1 >> 32));
                j = (int)(uint32_t)r0;
                keep = (double)d < a.ratio * d2;                            // one fp64 multiply
            }
        }
        sslam::block_compact<BFK_RATIO_T>(keep, wsum, base, [&](int o) {
            a.ij_out[2 * o] = i; a.ij_out[2 * o + 1] = j;
            a.dist_out[o] = d;
        });
    }
    if (threadIdx.x < 4) a.info_out[threadIdx.x] = threadIdx.x == 0 ? base : threadIdx.x == 1 ? m : threadIdx.x == 2 ? n : 0;
}

template <class Norm>
void bfk_launch_partial(hipStream_t s, const BFKArgs& a) {
    const dim3 grid(a.S, sslam::cdiv(a.M, BF_TILE));
    if (a.K == 2) hipLaunchKernelGGL((bf_knn_partial_kernel<Norm, 2>), grid, dim3(BF_T), 0, s, a);
    else if (a.K == 4) hipLaunchKernelGGL((bf_knn_partial_kernel<Norm, 4>), grid, dim3(BF_T), 0, s, a);
    else hipLaunchKernelGGL((bf_knn_partial_kernel<Norm, 8>), grid, dim3(BF_T), 0, s, a);
}

int bfk_enqueue(hipStream_t s, const BFKArgs& a, int norm, bool ratio) {
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (a.M > 0 && a.S > 0) {
        if (norm == BF_NORM_HAMMING) bfk_launch_partial<HammingNorm>(s, a);
        else bfk_launch_partial<L2Norm>(s, a);
    }
    if (ratio) {
        if (a.M > 0 && a.S > 1) hipLaunchKernelGGL(bf_ratio_reduce_kernel, dim3(sslam::cdiv(a.M, BFK_FIN_T)), dim3(BFK_FIN_T), 0, s, a);
        hipLaunchKernelGGL(bf_ratio_finish_kernel, dim3(1), dim3(BFK_RATIO_T), 0, s, a);
    } else {
        const dim3 grid(sslam::cdiv(a.M > 0 ? a.M : 1, BFK_FIN_T));
        if (a.K == 2) hipLaunchKernelGGL(bf_knn_finish_kernel<2>, grid, dim3(BFK_FIN_T), 0, s, a);
        else if (a.K == 4) hipLaunchKernelGGL(bf_knn_finish_kernel<4>, grid, dim3(BFK_FIN_T), 0, s, a);
        else hipLaunchKernelGGL(bf_knn_finish_kernel<8>, grid, dim3(BFK_FIN_T), 0, s, a);
    }
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

// every refusal that needs no device, in the order of the arguments; then the plan
int bfk_check(const char* who, sslam_ctx* ctx, int norm, int D, int M, int N, int k, int splits, sslam::BfKnnPlan* plan) {
    if (int rc = bf_check(who, ctx, norm, D, M, N)) return rc;
    char msg[200];
    if (int rc = sslam::bfk_check_k(who, k, msg, sizeof msg)) { sslam::set_error("%s", msg); return rc; }
    if (int rc = sslam::bfk_check_splits(who, splits, N, msg, sizeof msg)) { sslam::set_error("%s", msg); return rc; }
    *plan = sslam::bfk_plan(M, N, k, splits);
    return 0;
}

int bfk_check_ratio(const char* who, double ratio) {
    SSLAM_REQUIRE(std::isfinite(ratio) && ratio > 0.0, "%s: ratio %g is not finite and > 0", who, ratio);
    return 0;
}

void bfk_fill(BFKArgs& a, const sslam::BfKnnPlan& p, int D, int M, int N) {
    a.D = D; a.M = M; a.N = N;
    a.k = p.k; a.K = p.K; a.S = p.S; a.tiles = p.tiles;
}

// the slab-backed pointers of BFKArgs, in slab order.  host: the inputs and outputs are the slab's too
void bfk_bind(sslam::Slab& sl, BFKArgs& a, const sslam::BfKnnPlan& p, size_t row_bytes, bool host, bool ratio) {
    const size_t M = (size_t)a.M, N = (size_t)a.N;
    a.lists = sl.take<unsigned long long>(p.scratch_bytes / sizeof(unsigned long long));
    if (!host) return;
    a.q = sl.take<uint8_t>(M * row_bytes); a.t = sl.take<uint8_t>(N * row_bytes);
    a.info_out = sl.take<int32_t>(4);
    if (ratio) { a.ij_out = sl.take<int32_t>(M * 2); a.dist_out = sl.take<float>(M); }
    else { a.idx_out = sl.take<int32_t>(M * p.k); a.dist_out = sl.take<float>(M * p.k); a.cnt_out = sl.take<int32_t>(M); }
}

}  // namespace

extern "C" int sslam_bf_knn_match_dev(sslam_ctx* ctx, int norm, int D, const void* q_dev, int M, const int32_t* m_dev,
                                      const void* t_dev, int N, const int32_t* n_dev, int k, int splits,
                                      int32_t* idx_out_dev, float* dist_out_dev, int32_t* cnt_out_dev, int32_t* info_out_dev) {
    const char* who = "sslam_bf_knn_match_dev";
    sslam::BfKnnPlan p;
    if (int rc = bfk_check(who, ctx, norm, D, M, N, k, splits, &p)) return rc;
    SSLAM_REQUIRE(info_out_dev != nullptr, "%s: info_out_dev is NULL", who);
    SSLAM_REQUIRE(M == 0 || (q_dev && idx_out_dev && dist_out_dev && cnt_out_dev),
                  "%s: q_dev / idx_out_dev / dist_out_dev / cnt_out_dev is NULL", who);
    SSLAM_REQUIRE(N == 0 || t_dev, "%s: t_dev is NULL", who);
    BFKArgs a{};
    bfk_fill(a, p, D, M, N);
    a.m_dev = m_dev; a.n_dev = n_dev; a.q = q_dev; a.t = t_dev;
    a.words_ok = D % 4 == 0 && ((uintptr_t)q_dev | (uintptr_t)t_dev) % 4 == 0;
    a.idx_out = idx_out_dev; a.dist_out = dist_out_dev; a.cnt_out = cnt_out_dev; a.info_out = info_out_dev;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bfk_bind(sl, a, p, bf_row_bytes(norm, D), false, false); })) return rc;
    return bfk_enqueue(ctx->stream, a, norm, false);
}

extern "C" int sslam_bf_knn_match_host(sslam_ctx* ctx, int norm, int D, const void* q, int M, const void* t, int N, int k,
                                       int splits, int32_t* idx_out, float* dist_out, int32_t* cnt_out) {
    const char* who = "sslam_bf_knn_match_host";
    sslam::BfKnnPlan p;
    if (int rc = bfk_check(who, ctx, norm, D, M, N, k, splits, &p)) return rc;
    SSLAM_REQUIRE(M == 0 || (idx_out && dist_out && cnt_out), "%s: idx_out / dist_out / cnt_out is NULL", who);
    SSLAM_REQUIRE(M == 0 || N == 0 || (q && t), "%s: q / t is NULL", who);
    if (M == 0) return 0;
    if (N == 0) {                                              // no train row: every list is empty, no device work
        for (size_t e = 0; e < (size_t)M * k; ++e) { idx_out[e] = -1; dist_out[e] = INFINITY; }
        for (int i = 0; i < M; ++i) cnt_out[i] = 0;
        return 0;
    }
    BFKArgs a{};
    bfk_fill(a, p, D, M, N);
    a.words_ok = D % 4 == 0;                                   // (slab pieces are 256-byte aligned)
    const size_t rb = bf_row_bytes(norm, D);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bfk_bind(sl, a, p, rb, true, false); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.q), static_cast<const uint8_t*>(q), (size_t)M * rb));
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.t), static_cast<const uint8_t*>(t), (size_t)N * rb));
    if (int rc = bfk_enqueue(s, a, norm, false)) return rc;
    SSLAM_HIP_CHECK(sslam::copy_down(s, idx_out, a.idx_out, (size_t)M * k));
    SSLAM_HIP_CHECK(sslam::copy_down(s, dist_out, a.dist_out, (size_t)M * k));
    SSLAM_HIP_CHECK(sslam::copy_down(s, cnt_out, a.cnt_out, (size_t)M));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_bf_ratio_match_dev(sslam_ctx* ctx, int norm, int D, const void* q_dev, int M, const int32_t* m_dev,
                                        const void* t_dev, int N, const int32_t* n_dev, double ratio, int splits,
                                        int32_t* ij_out_dev, float* dist_out_dev, int32_t* info_out_dev) {
    const char* who = "sslam_bf_ratio_match_dev";
    sslam::BfKnnPlan p;
    if (int rc = bfk_check(who, ctx, norm, D, M, N, 2, splits, &p)) return rc;
    if (int rc = bfk_check_ratio(who, ratio)) return rc;
    SSLAM_REQUIRE(info_out_dev != nullptr, "%s: info_out_dev is NULL", who);
    SSLAM_REQUIRE(M == 0 || (q_dev && ij_out_dev && dist_out_dev), "%s: q_dev / ij_out_dev / dist_out_dev is NULL", who);
    SSLAM_REQUIRE(N == 0 || t_dev, "%s: t_dev is NULL", who);
    BFKArgs a{};
    bfk_fill(a, p, D, M, N);
    a.ratio = ratio;
    a.m_dev = m_dev; a.n_dev = n_dev; a.q = q_dev; a.t = t_dev;
    a.words_ok = D % 4 == 0 && ((uintptr_t)q_dev | (uintptr_t)t_dev) % 4 == 0;
    a.ij_out = ij_out_dev; a.dist_out = dist_out_dev; a.info_out = info_out_dev;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bfk_bind(sl, a, p, bf_row_bytes(norm, D), false, true); })) return rc;
    return bfk_enqueue(ctx->stream, a, norm, true);
}

extern "C" int sslam_bf_ratio_match_host(sslam_ctx* ctx, int norm, int D, const void* q, int M, const void* t, int N,
                                         double ratio, int splits, int32_t* ij_out, float* dist_out, int32_t* k_out) {
    const char* who = "sslam_bf_ratio_match_host";
    sslam::BfKnnPlan p;
    if (int rc = bfk_check(who, ctx, norm, D, M, N, 2, splits, &p)) return rc;
    if (int rc = bfk_check_ratio(who, ratio)) return rc;
    SSLAM_REQUIRE(k_out != nullptr, "%s: k_out is NULL", who);
    SSLAM_REQUIRE(M == 0 || N == 0 || (q && t && ij_out && dist_out), "%s: q / t / ij_out / dist_out is NULL", who);
    *k_out = 0;
    if (M == 0 || N == 0) return 0;
    BFKArgs a{};
    bfk_fill(a, p, D, M, N);
    a.ratio = ratio;
    a.words_ok = D % 4 == 0;                                   // (slab pieces are 256-byte aligned)
    const size_t rb = bf_row_bytes(norm, D);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bfk_bind(sl, a, p, rb, true, true); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.q), static_cast<const uint8_t*>(q), (size_t)M * rb));
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.t), static_cast<const uint8_t*>(t), (size_t)N * rb));
    if (int rc = bfk_enqueue(s, a, norm, true)) return rc;
    int32_t info[4] = {0, 0, 0, 0};
    SSLAM_HIP_CHECK(sslam::copy_down(s, info, a.info_out, 4));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));                  // (the count sizes the rest)
    const size_t kept = (size_t)info[0];
    if (kept) {
        SSLAM_HIP_CHECK(sslam::copy_down(s, ij_out, a.ij_out, kept * 2));
        SSLAM_HIP_CHECK(sslam::copy_down(s, dist_out, a.dist_out, kept));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    *k_out = info[0];
    return 0;
}
