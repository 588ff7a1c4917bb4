// bf_match_kernels.hip - brute-force descriptor matching on the GPU: `cv2.BFMatcher(norm, crossCheck).match(des0, des1)`.
//
// Replaces the matcher of the reference's default configuration (`--detector orb --matcher bf`): `_get_opencv_matcher`
// builds `cv2.BFMatcher(norm, crossCheck=True)` (slam/core/features_utils.py:54-55, NORM_HAMMING for ORB / AKAZE, NORM_L2 for
// SIFT) and `feature_matcher` calls `.match(des0, des1)` on it (:173-178), twice per frame.  The same mutual nearest
// neighbour on two ALIKED descriptor sets is a cheap association where a LightGlue forward is not needed.
//
// Semantics (tests/bf_ref.py restates them and lists what could not be confirmed against a real cv2):
//   * NORM_HAMMING (6): rows of D = 1..256 bytes; d = popcount of the XOR over all D bytes, exact, returned as float;
//   * NORM_L2 (4): rows of D = 1..512 float32; per pair ONE accumulator, k ascending: diff = a_k - b_k (rounded),
//     acc = fmaf(diff, diff, acc), then d = sqrtf(acc) correctly rounded.  The difference form, never |a|^2 + |b|^2 - 2 a.b;
//   * nn_q[i] = argmin_j d(i, j), nn_t[j] = argmin_i d(i, j), strict <, the lowest index wins a tie; for L2 the comparison
//     is on the float AFTER the root; a NaN distance, or one that is not below FLT_MAX, never wins; a row with no winner has
//     no match;
//   * crossCheck off: (i, nn_q[i], d) per query row with a winner; on: only where nn_t[nn_q[i]] == i.  Query order.
//
// One memset of the keys and two launches:
//   1. bf_distance_kernel<Norm>, a workgroup of 256 per 64 x 64 tile of the query x train grid.  Both tiles are staged through
//      LDS in chunks of 32 elements (words of 4 bytes for Hamming: a D that is no multiple of 4 is zero-padded byte by byte
//      as it is staged, never read past the row; floats for L2), TRANSPOSED (k-major), so that a thread's fragment of one k
//      - 4 queries, 4 trains - is two 16-byte LDS reads into registers, the query one a broadcast over 16 lanes; the 4 x 4
//      accumulators stay in registers over the chunks.  The M x N matrix never exists: a thread folds its 16 distances into
//      the 64-bit key  (float bits of d) << 32 | the other side's index  - distances are non-negative, so bit order is value
//      order, and the lower index wins a tie -, the keys are reduced over the lanes that share a row (a column) and through
//      LDS over the waves, and 64 lanes per side and workgroup issue a 64-bit vector atomicMin on the rows' (columns') keys
//      in global memory.  A minimum does not depend on the order of arrival: the outputs are bitwise the same from run to
//      run.  Scratch: 8 (M + N) bytes.
//   2. bf_finish_kernel, one workgroup of 1024: the mutual test and the compaction in query order (sslam::block_compact).
// The L2 inner loop is plain fp32 VALU on purpose, no matrix core: the arithmetic above is the contract.  (The compiler pairs
// the subtracts and the fmas of two pairs into v_pk_add_f32 / v_pk_fma_f32 - each half one IEEE operation, the same bits -
// and the build's ISA guard checks that none has the op_sel form it bars.)
#include "bf_tile.hpp"
#include "geom_common.hpp"

namespace {

using namespace sslam::bf;               // the limits, the norms and the tile loop: bf_tile.hpp, shared with bf_knn_kernels.hip

constexpr int BF_FIN_T = 1024;

struct BFArgs : BFRows {
    int cross_check;
    unsigned long long* best_q;               // [M] min over the trains of (bits(d) << 32 | train)
    unsigned long long* best_t;               // [N] min over the queries of (bits(d) << 32 | query)
    int32_t* ij_out; float* dist_out; int32_t* info_out;
};

// ---- 1. a 64 x 64 tile of pairs per workgroup: the minimum key of every row and of every column of the tile ----------
template <class Norm>
__global__ __launch_bounds__(BF_T) void bf_distance_kernel(BFArgs a) {
    using Elem = typename Norm::Elem;
    __shared__ BFVec4<Elem> sq4[BF_STAGE_VEC4], st4[BF_STAGE_VEC4];
    __shared__ unsigned long long s_row[BF_TILE], s_col[BF_TILE];
    const int m = bf_count(a.m_dev, a.M), n = bf_count(a.n_dev, a.N);
    const int q0 = blockIdx.y * BF_TILE, t0 = blockIdx.x * BF_TILE;
    if (q0 >= m || t0 >= n) return;          // (the whole workgroup: the counts are uniform)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if (tid < BF_TILE) { s_row[tid] = BF_NONE; s_col[tid] = BF_NONE; }       // (ordered by the tile loop's first barrier: E >= 1)

    Elem acc[4][4];
    bf_tile_distances<Norm>(a, q0, t0, m, n, sq4, st4, acc);

    unsigned long long rk[4] = {BF_NONE, BF_NONE, BF_NONE, BF_NONE}, ck[4] = {BF_NONE, BF_NONE, BF_NONE, BF_NONE};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = Norm::finish(acc[i][j]);
            const int qi = q0 + 4 * ty + i, tj = t0 + 4 * tx + j;
            if (qi < m && tj < n && d < FLT_MAX) {                          // (NaN fails the comparison)
                rk[i] = bf_min(rk[i], bf_key(d, tj));
                ck[j] = bf_min(ck[j], bf_key(d, qi));
            }
        }
    // a row's 16 threads are 16 adjacent lanes; a column's 16 threads are 4 lanes (16 apart) of each of the 4 waves
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) rk[i] = bf_min(rk[i], __shfl_xor(rk[i], o));
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) ck[i] = bf_min(ck[i], __shfl_xor(ck[i], o));
    }
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s_row[4 * ty + i] = rk[i];
    }
    if ((tid & 63) < 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ck[j] != BF_NONE) atomicMin(&s_col[4 * tx + j], ck[j]);
    }
    __syncthreads();
    if (tid < BF_TILE) {
        const unsigned long long v = s_row[tid];
        if (v != BF_NONE) atomicMin(&a.best_q[q0 + tid], v);                 // (a key exists only for q0 + tid < m)
    } else if (tid < 2 * BF_TILE) {
        const unsigned long long v = s_col[tid - BF_TILE];
        if (v != BF_NONE) atomicMin(&a.best_t[t0 + tid - BF_TILE], v);
    }
}

// ---- 2. the mutual test, the matches in query order, the counts (one workgroup) -----------------------------------
__global__ __launch_bounds__(BF_FIN_T) void bf_finish_kernel(BFArgs a) {
    __shared__ int wsum[BF_FIN_T / 64], base;
    const int m = bf_count(a.m_dev, a.M), n = bf_count(a.n_dev, a.N);
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += BF_FIN_T) {
        const int i = i0 + threadIdx.x;
        bool keep = false;
        int j = 0;
        float d = 0.f;
        if (i < m) {
            const unsigned long long key = a.best_q[i];
            if (key != BF_NONE) {
                j = (int)(uint32_t)key;
                d = __uint_as_float((uint32_t)(key >> 32));
                keep = !a.cross_check || (uint32_t)a.best_t[j] == (uint32_t)i;
            }
        }
        sslam::block_compact<BF_FIN_T>(keep, wsum, base, [&](int o) {
            a.ij_out[2 * o] = i; a.ij_out[2 * o + 1] = j;
            a.dist_out[o] = d;
        });
    }
    if (threadIdx.x < 4) a.info_out[threadIdx.x] = threadIdx.x == 0 ? base : threadIdx.x == 1 ? m : threadIdx.x == 2 ? n : 0;
}

int bf_enqueue(hipStream_t s, const BFArgs& a, int norm) {
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    const size_t rows = (size_t)a.M + (size_t)a.N;
    if (rows) SSLAM_HIP_CHECK(hipMemsetAsync(a.best_q, 0xff, rows * sizeof(unsigned long long), s));
    if (a.M > 0 && a.N > 0) {
        const dim3 grid(sslam::cdiv(a.N, BF_TILE), sslam::cdiv(a.M, BF_TILE));
        if (norm == BF_NORM_HAMMING) hipLaunchKernelGGL(bf_distance_kernel<HammingNorm>, grid, dim3(BF_T), 0, s, a);
        else hipLaunchKernelGGL(bf_distance_kernel<L2Norm>, grid, dim3(BF_T), 0, s, a);
    }
    hipLaunchKernelGGL(bf_finish_kernel, dim3(1), dim3(BF_FIN_T), 0, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

// the slab-backed pointers of BFArgs, in slab order.  host: the inputs and outputs are the slab's too
void bf_bind(sslam::Slab& sl, BFArgs& a, size_t row_bytes, bool host) {
    const size_t M = (size_t)a.M, N = (size_t)a.N;
    a.best_q = sl.take<unsigned long long>(M + N);
    a.best_t = a.best_q ? a.best_q + M : nullptr;
    if (!host) return;
    a.q = sl.take<uint8_t>(M * row_bytes); a.t = sl.take<uint8_t>(N * row_bytes);
    a.ij_out = sl.take<int32_t>(M * 2); a.dist_out = sl.take<float>(M); a.info_out = sl.take<int32_t>(4);
}

}  // namespace

extern "C" int sslam_bf_match_dev(sslam_ctx* ctx, int norm, int cross_check, int D, const void* q_dev, int M,
                                  const int32_t* m_dev, const void* t_dev, int N, const int32_t* n_dev,
                                  int32_t* ij_out_dev, float* dist_out_dev, int32_t* info_out_dev) {
    const char* who = "sslam_bf_match_dev";
    if (int rc = bf_check(who, ctx, norm, D, M, N)) return rc;
    SSLAM_REQUIRE(info_out_dev != nullptr, "%s: info_out_dev is NULL", who);
    SSLAM_REQUIRE(M == 0 || (q_dev && ij_out_dev && dist_out_dev), "%s: q_dev / ij_out_dev / dist_out_dev is NULL", who);
    SSLAM_REQUIRE(N == 0 || t_dev, "%s: t_dev is NULL", who);
    BFArgs a{};
    a.D = D; a.M = M; a.N = N; a.m_dev = m_dev; a.n_dev = n_dev; a.q = q_dev; a.t = t_dev; a.cross_check = cross_check != 0;
    a.words_ok = D % 4 == 0 && ((uintptr_t)q_dev | (uintptr_t)t_dev) % 4 == 0;
    a.ij_out = ij_out_dev; a.dist_out = dist_out_dev; a.info_out = info_out_dev;
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bf_bind(sl, a, bf_row_bytes(norm, D), false); })) return rc;
    return bf_enqueue(ctx->stream, a, norm);
}

extern "C" int sslam_bf_match_host(sslam_ctx* ctx, int norm, int cross_check, int D, const void* q, int M, const void* t,
                                   int N, int32_t* ij_out, float* dist_out, int32_t* k_out) {
    const char* who = "sslam_bf_match_host";
    if (int rc = bf_check(who, ctx, norm, D, M, N)) return rc;
    SSLAM_REQUIRE(k_out != nullptr, "%s: k_out is NULL", who);
    SSLAM_REQUIRE(M == 0 || N == 0 || (q && t && ij_out && dist_out), "%s: q / t / ij_out / dist_out is NULL", who);
    *k_out = 0;
    if (M == 0 || N == 0) return 0;
    BFArgs a{};
    a.D = D; a.M = M; a.N = N; a.cross_check = cross_check != 0;
    a.words_ok = D % 4 == 0;                                   // (slab pieces are 256-byte aligned)
    const size_t rb = bf_row_bytes(norm, D);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = sslam::ctx_bind(ctx, [&](sslam::Slab& sl) { bf_bind(sl, a, rb, true); })) return rc;
    hipStream_t s = ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.q), static_cast<const uint8_t*>(q), (size_t)M * rb));
    SSLAM_HIP_CHECK(sslam::copy_up(s, static_cast<const uint8_t*>(a.t), static_cast<const uint8_t*>(t), (size_t)N * rb));
    if (int rc = bf_enqueue(s, a, norm)) return rc;
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
