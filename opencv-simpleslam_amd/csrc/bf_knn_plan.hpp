// bf_knn_plan.hpp - the host decisions of the k-nearest-neighbour matcher (bf_knn_kernels.hip), plain C++17 without a HIP
// include so that tests/test_bf_knn_plan.py can compile it with the host compiler:
//   * K, the list length the kernels are instantiated for: the smallest of 2 / 4 / 8 that is >= k;
//   * S, the number of column splits: the grid is S x ceil(M / 64) workgroups, and one pair of 2 048 x 2 048 has only 32 row
//     tiles, so the train tiles are shared out among S workgroups per row tile until the grid fills the 256 compute units
//     about twice.  S is in 1..ceil(N / 64) (0 when N is 0: nothing to launch);
//   * the range of train tiles of every split: split s walks [s T / S, (s + 1) T / S) of the T = ceil(N / 64) tiles -
//     consecutive, disjoint, none empty, sizes that differ by at most one;
//   * the scratch bytes: S lists of K keys of 8 bytes per query row.
#pragma once
#include <cstddef>
#include <cstdio>

namespace sslam {

constexpr int BFK_TILE = 64;             // rows of a tile (bf_tile.hpp's BF_TILE; bf_knn_kernels.hip asserts the two agree)
constexpr int BFK_MIN_K = 1, BFK_MAX_K = 8;
constexpr int BFK_TARGET_WORKGROUPS = 2 * 256;      // two per compute unit

struct BfKnnPlan {
    int k = 0;                            // neighbours asked for
    int K = 0;                            // list length of the kernels: 2, 4 or 8
    int row_tiles = 0, tiles = 0;         // ceil(M / 64), ceil(N / 64)
    int S = 0;                            // column splits
    size_t scratch_bytes = 0;             // 8 S M K
    int begin(int s) const { return S > 0 ? (int)((long long)s * tiles / S) : 0; }       // first train tile of split s; begin(S) = tiles
};

inline int bfk_cdiv(int a, int b) { return (a + b - 1) / b; }

inline int bfk_list_length(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : 8; }

// 0, or 2 with a message that names the value
inline int bfk_check_k(const char* who, int k, char* msg, size_t n) {
    if (k >= BFK_MIN_K && k <= BFK_MAX_K) return 0;
    std::snprintf(msg, n, "%s: k %d outside %d..%d", who, k, BFK_MIN_K, BFK_MAX_K);
    return 2;
}

// splits: 0 lets the plan choose, 1..ceil(N / 64) is honoured, anything else is refused
inline int bfk_check_splits(const char* who, int splits, int N, char* msg, size_t n) {
    const int tiles = bfk_cdiv(N, BFK_TILE);
    if (splits >= 0 && splits <= tiles) return 0;
    std::snprintf(msg, n, "%s: splits %d outside 0..%d (0: chosen here; at most one per 64 train rows, N = %d)", who, splits, tiles, N);
    return 2;
}

// (M, N, k, splits have passed the checks)
inline BfKnnPlan bfk_plan(int M, int N, int k, int splits) {
    BfKnnPlan p;
    p.k = k;
    p.K = bfk_list_length(k);
    p.row_tiles = bfk_cdiv(M, BFK_TILE);
    p.tiles = bfk_cdiv(N, BFK_TILE);
    if (splits > 0) p.S = splits;
    else if (p.tiles > 0) {
        const int want = bfk_cdiv(BFK_TARGET_WORKGROUPS, p.row_tiles > 0 ? p.row_tiles : 1);
        p.S = want < 1 ? 1 : want > p.tiles ? p.tiles : want;
    }
    p.scratch_bytes = (size_t)8 * (size_t)p.S * (size_t)M * (size_t)p.K;
    return p;
}

}  // namespace sslam
