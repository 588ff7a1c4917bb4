"""Numpy restatement of `cv2.BFMatcher(normType).knnMatch(queryDescriptors, trainDescriptors, k)` and of Lowe's ratio test on
its k = 2 result, for NORM_HAMMING and NORM_L2, one train image, no mask.  Nothing in the reference calls either; they are what
a user of the drop-in `BFMatcher` expects beside `match` (tests/bf_ref.py, whose distances these are).

PARITY UNPINNED: cv2 is absent here, so nothing below was compared with it.  Written from memory of OpenCV 4.x
(matchers.cpp, batch_distance.cpp) and not confirmed - `UNCONFIRMED` holds the same list for the tests to print.

DEFINED.  The distances are `bf_ref.distances`; a pair is valid iff d < FLT_MAX (a NaN never is).  The neighbours of query
row i are its valid train rows in ascending order of the key (float32 d, train index), the first min(k, valid) of them: a
total order, so the result does not depend on how the work is split.  idx int32 [M, k] is padded with -1, dist [M, k] with
+inf, cnt int32 [M] counts the neighbours.  The ratio test keeps row i iff cnt[i] >= 2 and float64(d1) < ratio * float64(d2),
one float64 multiply - Python's `m.distance < ratio * n.distance` on DMatch floats - and gives (i, idx1, d1) in query order.
"""
import numpy as np

import bf_ref
from bf_ref import FLT_MAX, NORM_HAMMING, NORM_L2  # noqa: F401  (re-exported)

MAX_K = 8

UNCONFIRMED = bf_ref.UNCONFIRMED[:2] + (
    "knnMatch ties: cv2's batchDistance keeps the lower train index first among equal distances (here: the key (d, index))",
    "knnMatch: a row with fewer than k valid train rows gets a shorter list (here cnt < k, idx -1, dist +inf in the arrays)",
    "knnMatch with crossCheck=True asserts k == 1; each list then holds the mutual match or nothing",
    "a NaN distance, or one not below FLT_MAX, is never a neighbour",
    "FlannBasedMatcher with a KD-tree index refuses uint8 descriptors",
)

_memo = {}


def case_distances(case, l2="f32"):
    """the [M, N] distance matrix of a tests/bf_cases.py case, computed once and left unchanged"""
    key = (case["name"], l2)
    if key not in _memo:
        d = bf_ref.distances(case["q"], case["t"], case["norm"], l2)
        d.setflags(write=False)
        _memo[key] = d
    return _memo[key]


def knn_of_distances(d, k):
    """-> (idx int32 [M,k], dist [M,k] of d's dtype, cnt int32 [M]) of a distance matrix"""
    assert 1 <= k <= MAX_K
    M, N = d.shape
    valid = d < FLT_MAX                                     # NaN: False
    dm = np.where(valid, d, np.inf)
    order = np.argsort(dm, axis=1, kind="stable")[:, :k]    # stable: the lower index first among equal distances
    cnt = np.minimum(valid.sum(1), k).astype(np.int32)
    idx = np.full((M, k), -1, np.int32)
    dist = np.full((M, k), np.inf, d.dtype)
    have = np.arange(k)[None, :] < cnt[:, None]
    kk = order.shape[1]
    idx[:, :kk] = np.where(have[:, :kk], order, -1)
    dist[:, :kk] = np.where(have[:, :kk], np.take_along_axis(dm, order, 1), np.inf)
    return idx, dist, cnt


def knn(q, t, norm, k, l2="f32"):
    q, t = bf_ref._check(q, t, norm)
    if len(q) == 0 or len(t) == 0:
        return (np.full((len(q), k), -1, np.int32), np.full((len(q), k), np.inf, np.float32), np.zeros(len(q), np.int32))
    return knn_of_distances(bf_ref.distances(q, t, norm, l2), k)


def knn_loop(q, t, norm, k):
    """a plain double loop: per query row the valid pairs sorted as (d, j) tuples"""
    q, t = bf_ref._check(q, t, norm)
    pair = bf_ref.hamming_pair if norm == NORM_HAMMING else bf_ref.l2_pair
    idx, dist, cnt = [], [], []
    for i in range(len(q)):
        keys = []
        for j in range(len(t)):
            d = pair(q[i], t[j])
            if d < FLT_MAX:
                keys.append((d, j))
        keys.sort()
        keys = keys[:k]
        cnt.append(len(keys))
        idx.append([j for _, j in keys] + [-1] * (k - len(keys)))
        dist.append([d for d, _ in keys] + [np.inf] * (k - len(keys)))
    return (np.array(idx, np.int32).reshape(len(q), k), np.array(dist, np.float32).reshape(len(q), k), np.array(cnt, np.int32))


def ratio_of_knn(idx, dist, cnt, ratio):
    """the ratio test on a k >= 2 result -> (ij int32 [K,2], dist float32 [K]) in query order"""
    assert np.isfinite(ratio) and ratio > 0 and idx.shape[1] >= 2
    with np.errstate(invalid="ignore"):
        keep = (cnt >= 2) & (dist[:, 0].astype(np.float64) < np.float64(ratio) * dist[:, 1].astype(np.float64))
    i = np.nonzero(keep)[0]
    return np.stack([i, idx[i, 0]], 1).astype(np.int32), dist[i, 0]


def ratio_match(q, t, norm, ratio):
    return ratio_of_knn(*knn(q, t, norm, 2), ratio)


def tied_rows(d, k):
    """the number of rows whose k-th and (k+1)-th neighbours are at the same distance (N > k)"""
    s = np.sort(np.where(d < FLT_MAX, d, np.inf), axis=1)
    return int((s[:, k - 1] == s[:, k]).sum())
