"""Numpy restatement of `cv2.BFMatcher(normType, crossCheck).match(queryDescriptors, trainDescriptors)` for NORM_HAMMING and
NORM_L2, one train image, no mask - what `feature_matcher` calls on the reference's OpenCV branch
(slam/core/features_utils.py:173-178; the matcher is built at :54-55).

PARITY UNPINNED: cv2 is absent here, so nothing below was compared with it.  Written from memory of OpenCV 4.x
(matchers.cpp, batch_distance.cpp) and not confirmed - `UNCONFIRMED` holds the same list for the tests to print:
  * the ORDER of the float32 accumulation of NORM_L2: OpenCV's `normL2Sqr_` adds the squared differences four (or a SIMD
    register's worth) at a time into several partial sums, and which path runs depends on its build; see "defined arithmetic";
  * that `batchDistance` takes the root of every NORM_L2 distance BEFORE it compares them, so that two different sums whose
    float32 roots are equal are a tie, which the lower index wins (built here);
  * the tie rule itself: strict `<` while scanning the train rows in ascending order, so the lowest index wins;
  * what crossCheck does in 4.11: 4.x runs `batchDistance` in both directions and keeps the pairs that are mutual nearest
    neighbours (built here); earlier versions kept, per train row, the closest query row that votes for it, without the
    second test - the two differ when a query's nearest train row prefers another query;
  * that a NaN distance never wins (every comparison with it is false) and that a row whose distances are all NaN, or not
    below FLT_MAX (the initial "best" of the scan), yields no match rather than a match with trainIdx -1;
  * that the result comes in ascending queryIdx with imgIdx 0.

DEFINED ARITHMETIC.  NORM_HAMMING is exact in integers: the number of set bits of a XOR b over all D bytes, returned as
float32.  NORM_L2, per pair and in float32: acc = 0; for k ascending: diff = a_k - b_k (one rounding), acc = fma(diff, diff, acc)
(one rounding); d = sqrt(acc), correctly rounded.  The difference form, never |a|^2 + |b|^2 - 2 a.b.  The kernel performs
the same operations one for one.  (`fma` here: the product of two float32 is exact in float64; the sum with acc is rounded to
float64 and then to float32 - a double rounding that can differ from a true fma only when the float64 sum lands exactly on a
float32 tie; the tests that compare BITS use integer-valued rows, where every step is exact, and the others compare with
`l2="f64"` under a bound.)
"""
import numpy as np

NORM_L2 = 4
NORM_HAMMING = 6
FLT_MAX = float(np.finfo(np.float32).max)

UNCONFIRMED = (
    "NORM_L2: the order of OpenCV's float32 accumulation (SIMD build dependent); here one accumulator, k ascending, fma",
    "NORM_L2: nearest neighbours are compared on the float32 value after the square root",
    "ties: strict <, the lowest index wins",
    "crossCheck in 4.11: mutual nearest neighbours (both directions), not the older one-sided vote",
    "a NaN distance, or one not below FLT_MAX, never wins; a row without a winner has no match",
    "matches in ascending queryIdx, imgIdx 0",
)

_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)
_POPCOUNT32 = _POPCOUNT.astype(np.int32)


# ---- distance of one pair (the plain form) ---------------------------------------------------------------------------
def hamming_pair(a, b):
    return int(_POPCOUNT[np.bitwise_xor(a, b)].sum())


def _f32(v):
    return float(np.float32(v))


def l2_pair(a, b):
    """float32 chain of one pair, k ascending; returns the float32 root as a python float"""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (a - b).astype(np.float32)
        sq = diff.astype(np.float64) ** 2                    # exact: 24 x 24 bits
        part = np.cumsum(sq)                                  # sequential float64 partial sums
        if (part == part.astype(np.float32)).all():
            # every partial sum is a float32 (and, by induction, exact): no step of the float32 chain rounds
            acc = float(part[-1])
        else:
            acc = 0.0
            for s in sq.tolist():
                acc = _f32(acc + s)
        return float(np.sqrt(np.float32(acc)))


def l2_pair_f64(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.sqrt(np.sum(d * d)))


# ---- all distances at once (the vectorised form) ---------------------------------------------------------------------
def distances(q, t, norm, l2="f32"):
    """[M, N] distances: float32 for NORM_HAMMING and NORM_L2 / "f32", float64 for NORM_L2 / "f64" """
    if norm == NORM_HAMMING:
        acc = np.zeros((len(q), len(t)), np.int32)
        for k in range(q.shape[1]):                          # (byte by byte: no [M, N, D] array)
            acc += _POPCOUNT32[np.bitwise_xor(q[:, k, None], t[None, :, k])]
        return acc.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if l2 == "f64":
            d = q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :]
            return np.sqrt((d * d).sum(-1))
        acc = np.zeros((len(q), len(t)), np.float32)
        for k in range(q.shape[1]):
            diff = (q[:, k, None] - t[None, :, k]).astype(np.float32)
            acc = (acc.astype(np.float64) + diff.astype(np.float64) ** 2).astype(np.float32)
        return np.sqrt(acc)


def _check(q, t, norm):
    q, t = np.asarray(q), np.asarray(t)
    want = np.uint8 if norm == NORM_HAMMING else np.float32
    assert norm in (NORM_L2, NORM_HAMMING)
    assert q.dtype == want and t.dtype == want and q.ndim == 2 and t.ndim == 2 and q.shape[1] == t.shape[1]
    return q, t


def match(q, t, norm, cross_check, l2="f32"):
    """-> (ij int32 [K,2], dist [K]) in query order; dist is float32, float64 with l2="f64" """
    q, t = _check(q, t, norm)
    if len(q) == 0 or len(t) == 0:
        return np.empty((0, 2), np.int32), np.empty(0, np.float64 if l2 == "f64" and norm == NORM_L2 else np.float32)
    d = distances(q, t, norm, l2)
    valid = d < FLT_MAX                                     # NaN: False
    dm = np.where(valid, d, np.inf)
    nn_q, nn_t = dm.argmin(1), dm.argmin(0)                 # the first minimum: the lowest index on a tie
    keep = valid.any(1)
    if cross_check:
        keep &= nn_t[nn_q] == np.arange(len(q))             # (a query with a winner makes its train row one with a winner)
    i = np.nonzero(keep)[0]
    return np.stack([i, nn_q[i]], 1).astype(np.int32), d[i, nn_q[i]]


def nearest_loop(q, t, norm, l2="f32"):
    """a plain double loop over the pairs -> (best_q, nn_q, nn_t): per query row the smallest distance and its train row
    (-1: none), per train row its query row"""
    q, t = _check(q, t, norm)
    pair = hamming_pair if norm == NORM_HAMMING else (l2_pair_f64 if l2 == "f64" else l2_pair)
    M, N = len(q), len(t)
    best_q, nn_q = [FLT_MAX] * M, [-1] * M
    best_t, nn_t = [FLT_MAX] * N, [-1] * N
    for i in range(M):
        for j in range(N):
            d = pair(q[i], t[j])
            if d < best_q[i]:
                best_q[i], nn_q[i] = d, j
            if d < best_t[j]:
                best_t[j], nn_t[j] = d, i
    return best_q, nn_q, nn_t


def match_loop(q, t, norm, cross_check, l2="f32", nearest=None):
    """`match` on top of `nearest_loop` (`nearest`: its result, when the caller already has it)"""
    best_q, nn_q, nn_t = nearest or nearest_loop(q, t, norm, l2)
    M = len(q)
    ij, dist = [], []
    for i in range(M):
        j = nn_q[i]
        if j >= 0 and (not cross_check or nn_t[j] == i):
            ij.append((i, j))
            dist.append(best_q[i])
    return (np.array(ij, np.int32).reshape(-1, 2),
            np.array(dist, np.float64 if l2 == "f64" and norm == NORM_L2 else np.float32))


def gaps(d):
    """per row the gap between the smallest and the second smallest entry of d ([M, N], N >= 2)"""
    s = np.sort(d, axis=1)
    return s[:, 1] - s[:, 0]
