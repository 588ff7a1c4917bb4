"""`sslam_bf_match_host` / `_dev` against the restatement of cv2.BFMatcher.match (tests/bf_ref.py): Hamming and integer-valued L2
are exact, so pairs, count and distances must be IDENTICAL; unit rows must give the float64 restatement's pairs (their gaps
leave float32 no choice: tests/test_bf_ref.py) and distances within the float32 chain's bound; the device entry with device
counts, with a negative count, and chained into `sslam_fmat_ransac_dev`."""
import numpy as np
import pytest

import bf_cases
import bf_ref
import two_view
from conftest import load_pkg

pytestmark = pytest.mark.gpu

EXACT = {c["name"]: c for c in bf_cases.exact_cases()}


@pytest.fixture(scope="module")
def B(gpu_ctx):
    return load_pkg("bf_matcher")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_identical(got, want, what):
    (ij, dist), (ij_w, dist_w) = got, want
    assert ij.dtype == np.int32 and dist.dtype == np.float32
    assert len(ij) == len(ij_w) == len(dist), (what, len(ij), len(ij_w))
    np.testing.assert_array_equal(ij, ij_w, err_msg=what)
    np.testing.assert_array_equal(_bits(dist), _bits(dist_w), err_msg=what)


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_equal_the_restatement(B, gpu_ctx, name, cross_check):
    c = EXACT[name]
    got = B.BFMatcher(c["norm"], crossCheck=cross_check, ctx=gpu_ctx).match_arrays(c["q"], c["t"])
    _assert_identical(got, bf_cases.expected(c, cross_check), f"{name} crossCheck={cross_check}")
    if "planted" in c:
        pairs = set(map(tuple, got[0].tolist()))
        assert all((int(i), int(j)) in pairs for i, j in c["planted"])
    if name == "l2_nonfinite_40x50_d16":
        assert bf_cases.NONFINITE_QUERY not in got[0][:, 0] and bf_cases.NONFINITE_TRAIN not in got[0][:, 1]


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("norm,M,N,D", [(bf_ref.NORM_HAMMING, 2500, 1100, 8), (bf_ref.NORM_L2, 1025, 2049, 5),
                                        (bf_ref.NORM_HAMMING, 65536, 64, 3), (bf_ref.NORM_HAMMING, 64, 65536, 4)])
def test_more_rows_than_one_compaction_turn_and_the_largest_side(B, gpu_ctx, norm, M, N, D, cross_check):
    """the finish kernel compacts 1 024 query rows per turn: 1 025 / 2 500 rows take several, 65 536 (the limit, 1 024 tiles on a
    grid axis) sixty-four; exact inputs, identical results"""
    r = np.random.default_rng(M + N + D)
    if norm == bf_ref.NORM_HAMMING:
        q, t = r.integers(0, 256, (M, D), dtype=np.uint8), r.integers(0, 256, (N, D), dtype=np.uint8)
    else:
        q, t = r.integers(-8, 9, (M, D)).astype(np.float32), r.integers(-8, 9, (N, D)).astype(np.float32)
    got = B.BFMatcher(norm, crossCheck=cross_check, ctx=gpu_ctx).match_arrays(q, t)
    want = bf_ref.match(q, t, norm, cross_check)
    assert len(want[0]) > (1024 if not cross_check and M > 1024 else 0)
    _assert_identical(got, want, f"{M}x{N}x{D}")


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("seed", [0, 2])
def test_unit_rows_give_the_float64_pairs(B, gpu_ctx, seed, cross_check):
    """The gap between the best and the second-best squared distance (>= 1e-4, asserted first, over rows and columns) is
    more than twice the float32 chain's error bound (D + 2) 2^-24 S <= 3.1e-5, so the float64 argmin is the only legal
    answer, for every row.  Distances: the bound on the squared sum is 7.8e-6 relative and the root halves it."""
    c = bf_cases.l2_unit_case(seed)
    sq = bf_ref.distances(c["q"], c["t"], c["norm"], "f64") ** 2
    assert bf_ref.gaps(sq).min() >= 1e-4 and bf_ref.gaps(sq.T).min() >= 1e-4
    ij64, d64 = bf_cases.expected(c, cross_check, "f64")
    ij, dist = B.BFMatcher(B.NORM_L2, crossCheck=cross_check, ctx=gpu_ctx).match_arrays(c["q"], c["t"])
    err = np.abs(dist.astype(np.float64) - d64[:len(dist)]) / d64[:len(dist)] if len(dist) == len(d64) else None
    print(f"{c['name']} crossCheck={cross_check}: K {len(ij)} (float64: {len(ij64)}), "
          f"max |dist - dist64| / dist64 = {err.max() if err is not None else 'n/a'}")
    np.testing.assert_array_equal(ij, ij64)
    assert (np.abs(dist.astype(np.float64) - d64) <= 1e-5 * d64).all()
    if seed == 0 and cross_check:
        assert len(ij) == 114


@pytest.mark.parametrize("name", ["ham_257x191_d61", "ham_257x191_d1", "l2int_257x191_d129", "l2unit"])
def test_the_same_call_twice_is_bitwise_the_same(B, gpu_ctx, name):
    c = bf_cases.l2_unit_case() if name == "l2unit" else EXACT[name]
    m = B.BFMatcher(c["norm"], crossCheck=True, ctx=gpu_ctx)
    first = m.match_arrays(c["q"], c["t"])
    for _ in range(3):
        again = m.match_arrays(c["q"], c["t"])
        _assert_identical(again, first, name)


def _dev_match(B, ctx, c, cross_check, M, N, m_dev, n_dev, fill=0):
    """sslam_bf_match_dev on buffers of M x N rows (the case's rows, then `fill`) with the device counts m_dev / n_dev (None:
    no count buffer).  -> (ij [K,2], dist [K], info [4]); asserts that nothing was written past K."""
    q, t = c["q"], c["t"]
    D = q.shape[1]
    qb, tb = np.full((M, D), fill, q.dtype), np.full((N, D), fill, t.dtype)
    qb[:min(M, len(q))] = q[:M]
    tb[:min(N, len(t))] = t[:N]
    d_q, d_t = ctx.upload(qb), ctx.upload(tb)
    d_m = ctx.upload(np.array([m_dev], np.int32)) if m_dev is not None else None
    d_n = ctx.upload(np.array([n_dev], np.int32)) if n_dev is not None else None
    d_ij, d_dist = ctx.upload(np.full((M, 2), -1, np.int32)), ctx.upload(np.full(M, -1, np.float32))
    d_info = ctx.upload(np.full(4, -9, np.int32))
    try:
        B.BFMatcher(c["norm"], crossCheck=cross_check).match_dev(ctx, D, d_q, M, d_t, N, d_ij, d_dist, d_info, m_dev=d_m, n_dev=d_n)
        ctx.sync()
        ij, dist, info = np.empty((M, 2), np.int32), np.empty(M, np.float32), np.empty(4, np.int32)
        ctx.d2h(ij, d_ij); ctx.d2h(dist, d_dist); ctx.d2h(info, d_info)
    finally:
        for p in (d_q, d_t, d_m, d_n, d_ij, d_dist, d_info):
            if p is not None:
                ctx.free(p)
    K = int(info[0])
    assert 0 <= K <= M
    assert (ij[K:] == -1).all() and (dist[K:] == -1).all()
    return ij[:K], dist[:K], info


@pytest.mark.parametrize("cross_check", [False, True])
@pytest.mark.parametrize("name", ["ham_257x191_d32", "ham_257x191_d61", "l2int_257x191_d128", "l2int_257x191_d3"])
def test_device_entry_with_device_counts_below_the_bounds(B, gpu_ctx, name, cross_check):
    """(257, 191) buffers, m_dev = 63, n_dev = 65: the result is the host entry's on the sliced arrays.  The rows beyond the
    counts are zeros - for integer-valued rows a zero row is close to everything - and never match."""
    c = EXACT[name]
    cut = dict(c, q=c["q"].copy(), t=c["t"].copy())
    cut["q"][63:] = 0
    cut["t"][65:] = 0
    ij, dist, info = _dev_match(B, gpu_ctx, cut, cross_check, 257, 191, 63, 65)
    want = bf_ref.match(c["q"][:63], c["t"][:65], c["norm"], cross_check)
    _assert_identical((ij, dist), want, name)
    assert info.tolist() == [len(want[0]), 63, 65, 0]
    assert (ij[:, 0] < 63).all() and (ij[:, 1] < 65).all()
    host = B.BFMatcher(c["norm"], crossCheck=cross_check, ctx=gpu_ctx).match_arrays(c["q"][:63], c["t"][:65])
    _assert_identical((ij, dist), host, name + " (host entry)")


def test_device_entry_without_count_buffers_and_with_counts_above_the_bounds(B, gpu_ctx):
    c = EXACT["ham_63x65_d61"]                                              # (an odd D: the device rows are not word-aligned)
    want = bf_cases.expected(c, True)
    ij, dist, info = _dev_match(B, gpu_ctx, c, True, 63, 65, None, None)
    _assert_identical((ij, dist), want, "no counts")
    assert info.tolist() == [len(want[0]), 63, 65, 0]
    ij, dist, info = _dev_match(B, gpu_ctx, c, True, 63, 65, 1 << 20, 66)   # clamped to the bounds
    _assert_identical((ij, dist), want, "counts above the bounds")
    assert info.tolist() == [len(want[0]), 63, 65, 0]


@pytest.mark.parametrize("m_dev,n_dev", [(-1, 65), (63, -1), (-5, -5), (0, 65), (63, 0)])
def test_device_entry_with_a_negative_or_zero_count_matches_nothing(B, gpu_ctx, m_dev, n_dev):
    c = EXACT["ham_63x65_d32"]
    ij, dist, info = _dev_match(B, gpu_ctx, c, False, 63, 65, m_dev, n_dev)
    assert len(ij) == 0 and info.tolist() == [0, max(m_dev, 0), max(n_dev, 0), 0]


def _planted_scene():
    """the planted Hamming case with pixel coordinates: the 200 planted pairs see a synthetic two-view scene (20 % of them
    off the epipolar geometry), every other keypoint lies anywhere"""
    c = bf_cases.planted_hamming()
    p1, p2, _truth = two_view.make_matches(len(c["planted"]), outlier_frac=0.2, noise=0.3, seed=21)
    rng = np.random.default_rng(22)
    kp1 = rng.uniform(0, 1000, (len(c["q"]), 2)).astype(np.float32)
    kp2 = rng.uniform(0, 1000, (len(c["t"]), 2)).astype(np.float32)
    kp1[c["planted"][:, 0]] = p1
    kp2[c["planted"][:, 1]] = p2
    return c, kp1, kp2


def test_device_match_chains_into_the_device_ransac_filter(B, gpu_ctx):
    """sslam_bf_match_dev -> sslam_fmat_ransac_dev on the pairs and the count it left on the device: the kept pairs are those
    of the host route (match_arrays, gather the pixels, sslam_fmat_ransac_host)."""
    E = load_pkg("epipolar")
    ctx = gpu_ctx
    c, kp1, kp2 = _planted_scene()
    M, N, D = len(c["q"]), len(c["t"]), c["q"].shape[1]
    ij_h, _ = B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=ctx).match_arrays(c["q"], c["t"])
    assert len(ij_h) >= 200
    _F, mask, meta = E.find_fundamental_ransac(kp1[ij_h[:, 0]], kp2[ij_h[:, 1]], 3.0, 0.99, ctx=ctx)
    assert mask is not None and 120 <= mask.sum() < len(ij_h)
    want = ij_h[mask]

    d = [ctx.upload(a) for a in (c["q"], c["t"], kp1, kp2)]
    d_ij, d_dist, d_info = ctx.malloc(M * 8), ctx.malloc(M * 4), ctx.malloc(16)
    d_kept, d_finfo = ctx.upload(np.full((M, 2), -1, np.int32)), ctx.malloc(16)
    try:
        B.BFMatcher(B.NORM_HAMMING, crossCheck=True).match_dev(ctx, D, d[0], M, d[1], N, d_ij, d_dist, d_info)
        E.filter_matches_dev(ctx, M, d_info, d[2], d[3], d_ij, d_kept, d_finfo, thresh=3.0)
        ctx.sync()
        kept, finfo = np.empty((M, 2), np.int32), np.empty(4, np.int32)
        ctx.d2h(kept, d_kept); ctx.d2h(finfo, d_finfo)
    finally:
        for p in d + [d_ij, d_dist, d_info, d_kept, d_finfo]:
            ctx.free(p)
    assert finfo[0] == len(want) == meta["inliers"]
    np.testing.assert_array_equal(kept[:finfo[0]], want)
    assert (kept[finfo[0]:] == -1).all()
