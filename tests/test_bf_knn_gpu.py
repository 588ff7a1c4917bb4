"""`sslam_bf_knn_match_host` / `_dev` and `sslam_bf_ratio_match_host` / `_dev` against the restatement of knnMatch and of the
ratio test (tests/bf_knn_ref.py).  Hamming and integer-valued L2 are exact, so idx, the bits of dist and cnt must be IDENTICAL -
for every k, for every number of column splits, with the ties at the k-th place that these cases hold (tests/test_bf_knn_ref.py
counts them); k = 1 must be `match` without cross-check bit for bit; unit rows must give the float64 restatement's neighbours
where their gaps leave float32 no choice; the device entries with device counts; the ratio test chained into
`sslam_fmat_ransac_dev`."""
import numpy as np
import pytest

import bf_cases
import bf_knn_ref as R
import bf_ref
import two_view
from conftest import load_pkg

pytestmark = pytest.mark.gpu

EXACT = {c["name"]: c for c in bf_cases.exact_cases()}
L2_EXACT = [c["name"] for c in bf_cases.l2_exact_cases()]
KS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def B(gpu_ctx):
    return load_pkg("bf_matcher")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_identical(got, want, what):
    (idx, dist, cnt), (idx_w, dist_w, cnt_w) = got, want
    assert idx.dtype == np.int32 and dist.dtype == np.float32 and cnt.dtype == np.int32
    assert idx.shape == idx_w.shape and dist.shape == dist_w.shape and cnt.shape == cnt_w.shape, what
    np.testing.assert_array_equal(cnt, cnt_w, err_msg=what)
    np.testing.assert_array_equal(idx, idx_w, err_msg=what)
    np.testing.assert_array_equal(_bits(dist), _bits(dist_w), err_msg=what)


def _assert_pairs_identical(got, want, what):
    (ij, dist), (ij_w, dist_w) = got, want
    assert ij.dtype == np.int32 and dist.dtype == np.float32 and len(ij) == len(ij_w) == len(dist), (what, len(ij), len(ij_w))
    np.testing.assert_array_equal(ij, ij_w, err_msg=what)
    np.testing.assert_array_equal(_bits(dist), _bits(dist_w), err_msg=what)


def _tiles(N):
    return -(-N // 64)


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_equal_the_restatement(B, gpu_ctx, name):
    """k = 1, 2, 3, 8 (every list length of the kernels, and k below it), splits chosen by the plan, 1 and the largest"""
    c = EXACT[name]
    m = B.BFMatcher(c["norm"], ctx=gpu_ctx)
    d = R.case_distances(c)
    for k in KS:
        want = R.knn_of_distances(d, k)
        for splits in sorted({0, 1, _tiles(len(c["t"]))}):
            _assert_identical(m.knn_match_arrays(c["q"], c["t"], k, splits=splits), want, f"{name} k={k} splits={splits}")
    if name == "l2_nonfinite_40x50_d16":
        idx, _dist, cnt = m.knn_match_arrays(c["q"], c["t"], 8)
        assert cnt[bf_cases.NONFINITE_QUERY] == 0 and bf_cases.NONFINITE_TRAIN not in idx and (np.delete(cnt, bf_cases.NONFINITE_QUERY) == 8).all()


@pytest.mark.parametrize("name", ["ham_63x65_d32", "l2int_63x65_d3"])
def test_fewer_train_rows_than_k_are_padded(B, gpu_ctx, name):
    c = EXACT[name]
    m = B.BFMatcher(c["norm"], ctx=gpu_ctx)
    for N in (1, 2, 3, 8):
        for k in (2, 3, 8):
            got = m.knn_match_arrays(c["q"], c["t"][:N], k)
            _assert_identical(got, R.knn(c["q"], c["t"][:N], c["norm"], k), f"{name} N={N} k={k}")
            assert (got[2] == min(k, N)).all() and (got[0][:, min(k, N):] == -1).all() and np.isposinf(got[1][:, min(k, N):]).all()


@pytest.mark.parametrize("name", list(EXACT) + ["l2unit_s0", "l2unit_s5"])
def test_k1_is_match_without_cross_check_bit_for_bit(B, gpu_ctx, name):
    """the two kernels share one arithmetic chain (csrc/bf_tile.hpp): real-valued rows need no restatement here"""
    c = bf_cases.l2_unit_case(int(name[-1])) if name.startswith("l2unit") else EXACT[name]
    m = B.BFMatcher(c["norm"], crossCheck=False, ctx=gpu_ctx)
    ij, dist = m.match_arrays(c["q"], c["t"])
    idx, d, cnt = m.knn_match_arrays(c["q"], c["t"], 1)
    rows = np.nonzero(cnt)[0]
    _assert_pairs_identical((np.stack([rows, idx[rows, 0]], 1).astype(np.int32), d[rows, 0]), (ij, dist), name)
    idx2, d2, _ = m.knn_match_arrays(c["q"], c["t"], 2)                     # and the first column of any longer list
    np.testing.assert_array_equal(idx2[:, 0], idx[:, 0])
    np.testing.assert_array_equal(_bits(d2[:, 0]), _bits(d[:, 0]))


def _l2int(M, N, D, seed):
    r = np.random.default_rng(seed)
    return r.integers(-8, 9, (M, D)).astype(np.float32), r.integers(-8, 9, (N, D)).astype(np.float32)


@pytest.mark.parametrize("name", ["ham_257x191_d1", "ham_257x191_d61", "l2int_257x191_d3", "l2int_257x191_d129"])
def test_every_split_count_gives_the_same_bits(B, gpu_ctx, name):
    c = EXACT[name]
    m = B.BFMatcher(c["norm"], ctx=gpu_ctx)
    for k in (2, 3, 8):
        want = R.knn_of_distances(R.case_distances(c), k)
        for S in range(1, _tiles(191) + 1):
            _assert_identical(m.knn_match_arrays(c["q"], c["t"], k, splits=S), want, f"{name} k={k} S={S}")


def test_every_split_count_gives_the_same_bits_over_33_tiles(B, gpu_ctx):
    q, t = _l2int(1025, 2049, 5, 1025 + 2049 + 5)
    m = B.BFMatcher(B.NORM_L2, ctx=gpu_ctx)
    want = R.knn(q, t, bf_ref.NORM_L2, 3)
    assert R.tied_rows(bf_ref.distances(q, t, bf_ref.NORM_L2), 3) > 100
    for S in range(1, _tiles(2049) + 1):
        _assert_identical(m.knn_match_arrays(q, t, 3, splits=S), want, f"S={S}")
    _assert_pairs_identical(m.ratio_match_arrays(q, t, 0.75, splits=33), R.ratio_of_knn(*R.knn(q, t, bf_ref.NORM_L2, 2), 0.75), "ratio S=33")


@pytest.mark.parametrize("M,N,D,k", [(2500, 1100, 8, 8), (64, 65536, 4, 8), (65536, 64, 3, 2)])
def test_row_limits_and_more_rows_than_one_compaction_turn(B, gpu_ctx, M, N, D, k):
    """Hamming: 2 500 rows take three compaction turns of the ratio finish; N at the limit with distances of 0..32 only, so ties
    everywhere (1 024 train tiles: the plan's 512 splits and the largest, 1 024); M at the limit (1 024 row tiles on a grid axis)"""
    r = np.random.default_rng(M + N + D)
    q, t = r.integers(0, 256, (M, D), dtype=np.uint8), r.integers(0, 256, (N, D), dtype=np.uint8)
    m = B.BFMatcher(B.NORM_HAMMING, ctx=gpu_ctx)
    d = bf_ref.distances(q, t, bf_ref.NORM_HAMMING)
    want = R.knn_of_distances(d, k)
    for splits in sorted({0, _tiles(N)}):
        _assert_identical(m.knn_match_arrays(q, t, k, splits=splits), want, f"{M}x{N}x{D} k={k} splits={splits}")
    want_r = R.ratio_of_knn(*R.knn_of_distances(d, 2), 0.97)
    assert len(want_r[0]) > (1024 if M > 2000 else 0)
    _assert_pairs_identical(m.ratio_match_arrays(q, t, 0.97), want_r, f"{M}x{N}x{D} ratio")


@pytest.mark.parametrize("k", [2, 3, 4, 8])
def test_unit_rows_give_the_float64_neighbours(B, gpu_ctx, k):
    """l2_unit_case(seed=5).  Where the gaps between the first k + 1 sorted SQUARED float64 distances of a row are >= 6.2e-5 -
    twice the float32 chain's error bound (D + 2) 2^-24 S <= 3.1e-5 of tests/test_bf_gpu.py - the float64 order of the first k
    is the only legal answer.  Up to k = 4 that is every row (asserted); for k = 8 rows with a smaller gap are left out of the
    index comparison, at most 8 of 257 (3 %; a condition on the case, not a measurement: 5 at this seed).  Distances: within
    1e-5 relative (the bound on the squared sum is 7.8e-6 relative and the root halves it)."""
    c = bf_cases.l2_unit_case(seed=5)
    d64 = R.case_distances(c, "f64")
    gap = np.diff(np.sort(d64 ** 2, axis=1)[:, :k + 1], axis=1).min(axis=1)
    sure = gap >= 6.2e-5
    print(f"k = {k}: smallest gap {gap.min():.3g}, rows left out {int((~sure).sum())}")
    if k <= 4:
        assert sure.all()
    assert (~sure).sum() <= 8
    idx64, dist64, cnt64 = R.knn_of_distances(d64, k)
    idx, dist, cnt = B.BFMatcher(B.NORM_L2, ctx=gpu_ctx).knn_match_arrays(c["q"], c["t"], k)
    np.testing.assert_array_equal(cnt, cnt64)
    np.testing.assert_array_equal(idx[sure], idx64[sure])
    err = np.abs(dist.astype(np.float64) - dist64) / dist64
    print(f"max |dist - dist64| / dist64 = {err.max():.3g}")
    assert (np.abs(dist.astype(np.float64) - dist64) <= 1e-5 * dist64).all()


# ---- the device entries ----------------------------------------------------------------------------------------------------
FILL_I, FILL_F = -77, -5.0


def _dev_buffers(ctx, c, M, N, m_dev, n_dev, fill=0):
    q, t = c["q"], c["t"]
    qb, tb = np.full((M, q.shape[1]), fill, q.dtype), np.full((N, q.shape[1]), fill, t.dtype)
    qb[:min(M, len(q))] = q[:M]
    tb[:min(N, len(t))] = t[:N]
    return [ctx.upload(qb), ctx.upload(tb), ctx.upload(np.array([m_dev], np.int32)) if m_dev is not None else None,
            ctx.upload(np.array([n_dev], np.int32)) if n_dev is not None else None]


def _dev_knn(B, ctx, c, k, M, N, m_dev, n_dev, splits=0):
    """sslam_bf_knn_match_dev on buffers of M x N rows with the device counts (None: no count buffer), outputs pre-filled
    -> (idx [M,k], dist [M,k], cnt [M], info [4])"""
    d = _dev_buffers(ctx, c, M, N, m_dev, n_dev)
    o = [ctx.upload(np.full((M, k), FILL_I, np.int32)), ctx.upload(np.full((M, k), FILL_F, np.float32)), ctx.upload(np.full(M, FILL_I, np.int32)),
         ctx.upload(np.full(4, -9, np.int32))]
    try:
        B.BFMatcher(c["norm"]).knn_match_dev(ctx, c["q"].shape[1], d[0], M, d[1], N, k, o[0], o[1], o[2], o[3], m_dev=d[2], n_dev=d[3], splits=splits)
        ctx.sync()
        idx, dist, cnt, info = np.empty((M, k), np.int32), np.empty((M, k), np.float32), np.empty(M, np.int32), np.empty(4, np.int32)
        for h, p in zip((idx, dist, cnt, info), o):
            ctx.d2h(h, p)
    finally:
        for p in d + o:
            if p is not None:
                ctx.free(p)
    return idx, dist, cnt, info


def _dev_ratio(B, ctx, c, ratio, M, N, m_dev, n_dev):
    d = _dev_buffers(ctx, c, M, N, m_dev, n_dev)
    o = [ctx.upload(np.full((M, 2), FILL_I, np.int32)), ctx.upload(np.full(M, FILL_F, np.float32)), ctx.upload(np.full(4, -9, np.int32))]
    try:
        B.BFMatcher(c["norm"]).ratio_match_dev(ctx, c["q"].shape[1], d[0], M, d[1], N, o[0], o[1], o[2], ratio=ratio, m_dev=d[2], n_dev=d[3])
        ctx.sync()
        ij, dist, info = np.empty((M, 2), np.int32), np.empty(M, np.float32), np.empty(4, np.int32)
        for h, p in zip((ij, dist, info), o):
            ctx.d2h(h, p)
    finally:
        for p in d + o:
            if p is not None:
                ctx.free(p)
    K = int(info[0])
    assert 0 <= K <= M and (ij[K:] == FILL_I).all() and (dist[K:] == FILL_F).all()
    return ij[:K], dist[:K], info


@pytest.mark.parametrize("name", ["ham_257x191_d32", "ham_257x191_d61", "l2int_257x191_d128", "l2int_257x191_d3"])
def test_device_entry_with_device_counts_below_the_bounds(B, gpu_ctx, name):
    """(257, 191) buffers, m_dev = 63, n_dev = 65: the result is the restatement's on the sliced arrays; the rows beyond the
    counts are zeros - for integer-valued rows a zero row is close to everything - and are never a neighbour; output rows at and
    beyond m keep the fill value"""
    c = EXACT[name]
    cut = dict(c, q=c["q"].copy(), t=c["t"].copy())
    cut["q"][63:] = 0
    cut["t"][65:] = 0
    for k in (2, 8):
        for splits in (0, 1, 3):
            idx, dist, cnt, info = _dev_knn(B, gpu_ctx, cut, k, 257, 191, 63, 65, splits)
            _assert_identical((idx[:63], dist[:63], cnt[:63]), R.knn(c["q"][:63], c["t"][:65], c["norm"], k), f"{name} k={k} splits={splits}")
            assert (idx[63:] == FILL_I).all() and (dist[63:] == FILL_F).all() and (cnt[63:] == FILL_I).all()
            assert info.tolist() == [63, 65, k, splits or 3] and idx[:63].max() < 65
    ij, dist, info = _dev_ratio(B, gpu_ctx, cut, 0.75, 257, 191, 63, 65)
    want = R.ratio_match(c["q"][:63], c["t"][:65], c["norm"], 0.75)
    _assert_pairs_identical((ij, dist), want, name + " ratio")
    assert info.tolist() == [len(want[0]), 63, 65, 0]


def test_device_entry_without_count_buffers_and_with_counts_above_the_bounds(B, gpu_ctx):
    c = EXACT["ham_63x65_d61"]                                              # (an odd D: the device rows are not word-aligned)
    want = R.knn_of_distances(R.case_distances(c), 3)
    want_r = R.ratio_of_knn(*R.knn_of_distances(R.case_distances(c), 2), 0.8)
    for m_dev, n_dev in ((None, None), (1 << 20, 66)):                      # clamped to the bounds
        idx, dist, cnt, info = _dev_knn(B, gpu_ctx, c, 3, 63, 65, m_dev, n_dev)
        _assert_identical((idx, dist, cnt), want, f"counts {m_dev} {n_dev}")
        assert info.tolist() == [63, 65, 3, 2]
        ij, dist, info = _dev_ratio(B, gpu_ctx, c, 0.8, 63, 65, m_dev, n_dev)
        _assert_pairs_identical((ij, dist), want_r, f"ratio, counts {m_dev} {n_dev}")
        assert info.tolist() == [len(want_r[0]), 63, 65, 0]


@pytest.mark.parametrize("m_dev,n_dev", [(-1, 65), (63, -1), (-5, -5), (0, 65), (63, 0)])
def test_device_entry_with_a_negative_or_zero_count_finds_nothing(B, gpu_ctx, m_dev, n_dev):
    c = EXACT["ham_63x65_d32"]
    m = max(m_dev, 0)
    idx, dist, cnt, info = _dev_knn(B, gpu_ctx, c, 2, 63, 65, m_dev, n_dev)
    assert info.tolist() == [m, max(n_dev, 0), 2, 2]
    assert (cnt[:m] == 0).all() and (idx[:m] == -1).all() and np.isposinf(dist[:m]).all()
    assert (cnt[m:] == FILL_I).all() and (idx[m:] == FILL_I).all() and (dist[m:] == FILL_F).all()
    ij, _dist, info = _dev_ratio(B, gpu_ctx, c, 0.75, 63, 65, m_dev, n_dev)
    assert len(ij) == 0 and info.tolist() == [0, m, max(n_dev, 0), 0]


@pytest.mark.parametrize("name", ["ham_257x191_d61", "ham_257x191_d1", "l2int_257x191_d129", "l2unit"])
def test_the_same_call_three_times_is_bitwise_the_same(B, gpu_ctx, name):
    c = bf_cases.l2_unit_case() if name == "l2unit" else EXACT[name]
    m = B.BFMatcher(c["norm"], ctx=gpu_ctx)
    first, first_r = m.knn_match_arrays(c["q"], c["t"], 8), m.ratio_match_arrays(c["q"], c["t"], 0.9)
    for _ in range(2):
        _assert_identical(m.knn_match_arrays(c["q"], c["t"], 8), first, name)
        _assert_pairs_identical(m.ratio_match_arrays(c["q"], c["t"], 0.9), first_r, name)


# ---- the ratio test --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.7, 0.75, 0.8])
def test_ratio_test_keeps_exactly_the_planted_pairs(B, gpu_ctx, ratio):
    """(the margin |d1 - ratio d2| is >= 10.8 over all rows: tests/test_bf_knn_ref.py)"""
    c = bf_cases.planted_hamming()
    m = B.BFMatcher(B.NORM_HAMMING, ctx=gpu_ctx)
    ij, dist = m.ratio_match_arrays(c["q"], c["t"], ratio)
    np.testing.assert_array_equal(ij, c["planted"])
    _assert_pairs_identical((ij, dist), R.ratio_of_knn(*R.knn_of_distances(R.case_distances(c), 2), ratio), f"planted {ratio}")
    ms = m.ratio_match(c["q"], c["t"], ratio)
    assert [(x.queryIdx, x.trainIdx, x.imgIdx, x.distance) for x in ms] == [(int(i), int(j), 0, float(d)) for (i, j), d in zip(ij, dist)]
    # the Python idiom on knnMatch's DMatch floats
    pairs = m.knnMatch(c["q"], c["t"], k=2)
    assert len(pairs) == len(c["q"]) and all(len(p) == 2 for p in pairs)
    good = [p[0] for p in pairs if p[0].distance < ratio * p[1].distance]
    assert [(x.queryIdx, x.trainIdx, x.distance) for x in good] == [(x.queryIdx, x.trainIdx, x.distance) for x in ms]


@pytest.mark.parametrize("name", L2_EXACT)
def test_ratio_test_on_the_exact_l2_cases_equals_the_restatement(B, gpu_ctx, name):
    """equalities d1 == ratio d2 included (two copies of the query row among the train rows: 0 == 0.75 * 0): dropped"""
    c = EXACT[name]
    idx, dist, cnt = R.knn_of_distances(R.case_distances(c), 2)
    want = R.ratio_of_knn(idx, dist, cnt, 0.75)
    got = B.BFMatcher(B.NORM_L2, ctx=gpu_ctx).ratio_match_arrays(c["q"], c["t"], 0.75)
    _assert_pairs_identical(got, want, name)
    eq = np.nonzero((cnt >= 2) & (dist[:, 0].astype(np.float64) == 0.75 * dist[:, 1].astype(np.float64)))[0]
    assert not set(eq.tolist()) & set(got[0][:, 0].tolist())


def test_knnmatch_lists_compact_result_and_cross_check(B, gpu_ctx):
    c = EXACT["l2_nonfinite_40x50_d16"]
    m = B.BFMatcher(B.NORM_L2, ctx=gpu_ctx)
    idx, dist, cnt = R.knn_of_distances(R.case_distances(c), 3)
    out = m.knnMatch(c["q"], c["t"], 3)
    assert [len(x) for x in out] == cnt.tolist() and out[bf_cases.NONFINITE_QUERY] == []
    assert [[(x.queryIdx, x.trainIdx, x.imgIdx, x.distance) for x in row] for row in out] == \
        [[(i, int(j), 0, float(d)) for j, d in zip(idx[i, :cnt[i]], dist[i, :cnt[i]])] for i in range(len(idx))]
    compact = m.knnMatch(c["q"], c["t"], 3, compactResult=True)
    assert len(compact) == 39 and all(len(x) == 3 for x in compact)
    cc = B.BFMatcher(B.NORM_L2, crossCheck=True, ctx=gpu_ctx)
    ij, d = bf_cases.expected(c, True)
    lists = cc.knnMatch(c["q"], c["t"], 1)
    assert len(lists) == 40 and [(x.queryIdx, x.trainIdx, x.distance) for row in lists for x in row] == [(int(i), int(j), float(v)) for (i, j), v in zip(ij, d)]
    assert all(len(row) <= 1 for row in lists)


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


def test_device_ratio_match_chains_into_the_device_ransac_filter(B, gpu_ctx):
    """sslam_bf_ratio_match_dev -> sslam_fmat_ransac_dev on the pairs and the count it left on the device, nothing read back in
    between: the kept pairs are those of the host route (ratio_match_arrays, gather the pixels, sslam_fmat_ransac_host)."""
    E = load_pkg("epipolar")
    ctx = gpu_ctx
    c, kp1, kp2 = _planted_scene()
    M, N, D = len(c["q"]), len(c["t"]), c["q"].shape[1]
    ij_h, _ = B.BFMatcher(B.NORM_HAMMING, ctx=ctx).ratio_match_arrays(c["q"], c["t"], 0.75)
    assert len(ij_h) == 200
    _F, mask, meta = E.find_fundamental_ransac(kp1[ij_h[:, 0]], kp2[ij_h[:, 1]], 3.0, 0.99, ctx=ctx)
    assert mask is not None and 120 <= mask.sum() < len(ij_h)
    want = ij_h[mask]

    d = [ctx.upload(a) for a in (c["q"], c["t"], kp1, kp2)]
    d_ij, d_dist, d_info = ctx.malloc(M * 8), ctx.malloc(M * 4), ctx.malloc(16)
    d_kept, d_finfo = ctx.upload(np.full((M, 2), -1, np.int32)), ctx.malloc(16)
    try:
        B.BFMatcher(B.NORM_HAMMING).ratio_match_dev(ctx, D, d[0], M, d[1], N, d_ij, d_dist, d_info, ratio=0.75)
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
