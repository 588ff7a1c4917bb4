"""The F-matrix filter (csrc/ransac_kernels.hip) at the constants it switches on, against the restated
cv2.findFundamentalMat (oracle/ransac_ref.py): the sample loop's chunk bounds [0,8) [8,128) [128,max_iters), the
RS_LDS_POINTS = 4096 switch of the sampler / gather, the 1024-match turns of the tail's compaction, the solver's
1- and 3-root branches, and one scratch slab driven big, then small.

Comparison as in test_ransac_gpu._check (same `sample`, `iterations`, `lmeds`, identical mask, F within 1e-7 of its
scale); the device entry must equal the host entry bit for bit.  Every scene built to reach a branch first asserts on
the oracle, on the CPU, that it does.

The compaction patterns: "inliers only past the first 1024" needs >= 7 inliers there (a RANSAC winner always has its
own 7 sample points), so it exists from n = 1024 + 7 on; below that the same pattern is run at the half-way mark, which
still empties the low lanes of the turn."""
import numpy as np
import pytest

import two_view
from conftest import load_pkg
from oracle import ransac_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    return load_pkg("epipolar")


def _check(E, p1, p2, thresh=1.0, conf=0.99, max_iters=1000, oracle_iters=None, ctx=None):
    """test_ransac_gpu._check with max_iters / ctx; returns (F, mask, info) of the GPU and the oracle's info."""
    F, mask, info = E.find_fundamental_ransac(p1, p2, thresh, conf, max_iters, ctx=ctx)
    Fr, mr, ir = R.find_fundamental_ransac(p1, p2, thresh, conf, max_iters if oracle_iters is None else oracle_iters)
    assert (F is None) == (Fr is None)
    assert info["lmeds"] == ir["lmeds"]
    if F is None:
        assert mask is None and mr is None
        return F, mask, info, ir
    assert info["sample"] == ir["sample"] and info["iterations"] == ir["iterations"]
    np.testing.assert_array_equal(mask, mr)
    assert info["inliers"] == int(mr.sum())
    s = np.abs(Fr).max()
    np.testing.assert_allclose(F / s, Fr / s, atol=1e-7)
    return F, mask, info, ir


def _scatter(p1, p2, seed):
    """The matched points as a matcher would index them: two keypoint arrays and the index pairs into them."""
    n = len(p1)
    rng = np.random.default_rng(1000 + seed)
    n1, n2 = n + 50, n + 80
    q, t = rng.permutation(n1)[:n], rng.permutation(n2)[:n]
    kp1 = rng.uniform(0, 1000, (n1, 2)).astype(np.float32); kp1[q] = p1
    kp2 = rng.uniform(0, 1000, (n2, 2)).astype(np.float32); kp2[t] = p2
    return kp1, kp2, np.stack([q, t], 1).astype(np.int32)


def _dev_filter(E, ctx, kp1, kp2, ij, n_max, n_dev, max_iters=1000):
    """sslam_fmat_ransac_dev on a pair buffer of n_max entries (ij, zero padded) with the device count n_dev (taken as
    it is: the kernel clamps it).  Returns (kept pairs, info[4], mask[n_max], F[3,3])."""
    buf = np.zeros((n_max, 2), np.int32)
    m = min(n_max, len(ij))
    buf[:m] = ij[:m]
    d = [ctx.upload(np.ascontiguousarray(a)) for a in (kp1, kp2, buf, np.array([n_dev], np.int32))]
    out_ij, mask = ctx.upload(np.full((n_max, 2), -1, np.int32)), ctx.upload(np.zeros(n_max, np.uint8))
    info, F = ctx.malloc(16), ctx.malloc(72)
    E.filter_matches_dev(ctx, n_max, d[3], d[0], d[1], d[2], out_ij, info, max_iters=max_iters, mask_out_dev=mask, F_out_dev=F)
    h_ij, h_info = np.empty((n_max, 2), np.int32), np.empty(4, np.int32)
    h_mask, h_F = np.empty(n_max, np.uint8), np.empty(9)
    ctx.d2h(h_ij, out_ij); ctx.d2h(h_info, info); ctx.d2h(h_mask, mask); ctx.d2h(h_F, F)
    for p in d + [out_ij, info, mask, F]:
        ctx.free(p)
    assert 0 <= h_info[0] <= n_max
    assert (h_ij[h_info[0]:] == -1).all()                      # nothing written past the kept pairs
    return h_ij[:h_info[0]], h_info, h_mask.astype(bool), h_F.reshape(3, 3)


def _both_entries(E, ctx, p1, p2, seed, max_iters=1000, oracle_iters=None, n_max=None):
    """Host entry against the oracle, device entry bit-equal to the host entry.  Returns the oracle's info."""
    n = len(p1)
    F_h, mask_h, info_h, ir = _check(E, p1, p2, max_iters=max_iters, oracle_iters=oracle_iters, ctx=ctx)
    assert mask_h is not None
    kp1, kp2, ij = _scatter(p1, p2, seed)
    kept, info, mask, F = _dev_filter(E, ctx, kp1, kp2, ij, n_max or n, n, max_iters)
    np.testing.assert_array_equal(mask[:n], mask_h)
    assert not mask[n:].any()                                  # the mask beyond the device count is not written
    np.testing.assert_array_equal(kept, ij[mask_h])
    assert info[0] == mask_h.sum() and info[1] == info_h["iterations"] and info[3] == info_h["sample"]
    assert bool(info[2]) == info_h["lmeds"]
    np.testing.assert_array_equal(F, F_h)
    return ir


# ---- the loop ends inside chunk 0: the path every SLAM frame takes (chunk 0 decides, four early-exit launches) ----------
CHUNK0 = [(600, 0.02, 0.05, 0, 5), (600, 0.02, 0.05, 1, 2), (600, 0.02, 0.05, 2, 3), (600, 0.02, 0.05, 3, 3),
          (2048, 0.03, 0.1, 0, 4), (2048, 0.03, 0.1, 1, 5), (2048, 0.03, 0.1, 2, 5), (2048, 0.03, 0.1, 3, 3),
          (4096, 0.02, 0.1, 3, 8)]


@pytest.mark.parametrize("n,frac,noise,seed,iters", CHUNK0, ids=[f"chunk0-n{c[0]}-s{c[3]}-it{c[4]}" for c in CHUNK0])
def test_loop_ends_in_chunk_zero(E, gpu_ctx, n, frac, noise, seed, iters):
    p1, p2, _ = two_view.make_matches(n, outlier_frac=frac, noise=noise, seed=seed)
    _, _, ir = R.find_fundamental_ransac(p1, p2, 1.0, 0.99)
    assert ir["iterations"] == iters <= 8                       # the scene reaches the branch it is named for
    if n == 4096:
        assert ir["sample"] == 6                                # ends exactly on the chunk bound, at exactly RS_LDS_POINTS
    _both_entries(E, gpu_ctx, p1, p2, seed)


# ---- max_iters: degenerate chunk bounds {0, min(8,M), min(128,M), M} -----------------------------------------------
MAXIT = [(1, 0), (7, 5), (8, 5), (9, 5), (128, 87), (129, 87), (500, None)]


@pytest.mark.parametrize("max_iters,winner", MAXIT, ids=[f"maxiters-{m}" for m, _ in MAXIT])
def test_max_iters_edges(E, gpu_ctx, max_iters, winner):
    p1, p2, _ = two_view.make_matches(300, outlier_frac=0.6, noise=0.3, seed=0)
    _, mr, ir = R.find_fundamental_ransac(p1, p2, 1.0, 0.99, max_iters)
    assert mr is not None and ir["iterations"] == max_iters     # the budget never drops below the cap on this scene
    if winner is not None:
        assert ir["sample"] == winner
    _both_entries(E, gpu_ctx, p1, p2, 0, max_iters=max_iters)


@pytest.mark.parametrize("max_iters", [0, 5000], ids=["maxiters-0-defaults", "maxiters-5000-defaults"])
def test_max_iters_out_of_range_defaults_to_1000(E, gpu_ctx, max_iters):
    p1, p2, _ = two_view.make_matches(300, outlier_frac=0.6, noise=0.3, seed=0)
    ir = _both_entries(E, gpu_ctx, p1, p2, 0, max_iters=max_iters, oracle_iters=1000)
    assert ir["iterations"] > 500                               # (beyond every explicit cap above: the default was applied)


# ---- RS_LDS_POINTS ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097], ids=lambda n: f"lds-{n}")
def test_lds_threshold_host_entry(E, gpu_ctx, n):
    p1, p2, _ = two_view.make_matches(n, outlier_frac=0.3, noise=0.3, seed=n)
    _, _, _, ir = _check(E, p1, p2, ctx=gpu_ctx)
    assert ir["iterations"] > 8                                 # the sampler runs again after chunk 0 (rs_step_kernel's copy)


LDS_DEV = [(4096, 4096), (4097, 4096), (4097, 4097), (8192, 15), (8192, 14), (4097, 7)]


@pytest.mark.parametrize("n_max,n_dev", LDS_DEV, ids=[f"lds-nmax{a}-ndev{b}" for a, b in LDS_DEV])
def test_lds_threshold_device_entry(E, gpu_ctx, n_max, n_dev):
    """n_max decides the launch shape (fused or separate gather), the device count the sampler's memory space."""
    p1, p2, _ = two_view.make_matches(n_dev, outlier_frac=0.3 if n_dev > 100 else 0.15, noise=0.3, seed=n_dev)
    kp1, kp2, ij = _scatter(p1, p2, n_dev)
    if n_dev < 8:                                               # pass-through under the separate-gather launch shape
        kept, info, mask, F = _dev_filter(E, gpu_ctx, kp1, kp2, ij, n_max, n_dev)
        assert not mask[n_dev:].any()                           # the mask beyond the device count is not written
        assert info[0] == n_dev and info[3] == -2 and mask[:n_dev].all() and not F.any()
        np.testing.assert_array_equal(kept, ij)
        return
    ir = _both_entries(E, gpu_ctx, p1, p2, n_dev, n_max=n_max)
    assert ir["lmeds"] == (n_dev <= 14)


@pytest.mark.parametrize("n_dev,same_as", [(3000, 600), (-5, 0)], ids=["ndev-above-nmax", "ndev-negative"])
def test_device_count_is_clamped(E, gpu_ctx, n_dev, same_as):
    """rs_n clamps the device count to [0, n_max]: a count above the bound gives what the bound gives, a negative one
    what 0 gives."""
    p1, p2, _ = two_view.make_matches(600, outlier_frac=0.3, noise=0.3, seed=21)
    kp1, kp2, ij = _scatter(p1, p2, 21)
    got = _dev_filter(E, gpu_ctx, kp1, kp2, ij, 600, n_dev)
    want = _dev_filter(E, gpu_ctx, kp1, kp2, ij, 600, same_as)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    if same_as == 0:
        assert got[1][0] == 0 and got[1][3] == -2
    else:
        _, mask_h, _, _ = _check(E, p1, p2, ctx=gpu_ctx)
        np.testing.assert_array_equal(got[0], ij[mask_h])


# ---- the tail's compaction, 1024 matches per turn --------------------------------------------------------------------
def _patterned(n, pattern, seed=0):
    """A two-view scene whose inliers sit exactly where `pattern` says: exact correspondences (float32 rounding only),
    every other match pushed 30 - 80 px off its epipolar line."""
    p1, p2, _ = two_view.make_matches(n, outlier_frac=0.0, noise=0.0, seed=seed)
    want = np.ones(n, bool)
    if pattern == "head":                                      # inliers only in the first 1024 (n <= 1024: the first half)
        want[(1024 if n > 1024 else n // 2):] = False
    elif pattern == "tail":                                    # inliers only past the first 1024 (n < 1031: the second half)
        want[:(1024 if n >= 1031 else n // 2)] = False
    rng = np.random.default_rng(seed + 77)
    e2 = two_view.K @ two_view.T_VIEW; e2 = e2[:2] / e2[2]                    # epipole of image 2
    out = np.flatnonzero(~want)
    radial = p2[out] - e2
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    perp = np.stack([-radial[:, 1], radial[:, 0]], 1)
    p2[out] += (perp * (rng.uniform(30, 80, len(out)) * rng.choice([-1.0, 1.0], len(out)))[:, None]).astype(np.float32)
    return p1, p2, want


COMPACT = [(n, pat) for n in (1023, 1024, 1025, 2049) for pat in ("all", "head", "tail")]


@pytest.mark.parametrize("n,pattern", COMPACT, ids=[f"compact-{n}-{p}" for n, p in COMPACT])
def test_compaction_turns(E, gpu_ctx, n, pattern):
    p1, p2, want = _patterned(n, pattern)
    _, mr, ir = R.find_fundamental_ransac(p1, p2, 1.0, 0.99)
    assert mr is not None
    np.testing.assert_array_equal(mr, want)                     # the oracle's mask IS the pattern: the turn is full / empty
    kp1, kp2, ij = _scatter(p1, p2, n)
    kept, info, mask, _ = _dev_filter(E, gpu_ctx, kp1, kp2, ij, n, n)
    np.testing.assert_array_equal(mask, mr)
    np.testing.assert_array_equal(kept, ij[mr])                 # the kept pairs, in order
    assert info[0] == int(mr.sum()) and info[1] == ir["iterations"] and info[3] == ir["sample"]
    _check(E, p1, p2, ctx=gpu_ctx)


# ---- planar scene, the solver's root counts --------------------------------------------------------------------------
def _root_counts(p1, p2, iterations):
    """How many of the samples the loop examined gave 1, 2, 3 models (oracle's run7point on the replayed sample stream)."""
    rng = R.CvRNG()
    hist = {0: 0, 1: 0, 2: 0, 3: 0}
    for _ in range(iterations):
        idx = R.get_subset(p1, p2, rng)
        hist[len(R.run7point(p1[idx], p2[idx]))] += 1
    return hist


@pytest.mark.parametrize("n,seed,iters,winner", [(500, 1, 65, 16), (1500, 2, None, None)], ids=["planar-500", "planar-1500"])
def test_planar_scene_and_solver_branches(E, gpu_ctx, n, seed, iters, winner):
    p1, p2, _ = two_view.make_matches(n, outlier_frac=0.3, noise=0.3, seed=seed, planar=True)
    _, mr, ir = R.find_fundamental_ransac(p1, p2, 1.0, 0.99)
    assert mr is not None
    if iters is not None:
        assert (ir["iterations"], ir["sample"]) == (iters, winner)
    hist = _root_counts(p1, p2, ir["iterations"])
    assert hist[1] > 0 and hist[3] > 0, hist                    # both branches of the cubic among the examined samples
    _both_entries(E, gpu_ctx, p1, p2, seed)


# ---- one slab, big then small ----------------------------------------------------------------------------------------
def test_slab_reuse_big_then_small(E, native, gpu_ctx):
    """Stale counts / nmodels / medians of a larger earlier call in the reused scratch slab must not leak into a smaller
    later one: each call equals its own result from a fresh context, the first and the last are bit-identical."""
    scenes = [two_view.make_matches(5000, outlier_frac=0.3, noise=0.3, seed=5),
              two_view.make_matches(600, outlier_frac=0.65, noise=0.3, seed=7),
              two_view.make_matches(600, outlier_frac=0.02, noise=0.05, seed=0),
              two_view.make_matches(14, outlier_frac=0.15, noise=0.2, seed=2)]
    want_iters = [142, 1000, 5, None]
    for (p1, p2, _), it in zip(scenes, want_iters):
        _, _, ir = R.find_fundamental_ransac(p1, p2, 1.0, 0.99)
        assert it is None or ir["iterations"] == it
        assert ir["lmeds"] == (len(p1) == 14)
    scenes.append(scenes[0])
    shared = native.Context(0)
    try:
        got = []
        for k, (p1, p2, _) in enumerate(scenes):
            F, mask, info, _ = _check(E, p1, p2, ctx=shared)
            kp1, kp2, ij = _scatter(p1, p2, k)
            dev = _dev_filter(E, shared, kp1, kp2, ij, len(p1), len(p1))
            got.append((F, mask, info, dev))
            fresh = native.Context(0)
            try:
                F_f, mask_f, info_f = E.find_fundamental_ransac(p1, p2, 1.0, 0.99, ctx=fresh)
                dev_f = _dev_filter(E, fresh, kp1, kp2, ij, len(p1), len(p1))
            finally:
                fresh.close()
            np.testing.assert_array_equal(F, F_f)
            np.testing.assert_array_equal(mask, mask_f)
            assert info == info_f
            for a, b in zip(dev, dev_f):
                np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(got[0][0], got[-1][0])
        np.testing.assert_array_equal(got[0][1], got[-1][1])
        assert got[0][2] == got[-1][2]
    finally:
        shared.close()
