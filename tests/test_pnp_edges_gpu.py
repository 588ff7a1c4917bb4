"""csrc/pnp_kernels.hip at the places where it decides, against oracle/pnp_ref.py on the cases of tests/pnp_cases.py
(tests/test_pnp_cases.py shows on the restatement alone that each case reaches its branch): every sample's EPnP through
the n == 5 branch, the sample loop at the chunk bounds, the strides of the score / LM / tail / head loops and the LM's LDS
limit, the LM's exits and the closed threshold."""
import numpy as np
import pytest

import pnp_cases as C
import pnp_scenes as S
from conftest import load_pkg
from oracle import pnp_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    n = load_pkg("_native")
    if n.device_count() < 1:
        pytest.skip("needs an MI355X")
    return n


@pytest.fixture(scope="module")
def PN(native):
    return load_pkg("pnp")


def _host(PN, c, use_guess):
    return PN.solve_pnp_ransac(c["pts3d"], c["pts2d"], c["K"], c["px"], C.CONF, c["iters"], use_guess=use_guess)


SENTINEL = 0xA5


def _dev(native, PN, kop, xyz, kp, K, px, iters, use_guess):
    """The device entry on an association; the mask buffer is pre-filled, so a write past n_out shows."""
    ctx = native.default_context()
    Q = len(kop)
    d_kop, d_xyz, d_kp = ctx.upload(kop.astype(np.int32)), ctx.upload(xyz.astype(np.float64)), ctx.upload(kp.astype(np.float32))
    d_mask = ctx.upload(np.full(Q + 64, SENTINEL, np.uint8))
    d_T, d_info, d_n = ctx.malloc(128), ctx.malloc(16), ctx.malloc(4)
    PN.solve_pnp_ransac_dev(ctx, Q, d_kop, d_xyz, d_kp, K, d_T, d_info, px, C.CONF, iters, use_guess=use_guess,
                            mask_out_dev=d_mask, n_out_dev=d_n)
    ctx.sync()
    T, info, mask, n = np.empty(16), np.empty(4, np.int32), np.empty(Q + 64, np.uint8), np.empty(1, np.int32)
    for h, d in ((T, d_T), (info, d_info), (mask, d_mask), (n, d_n)):
        ctx.d2h(h, d)
    for d in (d_kop, d_xyz, d_kp, d_T, d_info, d_mask, d_n):
        ctx.free(d)
    n = int(n[0])
    assert (mask[n:] == SENTINEL).all(), "the device entry wrote past n_out in the mask"
    assert np.isin(mask[:n], (0, 1)).all()
    return T.reshape(4, 4), [int(v) for v in info], mask[:n].astype(bool), n


def _dev_equals_host(native, PN, c, use_guess, host):
    """The device entry on the case's correspondences (every slot associated, keypoints in order) - the host entry's
    result bit for bit."""
    n = len(c["pts3d"])
    T, info, mask, n_out = _dev(native, PN, np.arange(n), c["pts3d"], c["pts2d"], c["K"], c["px"], c["iters"], use_guess)
    ok, Th, mh, ih = host
    assert n_out == n
    assert info == [ih["inliers"], ih["samples"], ih["sample"], ih["lm_iters"]]
    assert np.array_equal(mask, mh)
    assert T.tobytes() == (Th if ok else np.eye(4)).tobytes()


def _compare(PN, name, use_guess, exact_points=()):
    """tests/test_pnp_gpu.py's comparison on a cached case: ok, samples, sample, inliers; the mask except where the winner's
    restated error lies within 1e-5 relative of the threshold (at most one point, never one of `exact_points`); the pose
    within 1e-6."""
    c, r = C.case(name), C.restated(name, use_guess)
    host = _host(PN, c, use_guess)
    gok, T, gmask, ginfo = host
    print(name, use_guess, "gpu", ginfo, "restated", r.info)
    assert gok == r.ok
    assert (ginfo["samples"], ginfo["sample"]) == (r.info["samples"], r.info["sample"])
    if not r.ok:
        assert T is None and not gmask.any() and ginfo["inliers"] == -1 and ginfo["lm_iters"] == 0
        return host, r
    t2 = np.float32(float(np.float32(c["px"])) ** 2)
    near = np.abs(r.err.astype(np.float64) - t2) <= 1e-5 * t2
    near[list(exact_points)] = False
    assert near.sum() <= 1
    np.testing.assert_array_equal(gmask[~near], r.mask[~near])
    assert ginfo["inliers"] == int(gmask.sum())
    if not near.any():
        assert ginfo["inliers"] == r.info["inliers"]
    if np.isfinite(r.rvec).all():
        Tr = O.pose_matrix(r.rvec, r.tvec)
        rot, tr = S.rot_err_rad(T[:3, :3], Tr[:3, :3]), np.linalg.norm(T[:3, 3] - Tr[:3, 3]) / (1 + np.linalg.norm(Tr[:3, 3]))
        print(f"  pose: rotation {rot:.3g} rad, translation {tr:.3g} relative; lm_iters {ginfo['lm_iters']} / {r.info['lm_iters']}")
        assert rot < 1e-6 and tr < 1e-6
    return host, r


# ---- A: every sample's EPnP ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_every_subsets_epnp(PN, name):
    """Each five-point subset of the family as its own n == 5 call (one EPnP on the points in order, no scoring, no LM)
    against O.epnp_model: rotation within 1e-9 rad, translation within 1e-9 (1 + |t|); NaN where the restatement is NaN,
    with the last row 0 0 0 1.  Subsets whose restated rotation angle exceeds pi - 1e-3 are left out (none in these
    families).  Measured maxima on the MI355X, rotation rad / relative translation: rand60 4.5e-16 / 0, kitti60 4.0e-16 / 0,
    clean60 5.2e-17 / 0, duplicate 0 / 0 (the rotation figures are the rounding of the comparison itself); coplanar 9 of 9,
    collinear 6 of 8 and identical 2 of 2 subsets NaN on both sides, the two finite lines 0 / 0."""
    subs, K = C.family(name)
    worst_r = worst_t = 0.0
    n_nan = 0
    for k, ((p3, p2), (r, t, tr)) in enumerate(zip(subs, C.family_restated(name))):
        ok, T, mask, info = PN.solve_pnp_ransac(p3, p2, K, C.PX, C.CONF, S.ITERS, use_guess=bool(k & 1))
        assert ok and mask.all() and info == {"inliers": 5, "samples": 0, "sample": -1, "lm_iters": 0}, (k, info)
        assert np.array_equal(T[3], [0, 0, 0, 1]), k
        if tr["nan_model"]:
            assert np.isnan(T[:3]).all(), (k, T)
            n_nan += 1
            continue
        if C.beyond_angle_bar(r):
            continue
        Tr = O.pose_matrix(r, t)
        er = S.rot_err_rad(T[:3, :3], Tr[:3, :3])
        et = np.linalg.norm(T[:3, 3] - t) / (1 + np.linalg.norm(t))
        worst_r, worst_t = max(worst_r, er), max(worst_t, et)
        assert er < 1e-9 and et < 1e-9, (name, k, er, et, tr)
    print(f"{name}: {len(subs)} subsets, {n_nan} NaN, max rotation {worst_r:.3g} rad, max translation {worst_t:.3g} relative")


# ---- B: the sample loop at its chunk bounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_guess", [False, True])
@pytest.mark.parametrize("name", list(C.LOOP_CASES))
def test_loop_case(native, PN, name, use_guess):
    """Planted winners at h in {0, 7, 8, 63, 64} (budget 100 / 300 and h + 1), max_iters in {0, 1, 7, 8, 9, 63, 64, 65},
    the budget landing on 7 / 8 / 9 / 63 / 64 / 65, no sample above 4 inliers, a winner with exactly 5, n = 6: host entry
    against the restatement, device entry against the host entry bit for bit.  Measured on the MI355X: the largest pose
    deviation 4.2e-10 rad / 8.7e-12 relative (planted_h7_full with a guess), every other case below 1e-13."""
    host, _ = _compare(PN, name, use_guess)
    _dev_equals_host(native, PN, C.case(name), use_guess, host)


# ---- C: sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_guess", [False, True])
@pytest.mark.parametrize("n", C.SIZES)
def test_host_size(PN, n, use_guess):
    """n on and next to the strides 64 (score), 256 (LM sums), 1024 (tail mask) and the LM's LDS limit 3072.  Measured on
    the MI355X: pose deviations up to 1.0e-12 rad / 5.0e-12 relative, `lm_iters` equal in all 22 cases with a pose."""
    _compare(PN, f"n{n}", use_guess)


@pytest.mark.parametrize("q,pattern", C.DEV_CASES)
def test_device_association(native, PN, q, pattern):
    """The head's compaction at n_points on and next to its stride of 1024: the device entry equals the host entry on the
    compacted correspondences bit for bit, and writes nothing past n_out in the mask."""
    kop, xyz, kp, sc = C.association(q, pattern)
    m = len(sc["pts3d"])
    for use_guess in (False, True):
        T, info, mask, n_out = _dev(native, PN, kop, xyz, kp, sc["K"], C.PX, S.ITERS, use_guess)
        assert n_out == m
        if m < 5:
            assert info[0] == -1 and np.array_equal(T, np.eye(4)) and not mask.any()
            continue
        ok, Th, mh, ih = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], C.PX, C.CONF, S.ITERS, use_guess=use_guess)
        assert ok and ih["inliers"] >= 5
        assert info == [ih["inliers"], ih["samples"], ih["sample"], ih["lm_iters"]]
        assert T.tobytes() == Th.tobytes() and np.array_equal(mask, mh)


# ---- D: the LM ---------------------------------------------------------------------------------------------------------------------
def test_guess_with_degenerate_last_sample(native, PN):
    """The loop's last sample is coplanar in the world (NaN model): with a guess the LM starts there, runs its 20
    iterations and returns a NaN pose with ok, as restated; without a guess the pose is finite; the next call is served."""
    c = C.case("degenerate_last")
    host, r = _compare(PN, "degenerate_last", True)
    ok, T, mask, info = host
    assert ok and np.isnan(r.rvec).all() and np.isnan(T[:3]).all() and np.array_equal(T[3], [0, 0, 0, 1])
    assert info["lm_iters"] == r.info["lm_iters"] == 20
    _dev_equals_host(native, PN, c, True, host)
    host, r = _compare(PN, "degenerate_last", False)
    assert np.isfinite(host[1]).all()
    _compare(PN, "planted_h7_last", True)


@pytest.mark.parametrize("name", list(C.LM_PINNED))
def test_lm_iters_where_every_decision_has_a_margin(native, PN, name):
    """Scenes whose every accept / reject decision and stop test has a traced relative margin >= 1e-9 (the kernel's other
    summation order moves the compared numbers by < 1e-12): the same number of LM iterations, at the 20-iteration cap and
    on the small step, with and without a guess."""
    _, _, _, guess, _ = C.LM_PINNED[name]
    host, r = _compare(PN, name, guess)
    assert host[3]["lm_iters"] == r.info["lm_iters"]
    _dev_equals_host(native, PN, C.case(name), guess, host)


@pytest.mark.parametrize("name", list(C.LM_K_CAP))
def test_lm_with_lambda_at_its_cap(PN, name):
    """k climbs to 16 (noise-free, with a guess); the decisions up there are rounding, so only the pose is compared."""
    _compare(PN, name, C.LM_K_CAP[name][3])


# ---- E: the threshold is closed ------------------------------------------------------------------------------------------------------
def test_threshold_is_closed(PN):
    """The winner's float32 error of one point equals the float32 threshold: in the mask at that threshold, out of it at the
    next float32 below - with no near-threshold exemption for that point."""
    i = C.THRESHOLD_POINT
    (_, _, m_at, _), _ = _compare(PN, "threshold_at", False, exact_points=(i,))
    (_, _, m_below, _), _ = _compare(PN, "threshold_below", False, exact_points=(i,))
    assert m_at[i] and not m_below[i]
