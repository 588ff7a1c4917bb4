"""`sslam_triangulate_2view_host` / `_dev` against the numpy reference (tests/triangulate_ref.py) on every scene of
tests/triangulate_scenes.py.

Verdicts (kept indices, reason per match) must be IDENTICAL.  That can only be asked when no match sits on a threshold, so
each test first asserts on the reference's diagnostics alone that every match clears every gate by a margin far above any
rounding difference: 1e-6 degrees of parallax, 1e-6 relative for each depth against the window bounds and the 1e-6 front
test, 1e-6 px for each reprojection error (all matches of all scenes, not a subset).

Positions: the tolerance is measured, not guessed.  `JACOBI_VS_LAPACK` is the largest relative disagreement, over the kept
points of all scenes, between the reference with LAPACK's SVD and the same reference with the float64 numpy port of the
one-sided Jacobi the kernel runs - two correct evaluations of the same arithmetic: 3.4e-13 (measured on the build machine;
`test_the_measured_floor_still_holds` re-measures it on the CPU part of every GPU run).  The GPU may differ from the
reference by 100 x that (it reorders and fuses operations): 3.4e-11 relative, and in no case more than 1e-6 (60 um at this
scene's far depth).
"""
import numpy as np
import pytest

import triangulate_ref as R
import triangulate_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SCENES = S.all_scenes()
JACOBI_VS_LAPACK = 3.4e-13
X_BAR = 100 * JACOBI_VS_LAPACK
assert X_BAR <= 1e-6


@pytest.fixture(scope="module")
def tri():
    return load_pkg("triangulation")


def _rel(X, Xref):
    return float((np.linalg.norm(X - Xref, axis=1) / np.linalg.norm(Xref, axis=1)).max()) if len(Xref) else 0.0


def assert_margins(diag, reason, P):
    """every match clears every gate, on the reference's own diagnostics (a match whose w is invalid has none)"""
    if P["use_parallax_gate"] and len(reason):
        assert np.abs(diag["parallax_deg"] - P["parallax_min_deg"]).min() > 1e-6
    ok = reason != R.INVALID_W
    for z in (diag["z1"][ok], diag["z2"][ok]):
        for bound in (P["min_depth"], P["max_depth"], 1e-6):
            assert (np.abs(z - bound) > 1e-6 * abs(bound)).all()
    for e in (diag["e1"][ok], diag["e2"][ok]):
        assert (np.abs(e - P["reproj_px_max"]) > 1e-6).all()
    w = np.abs(diag["w"])
    assert ((w < 1e-13) | (w > 1e-11)).all()                 # the |w| > 1e-12 test, a decade either side


def test_the_measured_floor_still_holds():
    worst = 0.0
    for s in SCENES.values():
        Xl, il, rl, _ = R.triangulate_2view(s["pts1"], s["pts2"], s["K"], s["T1"], s["T2"], svd="lapack", **s["params"])
        Xj, ij, rj, _ = R.triangulate_2view(s["pts1"], s["pts2"], s["K"], s["T1"], s["T2"], svd="jacobi", **s["params"])
        np.testing.assert_array_equal(rl, rj)
        worst = max(worst, _rel(Xj, Xl))
    print(f"LAPACK against the Jacobi port, all scenes: {worst:.3e}")
    assert worst <= JACOBI_VS_LAPACK


@pytest.mark.parametrize("name", list(SCENES))
def test_host_entry_equals_the_reference(tri, gpu_ctx, name):
    s = SCENES[name]
    P = s["params"]
    Xr, ir, rr, dr = R.triangulate_2view(s["pts1"], s["pts2"], s["K"], s["T1"], s["T2"], **P)
    assert_margins(dr, rr, P)
    np.testing.assert_array_equal(rr, s["reason"])
    X, idx, reasons, diag = tri.triangulate_2view(s["pts1"], s["pts2"], s["K"], s["T1"], s["T2"], want_diag=True, ctx=gpu_ctx, **P)
    rel = _rel(X, Xr) if np.array_equal(idx, ir) else float("nan")
    print(f"{name}: kept {len(idx)} / {len(rr)}, reasons {reasons}, positions rel {rel:.3e} (bar {X_BAR:.1e})")
    np.testing.assert_array_equal(diag["reason"], rr)
    np.testing.assert_array_equal(idx, ir)
    assert reasons == {k: int((rr == c).sum()) for c, k in enumerate(R.REASONS)}
    assert X.shape == Xr.shape and rel <= X_BAR
    # the diagnostics the drop-in logs from: the reference's values where it has any
    ok = rr != R.INVALID_W
    if P["use_parallax_gate"]:
        # a rounding of the cosine (a few eps) moves the angle by that over sin(angle), and by sqrt(that) where it clips to 1
        eps8 = 8 * np.finfo(np.float64).eps
        tol = np.degrees(eps8 / np.maximum(np.sin(np.radians(dr["parallax_deg"])), np.sqrt(eps8))) + 1e-10
        assert (np.abs(diag["parallax_deg"] - dr["parallax_deg"]) <= tol).all()
    front = ok & (dr["z1"] > 1e-6) & (dr["z2"] > 1e-6) & (rr != R.LOW_PARALLAX)
    np.testing.assert_allclose(diag["z1"][front], dr["z1"][front], rtol=1e-6)
    np.testing.assert_allclose(diag["e1"][front], dr["e1"][front], rtol=0, atol=1e-5)
    np.testing.assert_allclose(diag["e2"][front], dr["e2"][front], rtol=0, atol=1e-5)
    # without the diagnostics buffer: the same result
    X2, idx2, reasons2, none = tri.triangulate_2view(s["pts1"], s["pts2"], s["K"], s["T1"], s["T2"], ctx=gpu_ctx, **P)
    assert none is None and reasons2 == reasons and np.array_equal(idx2, idx) and X2.tobytes() == X.tobytes()


def _dev_run(tri, ctx, s, ij, n_dev_value, n_max, with_diag=True):
    """upload keypoints / pairs / poses, run the device entry, read everything back"""
    kp1, kp2 = s["kp1"], s["kp2"]
    bufs = [ctx.upload(a) for a in (kp1, kp2, np.ascontiguousarray(ij, np.int32), np.array([n_dev_value], np.int32),
                                    np.ascontiguousarray(s["T1"], np.float64), np.ascontiguousarray(s["T2"], np.float64))]
    d_kp1, d_kp2, d_ij, d_n, d_T1, d_T2 = bufs
    outs = [ctx.malloc(n_max * 24), ctx.malloc(n_max * 8), ctx.malloc(32), ctx.malloc(n_max * 4), ctx.malloc(n_max * 40)]
    d_X, d_ijo, d_info, d_reason, d_diag = outs
    try:
        tri.triangulate_2view_dev(ctx, n_max, d_n, d_kp1, d_kp2, d_ij, s["K"], d_T1, d_T2, d_X, d_ijo, d_info,
                                  reason_out_dev=d_reason if with_diag else None, diag_out_dev=d_diag if with_diag else None,
                                  **s["params"])
        ctx.sync()
        info = np.empty(8, np.int32); ctx.d2h(info, d_info)
        X = np.empty((n_max, 3)); ctx.d2h(X, d_X)
        ijo = np.empty((n_max, 2), np.int32); ctx.d2h(ijo, d_ijo)
        reason = np.empty(n_max, np.int32); ctx.d2h(reason, d_reason)
    finally:
        for p in bufs + outs:
            ctx.free(p)
    return info, X[:max(info[0], 0)], ijo[:max(info[0], 0)], reason


def _as_keypoints(s, seed):
    """the scene's matches as two shuffled keypoint arrays with decoys + the (query, train) pairs that index them"""
    rng = np.random.default_rng(seed)
    n = len(s["pts1"])
    m1, m2 = n + 37, n + 53
    q, t = rng.permutation(m1)[:n], rng.permutation(m2)[:n]
    kp1 = rng.uniform(0, 1200, (m1, 2)).astype(np.float32); kp2 = rng.uniform(0, 370, (m2, 2)).astype(np.float32)
    kp1[q] = s["pts1"]; kp2[t] = s["pts2"]
    return dict(s, kp1=kp1, kp2=kp2), np.stack([q, t], 1).astype(np.int32)


@pytest.mark.parametrize("name", ["outliers30_1000", "turns_2500", "behind_700", "parallel_rays_220"])
def test_device_entry_after_the_device_filter_is_bitwise_the_host_entry(tri, gpu_ctx, name):
    """keypoints on the device -> `sslam_fmat_ransac_dev` on the planted matches -> `sslam_triangulate_2view_dev` on the pairs
    and the count it left there, poses read from device memory: bitwise the host entry fed the same kept pairs."""
    E = load_pkg("epipolar")
    ctx = gpu_ctx
    s, ij = _as_keypoints(SCENES[name], 5)
    n = len(ij)
    d_kp1, d_kp2, d_ij, d_n = ctx.upload(s["kp1"]), ctx.upload(s["kp2"]), ctx.upload(ij), ctx.upload(np.array([n], np.int32))
    d_T1, d_T2 = ctx.upload(np.ascontiguousarray(s["T1"])), ctx.upload(np.ascontiguousarray(s["T2"]))
    d_fij, d_finfo = ctx.malloc(n * 8), ctx.malloc(16)
    d_X, d_ijo, d_info = ctx.malloc(n * 24), ctx.malloc(n * 8), ctx.malloc(32)
    try:
        E.filter_matches_dev(ctx, n, d_n, d_kp1, d_kp2, d_ij, d_fij, d_finfo, thresh=3.0)
        tri.triangulate_2view_dev(ctx, n, d_finfo, d_kp1, d_kp2, d_fij, s["K"], d_T1, d_T2, d_X, d_ijo, d_info, **s["params"])
        ctx.sync()
        finfo = np.empty(4, np.int32); ctx.d2h(finfo, d_finfo)
        fij = np.empty((n, 2), np.int32); ctx.d2h(fij, d_fij)
        info = np.empty(8, np.int32); ctx.d2h(info, d_info)
        X = np.empty((n, 3)); ctx.d2h(X, d_X)
        ijo = np.empty((n, 2), np.int32); ctx.d2h(ijo, d_ijo)
    finally:
        for p in (d_kp1, d_kp2, d_ij, d_n, d_T1, d_T2, d_fij, d_finfo, d_X, d_ijo, d_info):
            ctx.free(p)
    k = int(finfo[0])
    assert 8 <= k <= n
    fij = fij[:k]
    Xh, idxh, reasons_h, _ = tri.triangulate_2view(s["kp1"][fij[:, 0]], s["kp2"][fij[:, 1]], s["K"], s["T1"], s["T2"], ctx=ctx,
                                                    **s["params"])
    print(f"{name}: filter kept {k} / {n}, triangulation kept {info[0]} (host {len(idxh)})")
    assert info[0] == len(idxh) > 0 and info[7] == k
    assert [int(v) for v in info[1:7]] == [reasons_h[r] for r in R.REASONS]
    np.testing.assert_array_equal(ijo[:info[0]], fij[idxh])
    assert X[:info[0]].tobytes() == Xh.tobytes()


@pytest.mark.parametrize("count", [-1, 0])
def test_an_upstream_count_of_minus_one_gives_nothing(tri, gpu_ctx, count):
    s, ij = _as_keypoints(SCENES["odd_100"], 6)
    info, X, ijo, _ = _dev_run(tri, gpu_ctx, s, ij, count, len(ij))
    assert info.tolist() == [0] * 8 and len(X) == 0


def test_device_count_below_the_bound_and_diagnostics(tri, gpu_ctx):
    """a device count smaller than n_max: only that many pairs are read; reasons per match as the host entry's"""
    s, ij = _as_keypoints(SCENES["turns_1025"], 7)
    n_use = 700
    info, X, ijo, reason = _dev_run(tri, gpu_ctx, s, ij, n_use, len(ij))
    Xh, idxh, reasons_h, dh = tri.triangulate_2view(s["pts1"][:n_use], s["pts2"][:n_use], s["K"], s["T1"], s["T2"], want_diag=True,
                                                     ctx=gpu_ctx, **s["params"])
    assert info[7] == n_use and info[0] == len(idxh)
    np.testing.assert_array_equal(reason[:n_use], dh["reason"])
    np.testing.assert_array_equal(ijo, ij[:n_use][idxh])
    assert X.tobytes() == Xh.tobytes()


def test_bad_arguments_are_errors(tri, gpu_ctx, native):
    s = SCENES["odd_100"]
    with pytest.raises(ValueError):
        tri.triangulate_2view(s["pts1"], s["pts2"][:-1], s["K"], s["T1"], s["T2"], ctx=gpu_ctx)
    with pytest.raises(native.NativeError):
        tri.triangulate_2view(s["pts1"], s["pts2"], np.zeros((3, 3)), s["T1"], s["T2"], ctx=gpu_ctx)
