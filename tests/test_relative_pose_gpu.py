"""`sslam_recover_pose_host` / `sslam_two_view_metrics_host` against the numpy restatement (tests/relative_pose_ref.py) on
every scene of tests/relative_pose_scenes.py.

Verdicts (good, the mask, the four counts, N, the in-front count) must be IDENTICAL.  That can only be asked when no match
sits on a comparison, so each test first asserts on the restatement alone that the winner's count exceeds every other
candidate's and that every match clears every comparison of every candidate by a margin far above any rounding
difference: |Q2 Q3| > 1e-9 on the unit-norm homogeneous point, both depths 1e-6 away from 0 and 1e-6 relative away from
distance_thresh, the metrics' z1 and z2 1e-9 away from 0.  The SVD's sign and order choices permute the four candidates,
so the winner is compared by value and the counts sorted.

R, t, X and the parallax: the tolerance is measured, not guessed.  The `*_FLOOR` constants are the largest disagreement,
over all scenes, between the restatement with LAPACK's SVDs and the same restatement with the float64 numpy ports of the
one-sided Jacobi the kernels run - two correct evaluations of the same arithmetic (measured on the build machine;
`test_the_measured_floors_still_hold` re-measures them on the CPU part of every GPU run):
    entries of R and of the unit t   5.6e-16 -> 6e-16
    X, relative                      2.85e-10 -> 2.9e-10  (not rounding: X = Xh[:3] / (Xh[3] + 1e-12) and the SIGN of Xh is the
                                     SVD's to choose, so the 1e-12 enters with either sign - 2e-12 / |Xh[3]|, and a far point
                                     has |Xh[3]| near 1 / 100)
    parallax, degrees                1.1e-10 -> 1.2e-10   (the same 1e-12 through the median point)
The GPU may differ from the restatement by 100 x that (it reorders operations), and in no case by more than 1e-9 on R and t,
1e-6 relative on X, 1e-6 degrees on the parallax.
"""
import numpy as np
import pytest

import relative_pose_ref as R
import relative_pose_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SCENES = S.all_scenes()
RT_FLOOR, X_FLOOR, PAR_FLOOR = 6e-16, 2.9e-10, 1.2e-10
RT_BAR, X_BAR, PAR_BAR = 100 * RT_FLOOR, 100 * X_FLOOR, 100 * PAR_FLOOR
assert RT_BAR <= 1e-9 and X_BAR <= 1e-6 and PAR_BAR <= 1e-6


@pytest.fixture(scope="module")
def rp():
    return load_pkg("relative_pose")


@pytest.fixture(scope="module")
def ref():
    """the restatement's answers, computed once: name -> (recover_pose result, two_view_metrics result)"""
    return {name: (R.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"]),
                   R.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"]))
            for name, s in SCENES.items()}


def _rel(X, Xref):
    return float((np.linalg.norm(X - Xref, axis=1) / np.linalg.norm(Xref, axis=1)).max()) if len(Xref) else 0.0


def assert_vote_margins(s, detail):
    if s["n"] == 0:
        return
    c = detail["counts"]
    assert all(c[detail["winner"]] > v for k, v in enumerate(c) if k != detail["winner"]), c
    assert S.margins_clear(detail["margins"]).all()


def assert_metric_margins(detail):
    assert (np.abs(detail["z"]) > S.MARGIN_METRIC_Z).all()


def test_the_measured_floors_still_hold():
    w_rt = w_x = w_par = 0.0
    for s in SCENES.values():
        gl, Rl, tl, ml, dl = R.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"], svd="lapack")
        gj, Rj, tj, mj, dj = R.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"], svd="jacobi")
        assert gl == gj and np.array_equal(ml, mj) and sorted(dl["counts"]) == sorted(dj["counts"])
        if s["n"]:
            w_rt = max(w_rt, float(np.abs(Rl - Rj).max()), float(np.abs(tl - tj).max()))
        pl = R.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"], svd="lapack")
        pj = R.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"], svd="jacobi")
        assert pl[0] == pj[0] and pl[2] == pj[2]
        w_x = max(w_x, _rel(pj[3]["X"], pl[3]["X"]))
        w_par = max(w_par, abs(pl[1] - pj[1]))
    print(f"LAPACK against the Jacobi ports, all scenes: R / t {w_rt:.3e}, X {w_x:.3e} relative, parallax {w_par:.3e} degrees")
    assert w_rt <= RT_FLOOR and w_x <= X_FLOOR and w_par <= PAR_FLOOR


@pytest.mark.parametrize("name", list(SCENES))
def test_recover_pose_equals_the_restatement(rp, gpu_ctx, ref, name):
    s = SCENES[name]
    good_r, R_r, t_r, mask_r, d = ref[name][0]
    assert_vote_margins(s, d)
    good, Rm, t, mask, info = rp.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"], ctx=gpu_ctx,
                                              want_info=True)
    assert Rm.shape == (3, 3) and t.shape == (3, 1) and mask.shape == (s["n"], 1) and mask.dtype == np.uint8
    if s["n"] == 0:       # no vote: candidate 1 of the kernel's own SVD, which is one of the restatement's four
        cands = [(d["R1"], d["t"]), (d["R2"], d["t"]), (d["R1"], -d["t"]), (d["R2"], -d["t"])]
        err = min(max(np.abs(Rm - Rc).max(), np.abs(t.ravel() - tc).max()) for Rc, tc in cands)
        assert good == 0 and info == {"winner": 0, "counts": [0, 0, 0, 0]} and err <= RT_BAR
        return
    e_R, e_t = float(np.abs(Rm - R_r).max()), float(np.abs(t - t_r).max())
    print(f"{name}: good {good} / {s['n']}, counts {info['counts']} (restatement {d['counts']}), winner {info['winner']} "
          f"({d['winner']}), R {e_R:.3e}, t {e_t:.3e} (bar {RT_BAR:.1e})")
    assert good == good_r == info["counts"][info["winner"]]
    np.testing.assert_array_equal(mask, mask_r)
    assert sorted(info["counts"]) == sorted(d["counts"])
    assert e_R <= RT_BAR and e_t <= RT_BAR
    # a second call: bit for bit
    g2, R2, t2, m2 = rp.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"], ctx=gpu_ctx)
    assert g2 == good and R2.tobytes() == Rm.tobytes() and t2.tobytes() == t.tobytes() and m2.tobytes() == mask.tobytes()


@pytest.mark.parametrize("name", list(SCENES))
def test_two_view_metrics_equal_the_restatement(rp, gpu_ctx, ref, name):
    s = SCENES[name]
    pd_r, par_r, N_r, d = ref[name][1]
    assert_metric_margins(d)
    pd, par, N, X, z, info = rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"], want_points=True,
                                                 ctx=gpu_ctx, want_info=True)
    e_x = _rel(X, d["X"]) if X.shape == d["X"].shape else float("nan")
    print(f"{name}: N {N}, in front {info['in_front']}, posdepth {pd:.6f}, parallax {par:.9f} (restatement {par_r:.9f}, "
          f"bar {PAR_BAR:.1e}), X rel {e_x:.3e} (bar {X_BAR:.1e})")
    assert N == N_r and info["in_front"] == d["in_front"] and pd == pd_r
    assert X.shape == d["X"].shape and z.shape == d["z"].shape and e_x <= X_BAR
    assert abs(par - par_r) <= PAR_BAR
    if len(X):
        assert np.array_equal(z[:, 0], X[:, 2]) and (np.abs(z - d["z"]) <= X_BAR * np.linalg.norm(d["X"], axis=1).max()).all()
    # a second call, and the same matches compacted on the host instead of selected on the device: bit for bit
    again = rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"], want_points=True, ctx=gpu_ctx)
    keep = s["sel"] != 0
    host = rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"][keep], s["pts2"][keep], want_points=True, ctx=gpu_ctx)
    for other in (again, host):
        assert other[:3] == (pd, par, N) and other[3].tobytes() == X.tobytes() and other[4].tobytes() == z.tobytes()


def test_every_median_position_is_exact(rp, gpu_ctx):
    """every N of 2 .. 40 (both parities, fewer values than a wave, than the 256 bins of a selection pass) and either side
    of one turn of the tail's workgroup (1024), on the good matches of one scene"""
    s = SCENES["sideways_4096"]
    good = np.flatnonzero(s["kind"] == S.GOOD)
    for N in list(range(2, 41)) + [1023, 1024, 1025, 1026]:
        idx = good[:N]
        pd, par, n_used = rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"][idx], s["pts2"][idx], ctx=gpu_ctx)
        pr, par_r, n_r, _ = R.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"][idx], s["pts2"][idx])
        assert (n_used, pd) == (n_r, pr) and abs(par - par_r) <= PAR_BAR, N


def test_a_slab_driven_large_then_small(rp, native, ref):
    """one fresh context: the largest scene sizes its scratch slab, the small ones then run inside it"""
    ctx = native.Context(0)
    try:
        for name in ("rotation_4097", "forward_63", "single_1", "sideways_255"):
            s = SCENES[name]
            good, Rm, t, mask = rp.recover_pose(s["E"], s["pts1"], s["pts2"], s["K"], s["thresh"], mask=s["mask"], ctx=ctx)
            pd, par, N, X, z = rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"], want_points=True, ctx=ctx)
            (good_r, R_r, t_r, mask_r, _), (pd_r, par_r, N_r, d) = ref[name]
            assert good == good_r and np.array_equal(mask, mask_r) and np.abs(Rm - R_r).max() <= RT_BAR
            assert (pd, N) == (pd_r, N_r) and abs(par - par_r) <= PAR_BAR and _rel(X, d["X"]) <= X_BAR
    finally:
        ctx.close()


def test_bad_arguments_are_errors(rp, gpu_ctx, native):
    s = SCENES["forward_63"]
    with pytest.raises(ValueError):
        rp.recover_pose(s["E"], s["pts1"], s["pts2"][:-1], s["K"], ctx=gpu_ctx)
    with pytest.raises(ValueError):
        rp.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=s["sel"][:-1], ctx=gpu_ctx)
    with pytest.raises(native.NativeError):
        rp.recover_pose(s["E"], s["pts1"], s["pts2"], np.zeros((3, 3)), ctx=gpu_ctx)
    big = np.zeros((16385, 2), np.float32)
    with pytest.raises(native.NativeError, match="16384"):
        rp.two_view_metrics(s["K"], s["R"], s["t"], big, big, ctx=gpu_ctx)
