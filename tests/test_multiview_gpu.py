"""`sslam_triangulate_tracks_host` against the numpy restatement (tests/multiview_ref.py) on every scene of
tests/multiview_scenes.py: 0, 1, 255, 256, 257 and 1025 tracks, 1 / 2 / 3 / 5 / 33 views per track mixed inside one call, every
reason planted.

Verdicts (reason per track, kept indices, counters) must be IDENTICAL.  That can only be asked when no track sits on a
threshold, so each test first asserts on the restatement's diagnostics alone that every track clears every gate by a margin
far above any rounding difference: 1e-6 relative for the smallest and largest depth against the window bounds and the 1e-6
front test, 1e-6 px for the mean reprojection error, |w| a decade either side of 1e-12.

Positions: the tolerance is measured, not guessed.  `JACOBI_VS_LAPACK` is the largest relative disagreement, over the kept
points of all scenes, between the restatement with LAPACK's SVD of A and the same restatement with the float64 numpy port of
what the kernel runs (A folded into its triangular factor by Givens rotations, then the one-sided Jacobi) - two correct
evaluations of the same arithmetic: 4.2e-14 (measured on the build machine; `test_the_measured_floor_still_holds` of
tests/test_multiview_ref.py re-measures it on every run).  The GPU may differ from the restatement by 100 x that (its hypot,
divisions and sums round differently): 4.2e-12 relative, and in no case more than 1e-6.

Two cases differ from the wording of the issue that asked for them, for reasons tests/multiview_scenes.py spells out: the
planted invalid_w is a translation-only pair seeing one pixel (parallel rays; a pure-rotation pair sharing a ray meets in
the common centre and is bad_depth), and a point behind one camera with min_depth = 0 is bad_depth by the definition's own
order - that scene is kept as asked, and a second one with min_depth = -100 reaches behind_cam.
"""
import numpy as np
import pytest

import multiview_ref as R
import multiview_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SCENES = S.all_scenes()
JACOBI_VS_LAPACK = 4.2e-14
X_BAR = 100 * JACOBI_VS_LAPACK
assert X_BAR <= 1e-6

_REF = {}


def ref_of(name):
    """the restatement's result per scene, computed once"""
    if name not in _REF:
        s = SCENES[name]
        out = R.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"], s["uv"], **s["params"])
        for a in (out[0], out[1], out[2], *out[3].values()):
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


@pytest.fixture(scope="module")
def mv():
    return load_pkg("multiview")


def _rel(X, Xref):
    return float((np.linalg.norm(X - Xref, axis=1) / np.linalg.norm(Xref, axis=1)).max()) if len(Xref) else 0.0


def assert_margins(diag, reason, P):
    """every track clears every gate, on the restatement's own diagnostics (a track without a point has none)"""
    has = np.isin(reason, (R.KEPT, R.BAD_DEPTH, R.BEHIND_CAM, R.HIGH_REPROJ))
    for z in (diag["z_min"][has], diag["z_max"][has]):
        for bound in (P["min_depth"], P["max_depth"], 1e-6):
            assert (np.abs(z - bound) > 1e-6 * abs(bound)).all()
    e = diag["mean_err"][has]
    assert (np.abs(e[np.isfinite(e)] - P["max_rep_err"]) > 1e-6).all()
    w = np.abs(diag["w"][reason != R.TOO_FEW_VIEWS])
    assert ((w < 1e-13) | (w > 1e-11)).all()                 # the |w| > 1e-12 test, a decade either side


def _run(mv, ctx, s, **kw):
    return mv.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"], s["uv"], ctx=ctx, **s["params"], **kw)


@pytest.mark.parametrize("name", list(SCENES))
def test_host_entry_equals_the_restatement(mv, gpu_ctx, name):
    s = SCENES[name]
    P = s["params"]
    Xr, ir, rr, dr = ref_of(name)
    assert_margins(dr, rr, P)
    np.testing.assert_array_equal(rr, s["reason"])
    n = len(rr)
    if n >= 2:
        assert 0 < len(ir) < n                               # neither the kept nor the rejected set is empty
    X, idx, reasons, diag = _run(mv, gpu_ctx, s, want_diag=True)
    rel = _rel(X, Xr) if np.array_equal(idx, ir) else float("nan")
    print(f"{name}: kept {len(idx)} / {n}, reasons {reasons}, positions rel {rel:.3e} (bar {X_BAR:.1e})")
    np.testing.assert_array_equal(diag["reason"], rr)
    np.testing.assert_array_equal(idx, ir)
    assert reasons == {k: int((rr == c).sum()) for c, k in enumerate(R.REASONS)}
    assert X.shape == Xr.shape and rel <= X_BAR
    # the diagnostics: the restatement's values where every view sees the point in front
    front = np.isfinite(dr["mean_err"])
    np.testing.assert_allclose(diag["z_min"][front], dr["z_min"][front], rtol=1e-6)
    np.testing.assert_allclose(diag["z_max"][front], dr["z_max"][front], rtol=1e-6)
    np.testing.assert_allclose(diag["mean_err"][front], dr["mean_err"][front], rtol=0, atol=1e-5)
    none = np.isin(rr, (R.TOO_FEW_VIEWS, R.INVALID_W))
    assert np.isnan(diag["mean_err"][none]).all()
    # without the optional buffers: the same result
    X2, idx2, reasons2, nothing = _run(mv, gpu_ctx, s)
    assert nothing is None and reasons2 == reasons and np.array_equal(idx2, idx) and X2.tobytes() == X.tobytes()


def test_every_reason_is_reached_on_the_device(mv, gpu_ctx):
    total = {k: 0 for k in R.REASONS}
    for s in SCENES.values():
        for k, v in _run(mv, gpu_ctx, s)[2].items():
            total[k] += v
    print(total)
    assert all(v > 0 for v in total.values())


def test_two_view_tracks_agree_with_the_two_view_entry(mv, gpu_ctx):
    """every track of this scene has the same two views: the positions of `triangulate_2view` (its own 4 x 4 Jacobi, no
    triangular factor first) within the same bar"""
    tri = load_pkg("triangulation")
    s = SCENES["pairs_300"]
    a, b = s["pair_only"]
    X, idx, _, _ = _run(mv, gpu_ctx, s)
    X2, idx2, _, _ = tri.triangulate_2view(s["uv"][0::2], s["uv"][1::2], s["K"], s["Tcw"][a], s["Tcw"][b], min_depth=s["params"]["min_depth"],
                                           max_depth=s["params"]["max_depth"], use_parallax_gate=False, reproj_px_max=1e9, ctx=gpu_ctx)
    both, ia, ib = np.intersect1d(idx, idx2, return_indices=True)
    assert len(both) == len(idx) > 100                       # (the two-view call gates depth only: it keeps at least these)
    rel = _rel(X[ia], X2[ib])
    print(f"two-view tracks against triangulate_2view: rel {rel:.3e} (bar {X_BAR:.1e})")
    assert rel <= X_BAR


def test_a_result_does_not_depend_on_its_neighbours(mv, gpu_ctx):
    """the tracks of one scene in reverse order: bitwise the same points"""
    s = SCENES["mixed_257"]
    X, idx, _, _ = _run(mv, gpu_ctx, s)
    n = len(s["off"]) - 1
    order = np.arange(n)[::-1]
    cnt = np.diff(s["off"])[order]
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    obs = np.concatenate([np.arange(s["off"][i], s["off"][i + 1]) for i in order])
    Xr, idxr, _, _ = mv.triangulate_tracks(s["K"], s["Tcw"], off, s["view"][obs], s["uv"][obs], ctx=gpu_ctx, **s["params"])
    np.testing.assert_array_equal(order[idxr][::-1], idx)
    assert Xr[::-1].tobytes() == X.tobytes()


def test_bad_arguments_are_errors(mv, gpu_ctx, native):
    s = SCENES["mixed_255"]
    with pytest.raises(ValueError):
        mv.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"][:-1], s["uv"], ctx=gpu_ctx)
    bad_view = s["view"].copy()
    bad_view[3] = S.F
    with pytest.raises(native.NativeError):
        mv.triangulate_tracks(s["K"], s["Tcw"], s["off"], bad_view, s["uv"], ctx=gpu_ctx)
    bad_off = s["off"].copy()
    bad_off[2] = bad_off[1] - 1
    with pytest.raises(native.NativeError):
        mv.triangulate_tracks(s["K"], s["Tcw"], bad_off, s["view"], s["uv"], ctx=gpu_ctx)
