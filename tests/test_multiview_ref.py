"""The numpy restatement of multi-view triangulation (tests/multiview_ref.py) against the contract that the reference's
tests of its lost module record (tests/test_multi_view_utils.py, tests/test_multi_view_triangulation-minimal.py), on scenes
rebuilt from their parameters; the planted verdicts of tests/multiview_scenes.py; the measured floor of the GPU tolerance;
and the two drop-in module names.  No GPU."""
import numpy as np
import pytest

import multiview_ref as R
import multiview_scenes as S
from conftest import load_pkg

SCENES = S.all_scenes()
JACOBI_VS_LAPACK = 4.2e-14          # see tests/test_multiview_gpu.py
SVDS = ("lapack", "qr_jacobi")


def _pinhole(f, c):
    return np.array([[f, 0.0, c], [0.0, f, c], [0.0, 0.0, 1.0]])


@pytest.mark.parametrize("svd", SVDS)
def test_three_noise_free_views(svd):
    K = _pinhole(500.0, 320.0)
    poses = [S.translated_pose(0, 0, 0), S.translated_pose(1, 0, 0), S.translated_pose(0, 1, 0)]
    X_true = np.array([2.0, 1.5, 8.0])
    X = R.multi_view_triangulation(K, poses, S.observe(K, poses, X_true), min_depth=0.5, max_depth=50.0, max_rep_err=0.5, svd=svd)
    assert X is not None
    np.testing.assert_allclose(X, X_true, rtol=0, atol=1e-3)


@pytest.mark.parametrize("svd", SVDS)
def test_four_noisy_views(svd):
    K = _pinhole(600.0, 320.0)
    poses = [S.translated_pose(0, 0, 0), S.translated_pose(1, 0.2, 0), S.translated_pose(-0.3, 1, 0), S.translated_pose(0.5, -0.1, 0.3)]
    X_true = np.array([-1.5, 0.8, 6.5])
    pts2d = S.observe(K, poses, X_true, np.random.RandomState(42), 0.4)        # (the recorded scene seeds the legacy generator with 42)
    X = R.multi_view_triangulation(K, poses, pts2d, min_depth=0.5, max_depth=50.0, max_rep_err=2.0, svd=svd)
    assert X is not None
    err = float(np.linalg.norm(X - X_true))
    print(f"four noisy views ({svd}): {err:.4f} m")
    assert err < 0.05


@pytest.mark.parametrize("seed", [1, 2, 4, 5, 6, 9, 11])
def test_five_views_forty_points(seed):
    K, poses, pts_w, pts2d = S.five_view_scene(seed)
    d = np.linalg.norm(pts_w[:, None] - pts_w[None], axis=2)[np.triu_indices(len(pts_w), 1)]
    assert d.min() > 0.1                                     # (no two true points within the default merge radius)
    for svd in SVDS:
        errs = []
        for j in range(len(pts_w)):
            X = R.multi_view_triangulation(K, poses, np.float32([v[j] for v in pts2d]), min_depth=0.1, max_depth=10.0,
                                           max_rep_err=2.0, svd=svd)
            assert X is not None
            errs.append(np.linalg.norm(X - pts_w[j]))
        rms = float(np.sqrt(np.mean(np.square(errs))))
        print(f"seed {seed} ({svd}): RMS {rms:.4f} m")
        assert rms < 5e-2


def test_fewer_than_two_views_is_none():
    K = _pinhole(500.0, 320.0)
    assert R.multi_view_triangulation(K, [np.eye(4)], np.float32([[320, 320]]), 0.1, 10.0, 2.0) is None
    assert R.multi_view_triangulation(K, [], np.empty((0, 2), np.float32), 0.1, 10.0, 2.0) is None


@pytest.mark.parametrize("name", list(SCENES))
def test_every_track_gets_its_planted_reason(name):
    s = SCENES[name]
    for svd in SVDS:
        _, kept, reason, _ = R.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"], s["uv"], svd=svd, **s["params"])
        np.testing.assert_array_equal(reason, s["reason"])
        np.testing.assert_array_equal(kept, np.flatnonzero(s["reason"] == R.KEPT))


def test_every_reason_is_planted_somewhere():
    seen = np.unique(np.concatenate([s["reason"] for s in SCENES.values()]))
    assert seen.tolist() == list(range(len(R.REASONS)))
    views = np.unique(np.concatenate([np.diff(s["off"]) for s in SCENES.values()]))
    assert set(views.tolist()) >= {1, 2, 3, 5, 33}


def test_the_measured_floor_still_holds():
    worst = 0.0
    for s in SCENES.values():
        Xl, kl, rl, _ = R.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"], s["uv"], svd="lapack", **s["params"])
        Xj, kj, rj, _ = R.triangulate_tracks(s["K"], s["Tcw"], s["off"], s["view"], s["uv"], svd="qr_jacobi", **s["params"])
        np.testing.assert_array_equal(rl, rj)
        if len(Xl):
            worst = max(worst, float((np.linalg.norm(Xj - Xl, axis=1) / np.linalg.norm(Xl, axis=1)).max()))
    print(f"LAPACK on A against Givens-R + the Jacobi port, all scenes: {worst:.3e}")
    assert 0 < worst <= JACOBI_VS_LAPACK


def test_the_drop_in_modules_expose_the_names():
    mvu = load_pkg("slam.core.multi_view_utils")
    tu = load_pkg("slam.core.triangulation_utils")
    assert callable(mvu.multi_view_triangulation) and isinstance(mvu.MultiViewTriangulator, type)
    assert tu.multi_view_triangulation is mvu.multi_view_triangulation
    tri = mvu.MultiViewTriangulator(S.K)
    assert (tri.min_views, tri.merge_radius, tri.max_rep_err, tri.min_depth, tri.max_depth) == (2, 0.10, 2.0, 0.40, 100.0)
