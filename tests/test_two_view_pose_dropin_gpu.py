"""`recover_pose_from_fundamental` and `bootstrap_two_view_map` through the overlay's `two_view_pose` names, the way the
reference's bootstrap drives them (slam/core/two_view_bootstrap.py:202-220, :328-411), against the numpy restatement
(tests/relative_pose_ref.py): on the overlay's `Map` and on a plain dict-of-objects map."""
from types import SimpleNamespace

import numpy as np
import pytest

import relative_pose_ref as R
import relative_pose_scenes as S
from conftest import load_pkg
from test_relative_pose_gpu import PAR_BAR, RT_BAR, X_BAR

pytestmark = pytest.mark.gpu

SCENE = S.make_scene("dropin_700", 700, "sideways", 201, mismatch=0.2, far=0.15, behind=0.05)
ARGS = SimpleNamespace(min_depth=3.0, max_depth=45.0)


class PlainPoint:
    def __init__(self, pid, position):
        self.id, self.position, self.observations = pid, np.array(position, float), []

    def add_observation(self, keyframe_idx, kp_idx, descriptor):
        self.observations.append((keyframe_idx, kp_idx, descriptor))


class PlainMap:
    """a reference-style map: a dict of objects, ids from a counter"""
    def __init__(self):
        self.points, self._next_pid = {}, 0

    def add_points(self, pts3d, colours=None, keyframe_idx=-1):
        ids = []
        for p in np.asarray(pts3d):
            self.points[self._next_pid] = PlainPoint(self._next_pid, p)
            ids.append(self._next_pid)
            self._next_pid += 1
        return ids


@pytest.fixture(scope="module")
def tp():
    return load_pkg("slam.core.two_view_pose")


def planted_frames(s, seed=7, n_decoy=90):
    """the scene's matches as two shuffled keypoint lists with decoys, descriptors, and the DMatch list that pairs them"""
    ty = load_pkg("slam.core.types")
    rng = np.random.default_rng(seed)
    n = s["n"]
    m = n + n_decoy
    q, t = rng.permutation(m)[:n], rng.permutation(m)[:n]
    xy0 = rng.uniform(2, 1200, (m, 2)).astype(np.float32); xy1 = rng.uniform(2, 370, (m, 2)).astype(np.float32)
    xy0[q] = s["pts1"]; xy1[t] = s["pts2"]
    d0 = rng.standard_normal((m, 128)).astype(np.float32); d1 = rng.standard_normal((m, 128)).astype(np.float32)
    matches = ty.matches_from_ij(np.stack([q, t], 1).astype(np.int32))
    return ty.keypoints_from_xy(xy0), d0, ty.keypoints_from_xy(xy1), d1, matches, q, t


def _fundamental(s):
    Ki = np.linalg.inv(s["K"])
    return Ki.T @ s["E"] @ Ki


def test_recover_pose_from_fundamental_is_the_restatement(tp, gpu_ctx, caplog):
    import logging
    s = SCENE
    F = _fundamental(s)
    E = s["K"].T @ F @ s["K"]
    good, R_r, t_r, mask_r, d = R.recover_pose(E, s["pts1"], s["pts2"], s["K"])
    assert S.margins_clear(d["margins"]).all() and good >= 60
    inl = mask_r.ravel().astype(bool)
    pd_r, par_r, N_r, dd = R.two_view_metrics(s["K"], R_r, t_r, s["pts1"][inl], s["pts2"][inl])
    assert (np.abs(dd["z"]) > S.MARGIN_METRIC_Z).all()
    with caplog.at_level(logging.INFO, logger="two_view_bootstrap"):
        pose = tp.recover_pose_from_fundamental(s["K"], F, s["pts1"], s["pts2"], tp.InitParams())
    assert f"recoverPose(E): ok={good}  inliers={good}" in caplog.text and "F/E accepted" in caplog.text
    assert pose is not None and pose.model is tp.TwoViewModel.FUNDAMENTAL and pose.t.shape == (3, 1)
    assert np.abs(pose.R - R_r).max() <= RT_BAR and np.abs(pose.t - t_r).max() <= RT_BAR
    assert pose.posdepth == pd_r and abs(pose.parallax_deg - par_r) <= PAR_BAR
    # the thresholds reject as the reference's do
    assert tp.recover_pose_from_fundamental(s["K"], F, s["pts1"], s["pts2"], tp.InitParams(min_pts_for_tests=good + 1)) is None
    assert tp.recover_pose_from_fundamental(s["K"], F, s["pts1"], s["pts2"], tp.InitParams(min_parallax_deg=par_r + 0.5)) is None
    assert tp.triangulation_metrics(s["K"], R_r, t_r, s["pts1"][:1], s["pts2"][:1]) == (0.0, 0.0, 0)
    ok, pd, ang = tp.validate_two_view_pose(s["K"], R_r, t_r, s["pts1"][inl], s["pts2"][inl], tp.InitParams())
    assert ok and pd == pd_r and abs(ang - par_r) <= PAR_BAR


def _decision(tp, s, mask):
    pose = tp.TwoViewPose(tp.TwoViewModel.FUNDAMENTAL, s["R"].copy(), s["t"].reshape(3, 1).copy(), 1.0, 2.0)
    return tp.TwoViewDecision(pose=pose, inlier_mask=mask)


@pytest.mark.parametrize("kind", ["overlay_map", "plain_map"])
def test_bootstrap_builds_the_map_the_restatement_would(tp, gpu_ctx, kind):
    lmu = load_pkg("slam.core.landmark_utils")
    s = SCENE
    kp0, d0, kp1, d1, matches, q, t = planted_frames(s)
    mask = s["kind"] != S.MISMATCH
    wmap = lmu.Map() if kind == "overlay_map" else PlainMap()
    ok, T0, T1 = tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches, ARGS, wmap, decision=_decision(tp, s, mask))

    # the restatement of :372-408 on the same inliers
    _, _, _, dd = R.two_view_metrics(s["K"], s["R"], s["t"], s["pts1"], s["pts2"], sel=mask)
    z0, z1 = dd["z"][:, 0], dd["z"][:, 1]
    for z in (z0, z1):
        for bound in (ARGS.min_depth, ARGS.max_depth):
            assert (np.abs(z - bound) > 1e-6 * bound).all()           # no point on an edge of the depth window
    keep = (z0 > ARGS.min_depth) & (z0 < ARGS.max_depth) & (z1 > ARGS.min_depth) & (z1 < ARGS.max_depth)
    X_r = dd["X"][keep]
    sel = np.flatnonzero(mask)[keep]
    print(f"{kind}: {mask.sum()} inliers, {keep.sum()} inside the depth window, {len(wmap.points)} landmarks")
    assert ok and 80 <= keep.sum() < mask.sum()
    assert np.array_equal(T0, np.eye(4)) and np.array_equal(T1[:3, :3], s["R"]) and np.array_equal(T1[:3, 3], s["t"])
    assert np.array_equal(T1[3], [0, 0, 0, 1])
    ids = list(wmap.points.keys())
    assert ids == list(range(len(X_r))) and wmap._next_pid == len(X_r)
    canon = lmu._canon_desc if kind == "overlay_map" else (lambda d: d)
    X = np.array([np.asarray(wmap.points[p].position) for p in ids])
    assert (np.linalg.norm(X - X_r, axis=1) / np.linalg.norm(X_r, axis=1)).max() <= X_BAR
    for pid, m_idx in zip(ids, sel.tolist()):
        (f0, k0, dd0), (f1, k1, dd1) = wmap.points[pid].observations
        assert (f0, k0, f1, k1) == (0, q[m_idx], 1, t[m_idx])
        np.testing.assert_array_equal(dd0, canon(d0[q[m_idx]])); np.testing.assert_array_equal(dd1, canon(d1[t[m_idx]]))
    # the points are the scene's
    rel = np.linalg.norm(X - s["X_true"][sel], axis=1) / np.linalg.norm(s["X_true"][sel], axis=1)
    assert rel.max() < 1e-2


@pytest.mark.parametrize("kind", ["overlay_map", "plain_map"])
def test_early_returns_leave_the_map_untouched(tp, gpu_ctx, kind):
    lmu = load_pkg("slam.core.landmark_utils")
    s = SCENE
    kp0, d0, kp1, d1, matches, q, t = planted_frames(s)
    inl = s["kind"] != S.MISMATCH
    wmap = lmu.Map() if kind == "overlay_map" else PlainMap()
    none = (False, None, None)
    # 49 matches
    assert tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches[:49], ARGS, wmap, decision=_decision(tp, s, inl[:49])) == none
    assert tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches[:49], ARGS, wmap) == none       # (before the gate is asked for)
    # 59 inliers
    m59 = np.zeros(s["n"], bool); m59[np.flatnonzero(inl)[:59]] = True
    assert tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches, ARGS, wmap, decision=_decision(tp, s, m59)) == none
    # fewer than 80 points after the depth window: 79 good inliers and every far one
    few = np.zeros(s["n"], bool); few[np.flatnonzero(s["kind"] == S.GOOD)[:79]] = True; few[s["kind"] == S.FAR] = True
    assert few.sum() >= 100
    narrow = SimpleNamespace(min_depth=1.0, max_depth=50.0)
    assert tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches, narrow, wmap, decision=_decision(tp, s, few)) == none
    assert len(wmap.points) == 0 and wmap._next_pid == 0
    # ... and one more good inlier is enough
    few[np.flatnonzero(s["kind"] == S.GOOD)[79]] = True
    ok, _, _ = tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches, narrow, wmap, decision=_decision(tp, s, few))
    assert ok and len(wmap.points) == 80


def test_no_decision_is_an_error_not_half_a_gate(tp, gpu_ctx):
    lmu = load_pkg("slam.core.landmark_utils")
    s = SCENE
    kp0, d0, kp1, d1, matches, q, t = planted_frames(s)
    wmap = lmu.Map()
    with pytest.raises(NotImplementedError, match="homography"):
        tp.bootstrap_two_view_map(s["K"], kp0, d0, kp1, d1, matches, ARGS, wmap)
    assert len(wmap.points) == 0
