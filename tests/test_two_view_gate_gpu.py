"""The overlay's two-view gate (`slam/core/two_view_gate.py`) against a numpy gate assembled from the restatements under
tests/ and oracle/: homography RANSAC (homography_ref), F-matrix RANSAC (oracle.ransac_ref), recoverPose and the
triangulation metrics (relative_pose_ref); the 3 x 3 scores and the homography decomposition are numpy in the product too.

The model, the None-ness and the mask must be IDENTICAL; every scene first asserts on the numpy gate alone that its
ratio_H lies more than 0.05 away from the 0.45 the selection turns on.  R and t:
  * HOMOGRAPHY: the GPU's H may differ from the restatement's by H_BAR = 2e-7 of max |H| (tests/test_homography_gpu.py); R and
    the unit t are smooth functions of Hn whose sensitivity is of the order d / |t|, 10 in the planted scene: 10 x H_BAR,
    2e-6.  The numpy gate on LAPACK against the same gate on the Jacobi / elimination ports is printed beside it
    (1.5e-14 on the build machine);
  * FUNDAMENTAL: the GPU's F and the oracle's come from different null-space solvers and tests/test_ransac_gpu.py lets them
    differ by 1e-7 of max |F|; R and t are smooth functions of the unit-norm E with a unit singular gap, so ten times that,
    1e-6, bounds them.
"""
import logging
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import homography_ref as HR
import homography_scenes as HS
import relative_pose_ref as R
import relative_pose_scenes as S
from conftest import load_pkg
from oracle import ransac_ref
from test_homography_gpu import H_BAR
from test_two_view_pose_dropin_gpu import PlainMap, planted_frames

pytestmark = pytest.mark.gpu

K = S.K
ARGS = SimpleNamespace(min_depth=0.5, max_depth=200.0)
F_PATH_BAR = 1e-6
H_PATH_BAR = 10 * H_BAR


@pytest.fixture(scope="module")
def gate():
    return load_pkg("slam.core.two_view_gate")


def _planar(n, seed, motion, mismatch=0.2, noise=0.1, rotation_only=False):
    rng = np.random.default_rng(seed)
    Rm, t = S.MOTIONS[motion]
    nrm, d = np.array([0.05, 0.1, 1.0]) / np.linalg.norm([0.05, 0.1, 1.0]), 10.0
    z = rng.uniform(0.9, 1.1, n)
    ray = np.stack([rng.uniform(-0.7, 0.7, n), rng.uniform(-0.22, 0.22, n), np.ones(n)], 1)
    X1 = ray * (d / (ray @ nrm))[:, None]                       # on the plane n . X = d
    X2 = X1 @ Rm.T + (0 if rotation_only else 1) * t
    p1 = (X1 @ K.T); p1 = p1[:, :2] / p1[:, 2:]
    p2 = (X2 @ K.T); p2 = p2[:, :2] / p2[:, 2:]
    p1 += rng.normal(0, noise, p1.shape); p2 += rng.normal(0, noise, p2.shape)
    bad = rng.permutation(n)[:int(round(mismatch * n))]
    p2[bad] = np.column_stack([rng.uniform(2, 1238, len(bad)), rng.uniform(2, 373, len(bad))])
    return np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)


def _general(n, seed):
    s = S.make_scene("gate_general", n, "sideways", seed, mismatch=0.2, noise=0.1)
    return s["pts1"], s["pts2"]


SCENES = {
    "planar_parallax": _planar(200, 31, "sideways", mismatch=0.05),
    "general_3d": _general(250, 32),
    "planar_rotation": _planar(200, 33, "rotation", mismatch=0.05, rotation_only=True),
    "seven_matches": tuple(p[:7] for p in _planar(200, 34, "sideways", mismatch=0.0)),
}
EXPECT = {"planar_parallax": "HOMOGRAPHY", "general_3d": "FUNDAMENTAL", "planar_rotation": None, "seven_matches": None}


def numpy_gate(gate, p1, p2, params, linalg="lapack"):
    """`evaluate_two_view_bootstrap_with_masks` from the restatements.  Returns (model name or None, R, t, mask, trace)."""
    trace = {"ratio_H": None, "preferred": None, "h_validated": None}
    if len(p1) < 8:
        return None, None, None, None, trace
    H, maskH, _ = HR.find_homography_ransac(p1, p2, params.ransac_px, linalg=linalg)
    F, maskF, _ = ransac_ref.find_fundamental_ransac(p1, p2, params.ransac_px, 0.99, 1000)
    if H is None and F is None:
        return None, None, None, None, trace
    sc = gate.compute_model_scores(H, F, p1, p2, params)
    trace["ratio_H"] = sc.ratio_H
    svd = "jacobi" if linalg == "jacobi" else "lapack"

    def validate(Rm, t, a, b):
        pd, par, N, _ = R.two_view_metrics(K, Rm, t, a, b, svd=svd)
        return (N >= params.min_pts_for_tests and pd >= params.min_posdepth and par >= params.min_parallax_deg), pd, par

    if sc.ratio_H > params.score_ratio_H and H is not None:
        trace["preferred"] = "H"
        _, Rs, ts, _ = gate.decompose_homography_mat(H, K)
        best, key = None, (-1.0, -1.0)
        for Rm, t in zip(Rs, ts):
            t = t.reshape(3, 1) / (np.linalg.norm(t) + 1e-12)
            ok, pd, par = validate(Rm, t, p1, p2)
            if ok and (pd, par) > key:
                best, key = (Rm, t), (pd, par)
        trace["h_validated"] = best is not None
        if best is not None:
            return "HOMOGRAPHY", best[0], best[1], maskH, trace
    else:
        trace["preferred"] = "F"
    if F is not None:
        E = K.T @ F @ K
        good, Rm, t, maskRP, _ = R.recover_pose(E, p1, p2, K, svd=svd)
        if good and good >= params.min_pts_for_tests:
            inl = maskRP.ravel().astype(bool)
            if validate(Rm, t, p1[inl], p2[inl])[0]:
                return "FUNDAMENTAL", Rm, t, maskF & (maskRP.ravel() > 0), trace
    return None, None, None, None, trace


@pytest.fixture(scope="module")
def refs(gate):
    params = gate.InitParams()
    out = {}
    for name, (p1, p2) in SCENES.items():
        lap = numpy_gate(gate, p1, p2, params, "lapack")
        # (the second variant only where the homography decides: on the general scene its RANSAC runs all 2000 iterations,
        #  seconds of Python in the ported Jacobi, and the F/E path has a bar of its own)
        out[name] = (lap, numpy_gate(gate, p1, p2, params, "jacobi") if EXPECT[name] != "FUNDAMENTAL" else lap)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_the_gate_decides_what_the_numpy_gate_decides(gate, gpu_ctx, refs, name, caplog):
    p1, p2 = SCENES[name]
    (model, R_r, t_r, mask_r, trace), (model_j, R_j, t_j, mask_j, _) = refs[name]
    assert model == model_j == EXPECT[name]
    if len(p1) >= 8:
        assert abs(trace["ratio_H"] - 0.45) > 0.05, trace
    if name == "planar_rotation":
        assert trace["preferred"] == "H" and trace["h_validated"] is False        # ... and the F/E fallback fails too
    with caplog.at_level(logging.INFO, logger="two_view_bootstrap"):
        dec = gate.evaluate_two_view_bootstrap_with_masks(K, p1, p2)
    pose = gate.evaluate_two_view_bootstrap(K, p1, p2)
    assert (dec is None) == (model is None) == (pose is None)
    if name == "seven_matches":
        assert "needs at least 8" in caplog.text
    if name == "planar_rotation":
        assert "H path failed validation" in caplog.text and "Pair rejected: ambiguous" in caplog.text
    if model is None:
        return
    tvp = load_pkg("slam.core.two_view_pose")
    assert type(dec.pose) is tvp.TwoViewPose and dec.pose.model.name == model == pose.model.name
    assert dec.inlier_mask.dtype == np.bool_ and np.array_equal(dec.inlier_mask, mask_r)
    if model == "HOMOGRAPHY":
        floor = max(np.abs(R_r - R_j).max(), np.abs(t_r - t_j).max())
        bar = H_PATH_BAR
        assert floor <= bar
        # the mask is the H-RANSAC's own
        assert np.array_equal(gate._final_inlier_mask_for_model(dec.pose.model, p1, p2, K, dec.pose.R, dec.pose.t, 1.5), mask_r)
    else:
        floor, bar = 0.0, F_PATH_BAR
    e_R, e_t = float(np.abs(dec.pose.R - R_r).max()), float(np.abs(dec.pose.t - t_r).max())
    print(f"{name}: {model}, ratio_H {trace['ratio_H']:.3f}, {int(mask_r.sum())} inliers, R {e_R:.3e}, t {e_t:.3e} "
          f"(LAPACK against the ports {floor:.3e}, bar {bar:.1e})")
    assert dec.pose.t.shape == (3, 1) and e_R <= bar and e_t <= bar
    assert np.array_equal(pose.R, dec.pose.R) and np.array_equal(pose.t, dec.pose.t)


@pytest.mark.parametrize("name", ["planar_parallax", "general_3d"])
def test_bootstrap_without_a_decision_builds_the_same_map(gate, gpu_ctx, name):
    p1, p2 = SCENES[name]
    s = dict(n=len(p1), pts1=p1, pts2=p2)
    kp0, d0, kp1, d1, matches, q, t = planted_frames(s)
    dec = gate.evaluate_two_view_bootstrap_with_masks(K, p1, p2)
    with_dec, without = PlainMap(), PlainMap()
    a = gate.bootstrap_two_view_map(K, kp0, d0, kp1, d1, matches, ARGS, with_dec, decision=dec)
    b = gate.bootstrap_two_view_map(K, kp0, d0, kp1, d1, matches, ARGS, without)
    assert a[0] and b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert len(with_dec.points) == len(without.points) >= 80
    for pid in with_dec.points:
        assert np.array_equal(with_dec.points[pid].position, without.points[pid].position)
        assert [o[:2] for o in with_dec.points[pid].observations] == [o[:2] for o in without.points[pid].observations]


def test_a_rejected_pair_leaves_the_map_untouched(gate, gpu_ctx, caplog):
    p1, p2 = SCENES["planar_rotation"]
    kp0, d0, kp1, d1, matches, q, t = planted_frames(dict(n=len(p1), pts1=p1, pts2=p2))
    wmap = PlainMap()
    with caplog.at_level(logging.INFO, logger="two_view_bootstrap"):
        assert gate.bootstrap_two_view_map(K, kp0, d0, kp1, d1, matches, ARGS, wmap) == (False, None, None)
    assert "[BOOTSTRAP] Pair rejected by gate; aborting." in caplog.text and len(wmap.points) == 0
    assert gate.bootstrap_two_view_map(K, kp0, d0, kp1, d1, matches[:49], ARGS, wmap) == (False, None, None)


def test_two_view_pose_still_raises_without_a_decision(gate, gpu_ctx):
    tvp = load_pkg("slam.core.two_view_pose")
    p1, p2 = SCENES["planar_parallax"]
    kp0, d0, kp1, d1, matches, q, t = planted_frames(dict(n=len(p1), pts1=p1, pts2=p2))
    with pytest.raises(NotImplementedError, match="homography"):
        tvp.bootstrap_two_view_map(K, kp0, d0, kp1, d1, matches, ARGS, PlainMap())


def test_the_gate_never_imports_cv2(gate):
    mod = sys.modules.get("cv2")
    assert mod is None or "cv2_stub" in repr(getattr(mod, "__spec__", "")) + repr(getattr(mod, "__file__", "")) or not hasattr(mod, "findHomography")
    src = open(gate.__file__).read()
    assert "import cv2" not in src
