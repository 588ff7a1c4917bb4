"""The F/E leg of the reference's `slam/core/two_view_bootstrap.py` on the HIP backend, with no `cv2` on its import path:
the reference's names, signatures, defaults and log lines for

    recover_pose_from_fundamental (:202-220)   E = K^T F K, `cv2.recoverPose` -> `relative_pose.recover_pose`
                                               (`sslam_recover_pose_host`), then the validation below
    triangulation_metrics (:127-156)           `sslam_two_view_metrics_host`
    validate_two_view_pose (:158-170)          the three thresholds on those metrics
    _triangulate_points_cv (:314-326)          the same entry's points
    bootstrap_two_view_map (:328-411)          the map of an accepted pair, given its `TwoViewDecision`

and, in plain numpy, the residuals and scores around them (`sampson_distances_F`, `symmetric_transfer_errors_H`,
`truncated_inlier_score`, `compute_model_scores`; `cv2.convertPointsToHomogeneous` is appending a 1) and the data types.

This is a module of its own because the overlay's `two_view_bootstrap` holds `pts_from_matches` and nothing else (a driver
without OpenCV installs that one whole); these names are patched into the REFERENCE's `two_view_bootstrap` one by one
(INTEGRATION section 2); the gate itself - homography RANSAC, `decomposeHomographyMat`,
`recover_pose_from_homography`, `evaluate_two_view_bootstrap*` - is `two_view_gate`, which imports this module.  This
module's `bootstrap_two_view_map` needs its `decision`: without one it raises (the gate's function of that name runs the gate).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from enum import Enum, auto
from typing import Optional, Tuple

import numpy as np

from .pose_utils import _pose_rt_to_homogenous
from .two_view_bootstrap import pts_from_matches
from ... import relative_pose as _rp

logger = logging.getLogger("two_view_bootstrap")


class TwoViewModel(Enum):
    HOMOGRAPHY = auto()
    FUNDAMENTAL = auto()


@dataclass
class InitParams:
    ransac_px: float = 1.5
    chi2_H: float = 5.99
    chi2_F: float = 3.84
    min_pts_for_tests: int = 60
    min_posdepth: float = 0.90
    min_parallax_deg: float = 1.5
    score_ratio_H: float = 0.45


@dataclass
class TwoViewScores:
    S_H: float
    S_F: float
    ratio_H: float


@dataclass
class TwoViewPose:
    model: TwoViewModel
    R: np.ndarray
    t: np.ndarray
    posdepth: float
    parallax_deg: float


@dataclass
class TwoViewDecision:
    pose: TwoViewPose
    inlier_mask: np.ndarray


def _homogeneous(pts):
    """cv2.convertPointsToHomogeneous(pts)[:, 0, :]: a 1 appended, the dtype kept"""
    pts = np.asarray(pts)
    return np.concatenate([pts, np.ones((len(pts), 1), pts.dtype)], axis=1)


def symmetric_transfer_errors_H(H: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray) -> np.ndarray:
    """Squared symmetric transfer error for a homography H."""
    x1 = _homogeneous(pts_ref).T
    x2 = _homogeneous(pts_cur).T
    Hx1 = H @ x1
    Hinv = np.linalg.inv(H)
    Hinvx2 = Hinv @ x2
    p2 = (Hx1[:2] / (Hx1[2] + 1e-12)).T
    p1 = (Hinvx2[:2] / (Hinvx2[2] + 1e-12)).T
    e12 = np.sum((pts_cur - p2) ** 2, axis=1)
    e21 = np.sum((pts_ref - p1) ** 2, axis=1)
    d2 = e12 + e21
    logger.debug("H symmetric errors: med=%.3f px^2, 75p=%.3f px^2", float(np.median(d2)), float(np.percentile(d2, 75)))
    return d2


def sampson_distances_F(F: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray) -> np.ndarray:
    """Sampson distance for a fundamental matrix F."""
    x1 = _homogeneous(pts_ref)
    x2 = _homogeneous(pts_cur)
    Fx1 = (F @ x1.T).T
    Ftx2 = (F.T @ x2.T).T
    num = (np.sum(x2 * (F @ x1.T).T, axis=1)) ** 2
    den = Fx1[:, 0] ** 2 + Fx1[:, 1] ** 2 + Ftx2[:, 0] ** 2 + Ftx2[:, 1] ** 2 + 1e-12
    d2 = num / den
    logger.debug("F Sampson distances: med=%.3f, 75p=%.3f", float(np.median(d2)), float(np.percentile(d2, 75)))
    return d2


def truncated_inlier_score(residuals_sq: np.ndarray, chi2_cutoff: float) -> float:
    """ORB-style truncated linear score: sum(max(0, chi2 - d^2))."""
    S = float(np.maximum(0.0, chi2_cutoff - residuals_sq).sum())
    logger.debug("Truncated score @chi2=%.2f → S=%.1f (inlier-like=%d/%d)",
                 chi2_cutoff, S, int((residuals_sq < chi2_cutoff).sum()), residuals_sq.size)
    return S


def compute_model_scores(H: Optional[np.ndarray], F: Optional[np.ndarray], pts_ref: np.ndarray, pts_cur: np.ndarray,
                         params: InitParams) -> TwoViewScores:
    S_H = truncated_inlier_score(symmetric_transfer_errors_H(H, pts_ref, pts_cur), params.chi2_H) if H is not None else 0.0
    S_F = truncated_inlier_score(sampson_distances_F(F, pts_ref, pts_cur), params.chi2_F) if F is not None else 0.0
    ratio_H = S_H / (S_H + S_F + 1e-12)
    logger.info("Scores  S_H=%.1f  S_F=%.1f  → ratio_H=%.3f", S_H, S_F, ratio_H)
    return TwoViewScores(S_H=S_H, S_F=S_F, ratio_H=ratio_H)


def triangulation_metrics(K: np.ndarray, R: np.ndarray, t: np.ndarray, pts_ref: np.ndarray,
                          pts_cur: np.ndarray) -> Tuple[float, float, int]:
    """Return (posdepth_fraction, median_parallax_deg, N_points_used)."""
    if len(pts_ref) < 2:
        return 0.0, 0.0, 0
    posdepth, parallax_deg, N = _rp.two_view_metrics(K, R, t, pts_ref, pts_cur)
    logger.debug("Triangulation metrics: posdepth=%.3f  parallax_med=%.2f°  N=%d", posdepth, parallax_deg, N)
    return posdepth, parallax_deg, N


def validate_two_view_pose(K: np.ndarray, R: np.ndarray, t: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray,
                           params: InitParams) -> Tuple[bool, float, float]:
    posdepth, parallax_deg, N = triangulation_metrics(K, R, t, pts_ref, pts_cur)
    ok = (N >= params.min_pts_for_tests and
          posdepth >= params.min_posdepth and
          parallax_deg >= params.min_parallax_deg)
    logger.info("Validate pose: ok=%s  N=%d  posdepth=%.3f  parallax=%.2f°  (req: N≥%d, pos≥%.2f, par≥%.2f°)",
                ok, N, posdepth, parallax_deg, params.min_pts_for_tests, params.min_posdepth, params.min_parallax_deg)
    return ok, posdepth, parallax_deg


def recover_pose_from_fundamental(K: np.ndarray, F: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray,
                                  params: InitParams) -> Optional[TwoViewPose]:
    E = K.T @ F @ K
    ok, R, t, mask = _rp.recover_pose(E, pts_ref, pts_cur, K)
    ninl = int(np.count_nonzero(mask)) if mask is not None else 0
    logger.info("recoverPose(E): ok=%s  inliers=%d", ok, ninl)
    if not ok or mask is None or ninl < params.min_pts_for_tests:
        logger.info("F/E rejected: not enough inliers for validation.")
        return None
    inl = mask.ravel().astype(bool)
    ok2, pd, ang = validate_two_view_pose(K, R, t, pts_ref[inl], pts_cur[inl], params)
    if ok2:
        logger.info("F/E accepted: posdepth=%.3f  parallax=%.2f°", pd, ang)
        return TwoViewPose(TwoViewModel.FUNDAMENTAL, R, t, pd, ang)
    logger.info("F/E rejected after validation.")
    return None


def _triangulate_with_depths(K, R, t, pts_ref, pts_cur):
    if len(pts_ref) == 0:
        return np.empty((0, 3)), np.empty((0, 2))
    return _rp.two_view_metrics(K, R, t, pts_ref, pts_cur, want_points=True)[3:5]


def _triangulate_points_cv(K: np.ndarray, R: np.ndarray, t: np.ndarray, pts_ref: np.ndarray,
                           pts_cur: np.ndarray) -> np.ndarray:
    """Triangulate in the reference camera frame (world := cam0)."""
    return _triangulate_with_depths(K, R, t, pts_ref, pts_cur)[0]


def bootstrap_two_view_map(K: np.ndarray, kp_ref, desc_ref, kp_cur, desc_cur, matches, args, world_map,
                           params: InitParams = InitParams(), decision: Optional[TwoViewDecision] = None):
    """
    Build the initial map from one accepted two-view pair.

    `decision` is what the gate (`evaluate_two_view_bootstrap_with_masks`) returned.  The gate's homography leg is out of
    scope of this backend, so a call without a decision raises NotImplementedError instead of running half a gate.

    Side effects:
      - Triangulates, depth-filters, and adds points + observations (KF0 = I, KF1 = [R|t]).

    Returns: (success: bool, T0_cw: 4x4, T1_cw: 4x4)
    """
    if len(matches) < 50:
        logger.info("[BOOTSTRAP] Not enough matches for init (%d < 50).", len(matches))
        return False, None, None

    pts_ref, pts_cur = pts_from_matches(kp_ref, kp_cur, matches)

    if decision is None:
        raise NotImplementedError(
            "bootstrap_two_view_map without a decision would run evaluate_two_view_bootstrap_with_masks, whose homography leg "
            "(findHomography RANSAC, decomposeHomographyMat) is out of scope of this backend: run the reference's gate and "
            "pass its TwoViewDecision")
    pose = decision.pose
    mask = decision.inlier_mask.astype(bool)
    ninl = int(mask.sum())
    logger.info("[BOOTSTRAP] Using model=%s with %d inliers.", pose.model.name, ninl)

    if ninl < params.min_pts_for_tests:
        logger.info("[BOOTSTRAP] Too few inliers after gating (%d < %d).", ninl, params.min_pts_for_tests)
        return False, None, None

    # triangulate once on the final inliers; the two depths come with the points
    p0 = pts_ref[mask]
    p1 = pts_cur[mask]
    Xw, z = _triangulate_with_depths(K, pose.R, pose.t, p0, p1)
    z0, z1 = z[:, 0], z[:, 1]

    min_d = float(getattr(args, "min_depth", 0.0))
    max_d = float(getattr(args, "max_depth", 1e6))
    ok = (z0 > min_d) & (z0 < max_d) & (z1 > min_d) & (z1 < max_d)
    Xw = Xw[ok]
    logger.info("[BOOTSTRAP] Triangulated=%d  kept=%d after depth filter [%.3g, %.3g].", len(p0), len(Xw), min_d, max_d)
    if len(Xw) < 80:
        logger.info("[BOOTSTRAP] Not enough 3D points to seed the map (%d < 80).", len(Xw))
        return False, None, None

    T0_cw = np.eye(4, dtype=np.float64)
    T1_cw = _pose_rt_to_homogenous(pose.R, pose.t)

    cols = np.full((len(Xw), 3), 0.7, dtype=np.float32)  # grey
    ids = world_map.add_points(Xw, cols, keyframe_idx=0)

    qidx = np.int32([m.queryIdx for m in matches])
    tidx = np.int32([m.trainIdx for m in matches])
    sel = np.where(mask)[0][ok]  # indices into 'matches' of inliers that passed depth

    for pid, i0, i1 in zip(ids, qidx[sel], tidx[sel]):
        world_map.points[pid].add_observation(0, i0, desc_ref[i0])  # KF0
        world_map.points[pid].add_observation(1, i1, desc_cur[i1])  # KF1

    logger.info("[BOOTSTRAP] Map initialised: %d landmarks, 2 keyframes (KF0=I, KF1=[R|t]).", len(ids))
    return True, T0_cw, T1_cw
