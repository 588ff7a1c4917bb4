"""The rest of the reference's `slam/core/two_view_bootstrap.py` on the HIP backend, with no `cv2` on its import path: the
two-view gate that competes a homography against a fundamental matrix, in the reference's names, signatures, defaults and
log lines.

    decompose_homography_mat                     `cv2.decomposeHomographyMat(H, K)` in numpy (3 x 3 algebra, no kernel)
    recover_pose_from_homography (:174-200)      its candidates through `two_view_pose.validate_two_view_pose`
    evaluate_two_view_bootstrap (:224-261)       `cv2.findHomography` -> `homography.find_homography_ransac`
                                                 (`sslam_homography_ransac_host`), `cv2.findFundamentalMat` ->
                                                 `epipolar.find_fundamental_ransac` (`sslam_fmat_ransac_host`)
    _final_inlier_mask_for_model (:265-297)
    evaluate_two_view_bootstrap_with_masks (:300-310)
    bootstrap_two_view_map (:328-411)            runs the gate when it is given no decision, then hands over to
                                                 `two_view_pose.bootstrap_two_view_map`

The data types, the numpy scores and the F/E leg are `two_view_pose`'s (a `TwoViewPose` built here is that module's class).
INTEGRATION section 2 patches the reference's module from the two overlay modules.

Deviations from the reference:
  * fewer than 8 matches: the gate logs and returns None.  cv2 would still try a homography on 4 - 7 matches, but the
    F entry needs 8, `min_pts_for_tests` is 60 and `bootstrap_two_view_map` wants 50 matches: no such pair can start a map;
  * both RANSACs are seeded, so running them again returns the first run's answer: the masks of the first run are kept for
    `evaluate_two_view_bootstrap_with_masks` instead of being computed again (only `recoverPose` runs again, for its mask);
  * `decompose_homography_mat` restates OpenCV's `HomographyDecompInria` (Malis and Vargas, "Deeper understanding of the
    homography decomposition for vision-based control", INRIA RR-6303) from memory: parity with cv2 is unpinned, the
    properties are tested (tests/test_homography_decomp.py).  One step is added: Hn is negated when its determinant is
    negative, so that a homography handed over with the other sign still decomposes into proper rotations.
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np

from . import two_view_pose as _tvp
from .two_view_bootstrap import pts_from_matches
from .two_view_pose import (InitParams, TwoViewDecision, TwoViewModel, TwoViewPose, TwoViewScores,  # noqa: F401
                            compute_model_scores, recover_pose_from_fundamental, sampson_distances_F,
                            symmetric_transfer_errors_H, triangulation_metrics, truncated_inlier_score,
                            validate_two_view_pose)
from ... import epipolar as _ep
from ... import homography as _hg
from ... import relative_pose as _rp

logger = logging.getLogger("two_view_bootstrap")

MIN_MATCHES = 8          # what the F entry needs


def _opposite_of_minor(M, row, col):
    x1 = 1 if col == 0 else 0
    x2 = 1 if col == 2 else 2
    y1 = 1 if row == 0 else 0
    y2 = 1 if row == 2 else 2
    return M[y1, x2] * M[y2, x1] - M[y1, x1] * M[y2, x2]


def _signd(x):
    return 1.0 if x >= 0 else -1.0


def decompose_homography_mat(H, K):
    """`cv2.decomposeHomographyMat(H, K)` -> (number of solutions, Rs, ts, normals): lists of [3,3], [3,1], [3,1] arrays.
    Hn = K^-1 H K divided by its middle singular value; S = Hn^T Hn - I; one solution (R = Hn, t = 0, n = 0) when the
    largest absolute row sum of S is below 0.001 (a pure rotation), else the four of Malis and Vargas' analytical method."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    K = np.asarray(K, np.float64).reshape(3, 3)
    Hn = np.linalg.inv(K) @ H @ K
    Hn = Hn / np.linalg.svd(Hn, compute_uv=False)[1]
    if np.linalg.det(Hn) < 0:          # H and -H are one homography: take the sign whose rotations are proper
        Hn = -Hn
    S = Hn.T @ Hn - np.eye(3)
    if np.abs(S).sum(axis=1).max() < 0.001:
        return 1, [Hn.copy()], [np.zeros((3, 1))], [np.zeros((3, 1))]
    M00, M11, M22 = (_opposite_of_minor(S, i, i) for i in range(3))
    rtM00, rtM11, rtM22 = (np.sqrt(max(v, 0.0)) for v in (M00, M11, M22))
    e12 = _signd(_opposite_of_minor(S, 1, 2))
    e02 = _signd(_opposite_of_minor(S, 0, 2))
    e01 = _signd(_opposite_of_minor(S, 0, 1))
    nS = [abs(S[0, 0]), abs(S[1, 1]), abs(S[2, 2])]
    indx = 0
    if nS[0] < nS[1]:
        indx = 1
        if nS[1] < nS[2]:
            indx = 2
    elif nS[0] < nS[2]:
        indx = 2
    if indx == 0:
        npa = np.array([S[0, 0], S[0, 1] + rtM22, S[0, 2] + e12 * rtM11])
        npb = np.array([S[0, 0], S[0, 1] - rtM22, S[0, 2] - e12 * rtM11])
    elif indx == 1:
        npa = np.array([S[0, 1] + rtM22, S[1, 1], S[1, 2] - e02 * rtM00])
        npb = np.array([S[0, 1] - rtM22, S[1, 1], S[1, 2] + e02 * rtM00])
    else:
        npa = np.array([S[0, 2] + e01 * rtM11, S[1, 2] + rtM00, S[2, 2]])
        npb = np.array([S[0, 2] - e01 * rtM11, S[1, 2] - rtM00, S[2, 2]])
    traceS = S[0, 0] + S[1, 1] + S[2, 2]
    v = 2.0 * np.sqrt(max(1 + traceS - M00 - M11 - M22, 0.0))
    ESii = _signd(S[indx, indx])
    r = np.sqrt(max(2 + traceS + v, 0.0))
    n_t = np.sqrt(max(2 + traceS - v, 0.0))
    na = npa / np.linalg.norm(npa)
    nb = npb / np.linalg.norm(npb)
    half_nt = 0.5 * n_t
    esii_t_r = ESii * r
    ta_star = half_nt * (esii_t_r * nb - n_t * na)
    tb_star = half_nt * (esii_t_r * na - n_t * nb)
    Ra = Hn @ (np.eye(3) - (2.0 / v) * np.outer(ta_star, na))
    Rb = Hn @ (np.eye(3) - (2.0 / v) * np.outer(tb_star, nb))
    ta, tb = Ra @ ta_star, Rb @ tb_star
    col = lambda x: np.asarray(x, np.float64).reshape(3, 1).copy()
    Rs = [Ra.copy(), Ra.copy(), Rb.copy(), Rb.copy()]
    ts = [col(ta), col(-ta), col(tb), col(-tb)]
    ns = [col(na), col(-na), col(nb), col(-nb)]
    return 4, Rs, ts, ns


def recover_pose_from_homography(K: np.ndarray, H: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray,
                                 params: InitParams) -> Optional[TwoViewPose]:
    ret = decompose_homography_mat(H, K)
    if ret is None or len(ret) < 4 or not all(np.isfinite(R).all() and np.isfinite(t).all() for R, t in zip(ret[1], ret[2])):
        logger.warning("Homography decomposition failed.")
        return None
    _, Rs, ts, _ = ret
    logger.info("Homography decomposition → %d candidates", len(Rs))
    best: Optional[TwoViewPose] = None
    best_key = (-1.0, -1.0)  # maximize (posdepth, parallax)

    for idx, (R, t) in enumerate(zip(Rs, ts)):
        t = t.reshape(3, 1)
        t = t / (np.linalg.norm(t) + 1e-12)  # scale-free
        ok, pd, ang = validate_two_view_pose(K, R, t, pts_ref, pts_cur, params)
        logger.info("  H-cand #%d: ok=%s  posdepth=%.3f  parallax=%.2f°", idx, ok, pd, ang)
        if ok and (pd, ang) > best_key:
            best = TwoViewPose(TwoViewModel.HOMOGRAPHY, R, t, pd, ang)
            best_key = (pd, ang)
    if best is None:
        logger.info("No homography candidate passed validation.")
    else:
        logger.info("Chosen H-candidate: posdepth=%.3f  parallax=%.2f°", best.posdepth, best.parallax_deg)
    return best


def _evaluate(K, pts_ref, pts_cur, params):
    """`evaluate_two_view_bootstrap`, returning (pose or None, (H, maskH, F, maskF) of its two RANSACs or None)"""
    pts_ref = np.asarray(pts_ref, np.float32).reshape(-1, 2)
    pts_cur = np.asarray(pts_cur, np.float32).reshape(-1, 2)
    if len(pts_ref) < MIN_MATCHES:
        logger.info("Pair rejected: %d matches, the gate needs at least %d.", len(pts_ref), MIN_MATCHES)
        return None, None
    H, maskH, _ = _hg.find_homography_ransac(pts_ref, pts_cur, params.ransac_px)
    F, maskF, _ = _ep.find_fundamental_ransac(pts_ref, pts_cur, params.ransac_px, 0.99, 1000)
    first = (H, maskH, F, maskF)

    nH = int(maskH.sum()) if (maskH is not None and maskH.size) else 0
    nF = int(maskF.sum()) if (maskF is not None and maskF.size) else 0
    logger.info("RANSAC: H-inliers=%d (th=%.2f px), F-inliers=%d (th=%.2f px)", nH, params.ransac_px, nF, params.ransac_px)

    if H is None and F is None:
        logger.info("Both H and F estimation failed → reject pair.")
        return None, first

    scores = compute_model_scores(H, F, pts_ref, pts_cur, params)

    if scores.ratio_H > params.score_ratio_H and H is not None:
        logger.info("Model selection: prefer HOMOGRAPHY (ratio_H=%.3f > %.2f)", scores.ratio_H, params.score_ratio_H)
        pose = recover_pose_from_homography(K, H, pts_ref, pts_cur, params)
        if pose is not None:
            return pose, first
        logger.info("H path failed validation → trying F/E fallback.")
    else:
        logger.info("Model selection: prefer FUNDAMENTAL/E (ratio_H=%.3f ≤ %.2f)", scores.ratio_H, params.score_ratio_H)

    if F is not None:
        pose = recover_pose_from_fundamental(K, F, pts_ref, pts_cur, params)
        if pose is not None:
            return pose, first

    logger.info("Pair rejected: ambiguous or too weak for initialization.")
    return None, first


def evaluate_two_view_bootstrap(K: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray,
                                params: InitParams = InitParams()) -> Optional[TwoViewPose]:
    """Pick H vs F with comparable residuals, then recover a valid (R,t)."""
    return _evaluate(K, pts_ref, pts_cur, params)[0]


def _final_inlier_mask_for_model(model: TwoViewModel, pts_ref: np.ndarray, pts_cur: np.ndarray, K: np.ndarray,
                                 R: np.ndarray, t: np.ndarray, ransac_px: float, _first=None) -> np.ndarray:
    """
    Make a robust inlier mask aligned with pts_ref/pts_cur for the chosen model.
    F/E: intersect F-RANSAC inliers with recoverPose mask.
    H:   use H-RANSAC inliers.
    `_first`: the (H, maskH, F, maskF) of the gate's own run, which a second run of the seeded RANSACs would return again.
    """
    def _as_bool(m):
        if m is None:
            return None
        v = np.asarray(m).ravel()
        return (v.astype(np.uint8) > 0)

    pts_ref = np.asarray(pts_ref, np.float32).reshape(-1, 2)
    pts_cur = np.asarray(pts_cur, np.float32).reshape(-1, 2)
    if model is TwoViewModel.FUNDAMENTAL:
        F, maskF = _first[2:4] if _first is not None else _ep.find_fundamental_ransac(pts_ref, pts_cur, ransac_px, 0.99, 1000)[:2]
        if F is None or maskF is None:
            return np.zeros(len(pts_ref), dtype=bool)
        E = K.T @ F @ K
        _, _, _, maskRP = _rp.recover_pose(E, pts_ref, pts_cur, K)
        mF = _as_bool(maskF)
        mRP = _as_bool(maskRP)
        return mF if mRP is None else (mF & mRP)
    H, maskH = _first[0:2] if _first is not None else _hg.find_homography_ransac(pts_ref, pts_cur, ransac_px)[:2]
    if H is None or maskH is None:
        return np.zeros(len(pts_ref), dtype=bool)
    return _as_bool(maskH)


def evaluate_two_view_bootstrap_with_masks(K: np.ndarray, pts_ref: np.ndarray, pts_cur: np.ndarray,
                                           params: InitParams = InitParams()) -> Optional[TwoViewDecision]:
    """Same as evaluate_two_view_bootstrap, but also returns a robust inlier mask."""
    pose, first = _evaluate(K, pts_ref, pts_cur, params)
    if pose is None:
        return None
    mask = _final_inlier_mask_for_model(pose.model, pts_ref, pts_cur, K, pose.R, pose.t, params.ransac_px, _first=first)
    return TwoViewDecision(pose=pose, inlier_mask=mask.astype(bool))


def bootstrap_two_view_map(K: np.ndarray, kp_ref, desc_ref, kp_cur, desc_cur, matches, args, world_map,
                           params: InitParams = InitParams(), decision: Optional[TwoViewDecision] = None):
    """
    Build the initial map from one accepted two-view pair.

    If you already ran the gate, pass its 'decision' to avoid recomputation.
    Otherwise this function will run the gate internally.

    Returns: (success: bool, T0_cw: 4x4, T1_cw: 4x4)
    """
    if len(matches) < 50:
        logger.info("[BOOTSTRAP] Not enough matches for init (%d < 50).", len(matches))
        return False, None, None
    if decision is None:
        pts_ref, pts_cur = pts_from_matches(kp_ref, kp_cur, matches)
        decision = evaluate_two_view_bootstrap_with_masks(K, pts_ref, pts_cur, params)
        if decision is None:
            logger.info("[BOOTSTRAP] Pair rejected by gate; aborting.")
            return False, None, None
    return _tvp.bootstrap_two_view_map(K, kp_ref, desc_ref, kp_cur, desc_cur, matches, args, world_map, params, decision)
