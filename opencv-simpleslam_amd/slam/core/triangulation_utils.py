"""Drop-in for `triangulate_between_kfs_2view` of the reference's `slam/core/triangulation_utils.py` (:113-271) on the
HIP backend - map growth at every new keyframe (driver: main_revamped.py:562-585), with no `cv2` import anywhere on the
way: same signature, defaults and return value (the list of new point ids, `[]` when there is nothing to triangulate).

    match + filter      the overlay's `feature_matcher` / `filter_matches_ransac` (answered from the device-resident
                        records when the frame loop has just matched this pair: INTEGRATION section 2)
    triangulate + gate  `sslam_triangulate_2view_host`: cv2.triangulatePoints (:152), the homogeneous test (:153-159),
                        world-frame parallax (:54-77), depth / cheirality / reprojection gates (:189-249), fp64
    insert              one `world_map.add_points(X)` and the two `add_observation` calls per point, in kept order: the
                        ids, positions and observation order of the reference's point-by-point loop, on the overlay's
                        `Map` and on a reference-style dict-of-objects map alike

Each observation carries its own keyframe's descriptor, (prev.idx, i1, prev.desc[i1]) then (cur.idx, i2, cur.desc[i2]).
(The reference's `_map_add_point` (:80-108) hands the CURRENT keyframe's descriptor to both observations whenever the
current keyframe has descriptors; the per-view descriptor is what its observation list is built with (:253-256).)
The two `log.info` lines are kept: the parallax quartiles of the first 200 matches come from the kernel's per-match
diagnostics, the `[TRI] ... reasons:` summary from its counters.
"""
from __future__ import annotations

import logging

import numpy as np

from .features_utils import feature_matcher, filter_matches_ransac
from .multi_view_utils import multi_view_triangulation        # noqa: F401  (the reference's tests import it from here too)
from .two_view_bootstrap import pts_from_matches
from ... import triangulation as _tri

log_tri = logging.getLogger("triangulation")

_NO_DESC = np.zeros((1,), np.uint8)          # what the reference stores for an observation without a descriptor (:102)


def _insert_points(world_map, X, obs):
    """`obs`: per point ((kf_idx, kp_idx, desc), (kf_idx, kp_idx, desc)).  A failure removes the landmarks that did not
    get both observations, as the reference's `_map_add_point` removes a half-created one."""
    ids = list(world_map.add_points(np.asarray(X, dtype=np.float64).reshape(-1, 3)))
    if len(ids) != len(obs):
        raise RuntimeError("Map.add_points returned no ids.")
    done = 0
    try:
        for pid, pair in zip(ids, obs):
            mp = world_map.points[pid]
            for kf_idx, kp_idx, d in pair:
                mp.add_observation(int(kf_idx), int(kp_idx), d if d is not None else _NO_DESC)
            done += 1
    except Exception:
        for pid in ids[done:]:
            world_map.points.pop(pid, None)
        raise
    return ids


def triangulate_between_kfs_2view(
    args, K, world_map, prev_kf, cur_kf, matcher, log,
    use_parallax_gate: bool = True, parallax_min_deg: float = 2.0,
    reproj_px_max: float | None = None,
    debug_max_examples: int = 10
):
    """
    Triangulate new points from matches between two keyframes.

    Args:
      args: CLI args (uses min_depth, max_depth, ransac_thresh)
      K: (3,3) intrinsics
      world_map: Map (points: dict[int, MapPoint], add_points(...))
      prev_kf, cur_kf: Keyframe objects with .idx, .kps, .desc, .pose (Tcw)
      matcher: feature matcher from your pipeline
      log: logger (the 'triangulation' logger carries the per-match debug lines)
    """
    raw = feature_matcher(args, prev_kf.kps, cur_kf.kps, prev_kf.desc, cur_kf.desc, matcher)
    matches = filter_matches_ransac(prev_kf.kps, cur_kf.kps, raw, args.ransac_thresh)

    log.info("[TRI] KF %d→%d  raw=%d  after_RANSAC=%d (th=%.2f px)",
             prev_kf.idx, cur_kf.idx, len(raw), len(matches), float(args.ransac_thresh))
    log_tri.debug("prev_kf: idx=%d, kps=%d | cur_kf: idx=%d, kps=%d",
                  prev_kf.idx, len(prev_kf.kps), cur_kf.idx, len(cur_kf.kps))

    if len(matches) == 0:
        log.info("[TRI] No matches to triangulate for KFs %d→%d.", prev_kf.idx, cur_kf.idx)
        return []

    pts1, pts2 = pts_from_matches(prev_kf.kps, cur_kf.kps, matches)
    if reproj_px_max is None:
        reproj_px_max = float(args.ransac_thresh)
    min_d = float(getattr(args, "min_depth", 0.0))
    max_d = float(getattr(args, "max_depth", 1e6))

    X, kept_idx, reasons, diag = _tri.triangulate_2view(
        pts1, pts2, np.asarray(K, np.float64), np.asarray(prev_kf.pose, np.float64), np.asarray(cur_kf.pose, np.float64),
        min_depth=min_d, max_depth=max_d, use_parallax_gate=use_parallax_gate, parallax_min_deg=float(parallax_min_deg),
        reproj_px_max=float(reproj_px_max), want_diag=True)
    n_valid = len(matches) - reasons["invalid_w"]
    if n_valid == 0:
        log.warning("[TRI] cv2.triangulatePoints produced no finite depths (w).")
        return []

    if use_parallax_gate:
        sample_parallaxes = diag["parallax_deg"][:200]
        if sample_parallaxes.size:
            log.info("[TRI] Parallax(sample of %d): med=%.2f°, p25=%.2f°, p75=%.2f°",
                     len(sample_parallaxes),
                     float(np.median(sample_parallaxes)),
                     float(np.percentile(sample_parallaxes, 25)),
                     float(np.percentile(sample_parallaxes, 75)))

    if log_tri.isEnabledFor(logging.DEBUG):
        names = _tri.REASONS
        for m_idx in np.flatnonzero(diag["reason"] != 1)[:max(int(debug_max_examples), 0)]:
            m = matches[m_idx]
            log_tri.debug("%s  match=(%d,%d)  par=%.2f°  z1=%.3f z2=%.3f  e1=%.2f e2=%.2f", names[diag["reason"][m_idx]],
                          m.queryIdx, m.trainIdx, diag["parallax_deg"][m_idx] if use_parallax_gate else -1.0,
                          diag["z1"][m_idx], diag["z2"][m_idx], diag["e1"][m_idx], diag["e2"][m_idx])

    has1, has2 = prev_kf.desc is not None, cur_kf.desc is not None
    obs = []
    for m_idx in kept_idx.tolist():
        m = matches[m_idx]
        i1, i2 = m.queryIdx, m.trainIdx
        obs.append(((prev_kf.idx, i1, prev_kf.desc[i1] if has1 else None),
                    (cur_kf.idx, i2, cur_kf.desc[i2] if has2 else None)))
    kept_ids = _insert_points(world_map, X, obs) if len(obs) else []

    shown = {k: v for k, v in reasons.items() if v and k != "invalid_w"}
    log.info("[TRI] KF %d<->%d: kept=%d of %d valid w  | reasons: %s  (reproj<=%.1fpx, depth∈[%.2f,%.2f])",
             prev_kf.idx, cur_kf.idx, len(kept_ids), int(n_valid),
             shown, reproj_px_max, min_d, max_d)

    return kept_ids
