"""Two-view relative pose on the HIP backend: `cv2.recoverPose` and the reference's triangulation-based validation.

Stands in for `cv2.recoverPose(E, pts_ref, pts_cur, K)` (slam/core/two_view_bootstrap.py:208, slam/monocular/
main_revamped.py:514) and for the numeric bodies of `triangulation_metrics` (:127-156) and `_triangulate_points_cv`
(:314-326).  Parity with cv2 is unpinned (tests/relative_pose_ref.py restates both).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native


def _points(pts1, pts2):
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("pts1 / pts2 length mismatch")
    return p1, p2


def _bytes(flags, n, what):
    if flags is None:
        return None
    b = np.asarray(flags)
    b = np.ascontiguousarray(b.astype(np.uint8) if b.dtype != np.bool_ else b.view(np.uint8)).reshape(-1)
    if len(b) != n:
        raise ValueError(f"{what} has {len(b)} entries for {n} matches")
    return b


def recover_pose(E, pts1, pts2, K, distance_thresh: float = 50.0, mask=None, ctx=None, want_info: bool = False):
    """cv2.recoverPose(E, pts1, pts2, K[, distanceThresh][, mask]) -> (good, R [3,3], t [3,1], mask uint8 [n,1]).
    pts1, pts2: [n,2] matched pixels (cast to float32 as the reference holds them).  `mask` (optional, [n] or [n,1]
    uint8): only its non-zero matches can stay, and the result is `mask & (255 where the winner keeps the match)` - a
    0/1 mask stays 0/1; without it the result is 255 / 0.  `want_info` appends {"winner": 0..3, "counts": [4]}."""
    ctx = ctx or _native.default_context()
    p1, p2 = _points(pts1, pts2)
    n = len(p1)
    Ed = np.ascontiguousarray(E, np.float64).reshape(9)
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    m_in = _bytes(mask, n, "mask")
    R = np.zeros(9, np.float64)
    t = np.zeros(3, np.float64)
    m_out = np.zeros(max(n, 1), np.uint8)
    info = (C.c_int32 * 8)()
    P = _native.ptr
    _native.check(_native.lib().sslam_recover_pose_host(
        ctx.handle, n, P(p1), P(p2), P(Ed), P(Kd), float(distance_thresh), P(m_in), P(R), P(t), P(m_out), info),
        "sslam_recover_pose_host")
    out = (int(info[0]), R.reshape(3, 3), t.reshape(3, 1), m_out[:n].reshape(-1, 1))
    if want_info:
        out += ({"winner": int(info[2]), "counts": [int(info[3 + k]) for k in range(4)]},)
    return out


def two_view_metrics(K, R, t, pts1, pts2, sel=None, want_points: bool = False, ctx=None, want_info: bool = False):
    """`triangulation_metrics(K, R, t, pts1[sel], pts2[sel])` -> (posdepth, parallax_deg, N); N = 0 (and metrics 0, 0)
    when fewer than two matches are selected.  `sel`: [n] flags (bool or bytes, non-zero selects), None = every match.
    `want_points` appends X [N',3] (`_triangulate_points_cv` of the selected matches, in order) and z [N',2] (their
    depths in the two views), N' = the selected count; `want_info` appends {"in_front": the count behind posdepth}."""
    ctx = ctx or _native.default_context()
    p1, p2 = _points(pts1, pts2)
    n = len(p1)
    s = _bytes(sel, n, "sel")
    n_sel = n if s is None else int(np.count_nonzero(s))
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    Rd = np.ascontiguousarray(R, np.float64).reshape(9)
    td = np.ascontiguousarray(t, np.float64).reshape(3)
    metrics = np.zeros(2, np.float64)
    info = (C.c_int32 * 4)()
    X = np.zeros((max(n_sel, 1), 3), np.float64) if want_points else None
    z = np.zeros((max(n_sel, 1), 2), np.float64) if want_points else None
    P = _native.ptr
    _native.check(_native.lib().sslam_two_view_metrics_host(
        ctx.handle, n, P(p1), P(p2), P(s), P(Kd), P(Rd), P(td), P(metrics), info, P(X), P(z)),
        "sslam_two_view_metrics_host")
    out = (float(metrics[0]), float(metrics[1]), int(info[0]))
    if want_points:
        out += (X[:n_sel], z[:n_sel])
    if want_info:
        out += ({"in_front": int(info[1])},)
    return out


def relative_pose_2d2d(pts0, pts1, K, thresh: float, prob: float = 0.999, ctx=None):
    """The tracking-lost fallback's two calls chained (slam/monocular/main_revamped.py:512-514, main.py:402, main4.py:457):
    `E, inlE = cv2.findEssentialMat(pts0, pts1, K, cv2.RANSAC, prob, thresh)`, then, when there is an E whose mask has at
    least five ones, `cv2.recoverPose(E, pts0, pts1, K, mask=inlE)`.  Returns (inliers, R [3,3], t [3,1], mask uint8
    [n,1]), or (0, None, None, None) when the reference's guard fails.  Exactly five matches give a stack of models that
    cv2.recoverPose does not take: the empty result as well.  The pose scaling and composition stay the driver's."""
    from . import essential
    E, inl, _ = essential.find_essential_mat_ransac(pts0, pts1, K, prob, thresh, ctx=ctx)
    if E is None or inl is None or int(inl.sum()) < 5 or E.shape != (3, 3):
        return 0, None, None, None
    return recover_pose(E, pts0, pts1, K, mask=inl, ctx=ctx)
