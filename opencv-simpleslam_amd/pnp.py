"""PnP-RANSAC on the HIP backend.

Stands in for `cv2.solvePnPRansac(pts3d, pts2d, K, None, flags=cv2.SOLVEPNP_ITERATIVE, ...)` as
`solve_pnp_ransac` and `refine_pose_pnp` call it (slam/core/pnp_utils.py:307-341, :200-221).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native


def solve_pnp_ransac(pts3d, pts2d, K, reproj_px: float = 8.0, confidence: float = 0.99, max_iters: int = 100,
                     use_guess: bool = False, ctx=None):
    """pts3d [n,3], pts2d [n,2] (cast to float32 as the reference does), n >= 5.
    Returns (ok, Tcw [4,4] float64 or None, mask [n] bool, info dict).  `use_guess`: whether the caller passes a
    guess - OpenCV then starts its refinement from the last sample's pose, never from the guess's values."""
    ctx = ctx or _native.default_context()
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    if len(p3) != len(p2):
        raise ValueError("pts3d / pts2d length mismatch")
    n = len(p3)
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    guess = np.eye(4) if use_guess else None
    mask = np.zeros(n, np.uint8)
    T = np.zeros(16, np.float64)
    info = (C.c_int * 4)()
    P = _native.ptr
    _native.check(_native.lib().sslam_pnp_ransac_host(
        ctx.handle, n, P(p3), P(p2), P(Kd), P(guess), float(reproj_px), float(confidence), int(max_iters), P(mask),
        P(T), info), "sslam_pnp_ransac_host")
    meta = {"inliers": int(info[0]), "samples": int(info[1]), "sample": int(info[2]), "lm_iters": int(info[3])}
    if info[0] < 0:
        return False, None, np.zeros(n, bool), meta
    return True, T.reshape(4, 4), mask.astype(bool), meta


def solve_pnp_ransac_dev(ctx, n_points: int, kp_of_point_dev, pts3d_dev, kp_xy_dev, K, Tcw_out_dev, info_out_dev,
                         reproj_px: float = 8.0, confidence: float = 0.99, max_iters: int = 100,
                         use_guess: bool = False, mask_out_dev=None, n_out_dev=None):
    """Device-resident PnP on the association's output (`sslam_reproject_match_dev`): the `*_dev` arguments are device
    pointers (ints) - kp_of_point [n_points] int32, the map's points [n_points,3] float64, the keypoints [*,2] float32 -
    and the pose [16] float64, the inlier flags of the correspondences in map order, their count and info [4] int32
    stay on the device.  Enqueued on ctx's stream; nothing is read back here."""
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    guess = np.eye(4) if use_guess else None
    P = _native.ptr
    _native.check(_native.lib().sslam_pnp_ransac_dev(
        ctx.handle, int(n_points), P(kp_of_point_dev), P(pts3d_dev), P(kp_xy_dev), P(Kd), P(guess), float(reproj_px),
        float(confidence), int(max_iters), P(mask_out_dev), P(Tcw_out_dev), P(n_out_dev), P(info_out_dev)),
        "sslam_pnp_ransac_dev")
