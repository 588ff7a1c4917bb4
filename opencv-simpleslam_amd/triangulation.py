"""Two-view triangulation with the reference's gates on the HIP backend.

Stands in for the numeric body of `triangulate_between_kfs_2view` (slam/core/triangulation_utils.py:143-271):
`cv2.triangulatePoints`, the homogeneous test, the world-frame parallax, depth, cheirality and reprojection gates.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

# reason codes of include/sslam_hip.h, in the order the reference decides them
REASONS = ("kept", "invalid_w", "low_parallax", "bad_depth", "behind_cam", "high_reproj")
DIAG_FIELDS = ("parallax_deg", "z1", "z2", "e1", "e2")


def _reasons_dict(info):
    return {name: int(info[1 + k]) for k, name in enumerate(REASONS)}


def triangulate_2view(pts1, pts2, K, T1, T2, min_depth: float = 0.0, max_depth: float = 1e6,
                      use_parallax_gate: bool = True, parallax_min_deg: float = 2.0, reproj_px_max: float = 1.0,
                      want_diag: bool = False, ctx=None):
    """pts1, pts2: [n,2] matched pixels (cast to float32 as the reference holds them), K [3,3], T1 / T2 [4,4]
    camera-from-world of the two views.  Returns (X [kept,3] float64, kept_idx [kept] int32 match indices in order,
    reasons {name: count}, diag) - diag is None unless `want_diag`, else {"reason": int32 [n], "parallax_deg", "z1",
    "z2", "e1", "e2": float64 [n]}."""
    ctx = ctx or _native.default_context()
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("pts1 / pts2 length mismatch")
    n = len(p1)
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    T1d = np.ascontiguousarray(T1, np.float64).reshape(16)
    T2d = np.ascontiguousarray(T2, np.float64).reshape(16)
    X = np.zeros((max(n, 1), 3), np.float64)
    idx = np.zeros(max(n, 1), np.int32)
    info = (C.c_int32 * 8)()
    reason = np.zeros(max(n, 1), np.int32) if want_diag else None
    diag = np.zeros((max(n, 1), 5), np.float64) if want_diag else None
    P = _native.ptr
    _native.check(_native.lib().sslam_triangulate_2view_host(
        ctx.handle, n, P(p1), P(p2), P(Kd), P(T1d), P(T2d), float(min_depth), float(max_depth), int(bool(use_parallax_gate)),
        float(parallax_min_deg), float(reproj_px_max), P(X), P(idx), info, P(reason), P(diag)),
        "sslam_triangulate_2view_host")
    kept = int(info[0])
    out = None
    if want_diag:
        out = {"reason": reason[:n]}
        out.update({name: diag[:n, k] for k, name in enumerate(DIAG_FIELDS)})
    return X[:kept], idx[:kept], _reasons_dict(info), out


def triangulate_2view_dev(ctx, n_max: int, n_dev, xy1_dev, xy2_dev, ij_dev, K, T1_dev, T2_dev, X_out_dev, ij_out_dev,
                          info_out_dev, min_depth: float = 0.0, max_depth: float = 1e6, use_parallax_gate: bool = True,
                          parallax_min_deg: float = 2.0, reproj_px_max: float = 1.0, reason_out_dev=None,
                          diag_out_dev=None):
    """Device-resident triangulation on the output of `epipolar.filter_matches_dev`: the `*_dev` arguments are device
    pointers (ints) - the kept pairs [n_max,2] int32 and their count, the two frames' keypoints [*,2] float32, the two
    poses [16] float64 - and the points [n_max,3] float64, their pairs, info [8] int32 (and the per-match reasons /
    diagnostics when asked for) stay on the device.  Enqueued on ctx's stream; nothing is read back here."""
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    P = _native.ptr
    _native.check(_native.lib().sslam_triangulate_2view_dev(
        ctx.handle, int(n_max), P(n_dev), P(xy1_dev), P(xy2_dev), P(ij_dev), P(Kd), P(T1_dev), P(T2_dev), float(min_depth),
        float(max_depth), int(bool(use_parallax_gate)), float(parallax_min_deg), float(reproj_px_max), P(X_out_dev),
        P(ij_out_dev), P(info_out_dev), P(reason_out_dev), P(diag_out_dev)), "sslam_triangulate_2view_dev")
