"""N-view triangulation of feature tracks with the gates of the reference's CLI on the HIP backend.

The numeric body of `multi_view_triangulation` / `MultiViewTriangulator` (slam/core/multi_view_utils.py): per track the
DLT over all of its observations, the homogeneous test, the depth window, cheirality and the MEAN reprojection error
(`--mvt_rep_err`: "Max mean reprojection error (px) for multi-view triangulation").  include/sslam_hip.h states the
definition; the module itself was lost upstream, so parity with it is unpinned.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

# reason codes of include/sslam_hip.h, in the order they are decided
REASONS = ("kept", "too_few_views", "invalid_w", "bad_depth", "behind_cam", "high_reproj")
DIAG_FIELDS = ("mean_err", "z_min", "z_max")


def triangulate_tracks(K, Tcw, track_off, obs_view, obs_uv, min_depth: float = 0.40, max_depth: float = 100.0,
                       max_rep_err: float = 2.0, want_diag: bool = False, ctx=None):
    """K [3,3]; Tcw [F,4,4] camera-from-world of the F views; the observations as CSR: track i owns observations
    track_off[i] .. track_off[i+1]-1, observation o is pixel obs_uv[o] (cast to float32) in view obs_view[o].
    ONE device call for all tracks.  Returns (X [kept,3] float64, kept_idx [kept] int32 track indices in order,
    reasons {name: count}, diag) - diag is None unless `want_diag`, else {"reason": int32 [n], "mean_err", "z_min",
    "z_max": float64 [n]}."""
    ctx = ctx or _native.default_context()
    off = np.ascontiguousarray(track_off, np.int32).reshape(-1)
    if len(off) < 1:
        raise ValueError("track_off needs n + 1 entries")
    n = len(off) - 1
    view = np.ascontiguousarray(obs_view, np.int32).reshape(-1)
    uv = np.ascontiguousarray(obs_uv, np.float32).reshape(-1, 2)
    if len(view) != len(uv) or int(off[-1]) != len(view):
        raise ValueError("track_off[-1], obs_view and obs_uv disagree on the number of observations")
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    Td = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 16)
    X = np.zeros((max(n, 1), 3), np.float64)
    idx = np.zeros(max(n, 1), np.int32)
    info = (C.c_int32 * 8)()
    reason = np.zeros(max(n, 1), np.int32) if want_diag else None
    diag = np.zeros((max(n, 1), 3), np.float64) if want_diag else None
    P = _native.ptr
    _native.check(_native.lib().sslam_triangulate_tracks_host(
        ctx.handle, n, len(Td), P(off), P(view), P(uv), P(Kd), P(Td), float(min_depth), float(max_depth), float(max_rep_err),
        P(X), P(idx), info, P(reason), P(diag)), "sslam_triangulate_tracks_host")
    kept = int(info[0])
    out = None
    if want_diag:
        out = {"reason": reason[:n]}
        out.update({name: diag[:n, k] for k, name in enumerate(DIAG_FIELDS)})
    return X[:kept], idx[:kept], {name: int(info[1 + k]) for k, name in enumerate(REASONS)}, out
