"""Homography RANSAC on the HIP backend.

Stands in for `cv2.findHomography(pts_ref, pts_cur, cv2.RANSAC, px)` as the reference's two-view gate calls it
(slam/core/two_view_bootstrap.py:230, :294) and its tracking fallbacks do (slam/monocular/main.py:409, main4.py:458).
Parity with cv2 is unpinned (tests/homography_ref.py restates the algorithm and names what could not be confirmed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native


def find_homography_ransac(pts1, pts2, thresh: float = 3.0, confidence: float = 0.995, max_iters: int = 2000, ctx=None):
    """pts1, pts2: [n,2] matched pixels, source and destination (cast to float32 as the reference holds them),
    4 <= n <= 16384.  Returns (H [3,3] float64 or None, mask [n] bool or None, info dict) - (None, None) where cv2
    returns (None, None).  The mask is the RANSAC loop's; H is refitted on it and polished."""
    ctx = ctx or _native.default_context()
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("pts1 / pts2 length mismatch")
    n = len(p1)
    mask = np.zeros(max(n, 1), np.uint8)
    H = np.zeros(9, np.float64)
    info = (C.c_int32 * 4)()
    P = _native.ptr
    _native.check(_native.lib().sslam_homography_ransac_host(
        ctx.handle, n, P(p1), P(p2), float(thresh), float(confidence), int(max_iters), P(mask), P(H), info),
        "sslam_homography_ransac_host")
    meta = {"inliers": int(info[0]), "iterations": int(info[1]), "sample": int(info[3])}
    if info[0] < 0:
        return None, None, meta
    return H.reshape(3, 3), mask[:n].astype(bool), meta
