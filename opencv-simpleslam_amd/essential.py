"""Essential-matrix RANSAC on the HIP backend.

Stands in for `cv2.findEssentialMat(pts0, pts1, K, cv2.RANSAC, 0.999, thresh)` as the reference's tracking-lost fallback
calls it (slam/monocular/main_revamped.py:512, main.py:402, main4.py:457).  Parity with cv2 is unpinned
(tests/essential_ref.py restates the algorithm and names what could not be confirmed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

MODEL_POINTS = 5


def find_essential_mat_ransac(pts1, pts2, K, prob: float = 0.999, thresh: float = 1.0, max_iters: int = 1000, ctx=None):
    """pts1, pts2: [n,2] matched pixels (cast to float32 as the reference holds them), n <= 16384; K: [3,3].
    Returns (E, mask, info): E [3,3] float64 of unit Frobenius norm ([3k,3], every model stacked, for n == 5), mask uint8
    [n,1] of 0 / 1 - the shape `relative_pose.recover_pose(..., mask=)` takes - and info {"inliers", "iterations", "model",
    "sample"}.  (None, None, info) where cv2 returns (None, None): no model, or n < 5 (answered here, without the library)."""
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    if len(p1) != len(p2):
        raise ValueError("pts1 / pts2 length mismatch")
    n = len(p1)
    if n < MODEL_POINTS:
        return None, None, {"inliers": -1, "iterations": 0, "model": 0, "sample": -1}
    ctx = ctx or _native.default_context()
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    mask = np.zeros(n, np.uint8)
    E = np.zeros(90, np.float64)
    info = (C.c_int32 * 4)()
    P = _native.ptr
    _native.check(_native.lib().sslam_essential_ransac_host(
        ctx.handle, n, P(p1), P(p2), P(Kd), float(prob), float(thresh), int(max_iters), P(mask), P(E), info),
        "sslam_essential_ransac_host")
    meta = {"inliers": int(info[0]), "iterations": int(info[1]), "model": int(info[2]), "sample": int(info[3])}
    if info[0] < 0:
        return None, None, meta
    k = int(info[2]) if n == MODEL_POINTS else 1
    return E[:9 * k].reshape(3 * k, 3).copy(), mask.reshape(-1, 1), meta
