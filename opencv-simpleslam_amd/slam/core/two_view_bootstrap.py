"""The one name `triangulation_utils` takes from the reference's `slam/core/two_view_bootstrap.py`:
`pts_from_matches` (:415-418), so that importing the overlay's triangulation never reaches `cv2`.

The two-view bootstrap itself is not here but in two modules of its own, `two_view_pose` (the F/E leg, the scores, the map
building) and `two_view_gate` (homography RANSAC, `decomposeHomographyMat`, the model selection): a driver patches their
names into the module it bootstraps with, and this one stays importable on its own.
"""
from __future__ import annotations

import numpy as np


def pts_from_matches(kps_ref, kps_cur, matches):
    """Matched pixel coordinates of both frames as float32 [n,2] arrays, in match order."""
    pts_ref = np.float32([kps_ref[m.queryIdx].pt for m in matches])
    pts_cur = np.float32([kps_cur[m.trainIdx].pt for m in matches])
    return pts_ref, pts_cur
