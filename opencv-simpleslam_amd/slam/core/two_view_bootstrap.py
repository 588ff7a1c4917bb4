"""The one name `triangulation_utils` takes from the reference's `slam/core/two_view_bootstrap.py`:
`pts_from_matches` (:415-418), so that importing the overlay's triangulation never reaches `cv2`.

The two-view bootstrap itself - homography / essential-matrix RANSAC, `decomposeHomographyMat`, `recoverPose`, the model
selection around them - is OUT OF SCOPE of this backend and is not here: a driver that bootstraps a map keeps the
reference's module for that (it needs OpenCV) and patches in only the names it wants from this overlay.
"""
from __future__ import annotations

import numpy as np


def pts_from_matches(kps_ref, kps_cur, matches):
    """Matched pixel coordinates of both frames as float32 [n,2] arrays, in match order."""
    pts_ref = np.float32([kps_ref[m.queryIdx].pt for m in matches])
    pts_cur = np.float32([kps_cur[m.trainIdx].pt for m in matches])
    return pts_ref, pts_cur
