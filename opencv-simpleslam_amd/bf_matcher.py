"""Brute-force descriptor matcher on the HIP backend.

Stands in for `cv2.BFMatcher(normType, crossCheck)` as the reference's default configuration uses it
(`--detector orb --matcher bf`): `_get_opencv_matcher` builds `cv2.BFMatcher(norm, crossCheck=True)` with NORM_HAMMING for
ORB / AKAZE and NORM_L2 for SIFT (slam/core/features_utils.py:54-55) and `feature_matcher` calls `.match(des0, des1)` on it
and sorts the result by `.distance` (:173-178).  `BFMatcher(norm, crossCheck=True)` here is that object: hand it to
`feature_matcher` as the matcher.  The detectors that make ORB / SIFT / AKAZE descriptors have GPU forms too (orb.py, sift.py, akaze.py); only FLANN still needs OpenCV.

Only `match` is provided (one nearest neighbour, optionally cross-checked): no `knnMatch` with k > 1, no `radiusMatch`, no
NORM_L1 / NORM_HAMMING2, no train collections, no mask.  Semantics: include/sslam_hip.h, `sslam_bf_match_host`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

NORM_L2 = 4                # cv2's values
NORM_HAMMING = 6
MAX_ROWS = 65536
_DTYPE = {NORM_L2: np.float32, NORM_HAMMING: np.uint8}
_MAX_D = {NORM_L2: 512, NORM_HAMMING: 256}


def _norm_name(norm):
    return "NORM_L2" if norm == NORM_L2 else "NORM_HAMMING"


class BFMatcher:
    """`cv2.BFMatcher(normType, crossCheck)` with `.match(queryDescriptors, trainDescriptors)`."""

    def __init__(self, normType: int = NORM_L2, crossCheck: bool = False, ctx=None):
        if normType not in _DTYPE:
            raise ValueError(f"BFMatcher: normType {normType} is neither NORM_L2 (4) nor NORM_HAMMING (6)")
        self.normType = int(normType)
        self.crossCheck = bool(crossCheck)
        self.ctx = ctx

    def _rows(self, des, name):
        """`des` as the contiguous [rows, D] array the norm takes; a dtype that does not fit it is refused, never cast."""
        want = _DTYPE[self.normType]
        if hasattr(des, "detach"):
            des = des.detach().to("cpu").numpy()
        des = np.asarray(des)
        if des.size == 0 or des.dtype == object and des.ndim == 0:          # [] / None, as a detector returns for a blank image
            return np.empty((0, 0), want)
        if des.dtype != want:
            raise TypeError(f"BFMatcher({_norm_name(self.normType)}): {name} is {des.dtype}, the norm takes {np.dtype(want)}")
        if des.ndim != 2:
            raise ValueError(f"BFMatcher: {name} must be [rows, D], got shape {des.shape}")
        return np.ascontiguousarray(des)

    def match_arrays(self, des0, des1, mask=None):
        """-> (ij int32 [K,2] (queryIdx, trainIdx) in query order, dist float32 [K])."""
        if mask is not None:
            raise ValueError("BFMatcher.match: a mask is not supported")
        q, t = self._rows(des0, "queryDescriptors"), self._rows(des1, "trainDescriptors")
        M, N = len(q), len(t)
        if M == 0 or N == 0:
            return np.empty((0, 2), np.int32), np.empty(0, np.float32)
        D = q.shape[1]
        if t.shape[1] != D:
            raise ValueError(f"BFMatcher.match: queryDescriptors have D = {D}, trainDescriptors D = {t.shape[1]}")
        if not 1 <= D <= _MAX_D[self.normType]:
            raise ValueError(f"BFMatcher.match: D {D} outside 1..{_MAX_D[self.normType]} ({_norm_name(self.normType)})")
        if M > MAX_ROWS or N > MAX_ROWS:
            raise ValueError(f"BFMatcher.match: {M} x {N} rows, at most {MAX_ROWS} a side")
        ctx = self.ctx or _native.default_context()
        ij = np.empty((M, 2), np.int32)
        dist = np.empty(M, np.float32)
        k = C.c_int32(0)
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_match_host(ctx.handle, self.normType, int(self.crossCheck), D, P(q), M, P(t), N,
                                                        P(ij), P(dist), C.byref(k)), "sslam_bf_match_host")
        return ij[:k.value].copy(), dist[:k.value].copy()

    def match(self, queryDescriptors, trainDescriptors, mask=None):
        """-> list of DMatch(queryIdx, trainIdx, imgIdx 0, distance), ascending queryIdx (cv2.DMatch where OpenCV is
        installed, else the duck type of slam/core/types.py)."""
        from .slam.core.types import DMatch
        ij, dist = self.match_arrays(queryDescriptors, trainDescriptors, mask)
        if len(ij) == 0:
            return []
        qi, ti = ij.T.tolist()
        return [DMatch(a, b, 0, d) for a, b, d in zip(qi, ti, dist.tolist())]

    def match_dev(self, ctx, D: int, q_dev, M: int, t_dev, N: int, ij_out_dev, dist_out_dev, info_out_dev,
                  m_dev=None, n_dev=None):
        """Device-resident match: the `*_dev` arguments are device pointers (ints) - descriptors [M, D] / [N, D] of the
        norm's dtype, optional int32 counts (as `sslam_aliked_extract_dev` writes them; negative = empty) - and the pairs
        [M,2] int32, distances [M] float32 and info [4] int32 = {K, m, n, 0} stay on the device: `ij_out_dev` and
        `info_out_dev` are what `epipolar.filter_matches_dev` takes as `ij_dev` / `n_dev`.  Enqueued on ctx's stream."""
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_match_dev(ctx.handle, self.normType, int(self.crossCheck), int(D), P(q_dev), int(M),
                                                       P(m_dev), P(t_dev), int(N), P(n_dev), P(ij_out_dev), P(dist_out_dev),
                                                       P(info_out_dev)), "sslam_bf_match_dev")
