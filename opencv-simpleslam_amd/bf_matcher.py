"""Brute-force descriptor matcher on the HIP backend.

Stands in for `cv2.BFMatcher(normType, crossCheck)` as the reference's default configuration uses it
(`--detector orb --matcher bf`): `_get_opencv_matcher` builds `cv2.BFMatcher(norm, crossCheck=True)` with NORM_HAMMING for
ORB / AKAZE and NORM_L2 for SIFT (slam/core/features_utils.py:54-55) and `feature_matcher` calls `.match(des0, des1)` on it
and sorts the result by `.distance` (:173-178).  `BFMatcher(norm, crossCheck=True)` here is that object: hand it to
`feature_matcher` as the matcher.  The detectors that make ORB / SIFT / AKAZE descriptors have GPU forms too (orb.py, sift.py,
akaze.py), and `--matcher flann` has a stand-in on top of this class (flann_matcher.py).

Provided: `match` (one nearest neighbour, optionally cross-checked), `knnMatch` (the k nearest, k = 1..8) and the ratio test
on the two nearest as a stage of its own (`ratio_match`: `m.distance < ratio * n.distance`, the usual companion of SIFT
descriptors; nothing in the reference calls it), each with an array form and a device-resident form.  The search is exact.
Out of scope: `radiusMatch`, masks, train collections (`add` / `train`), NORM_L1 / NORM_HAMMING2 / NORM_L2SQR, k > 8.
Semantics: include/sslam_hip.h, `sslam_bf_match_host`, `sslam_bf_knn_match_host`, `sslam_bf_ratio_match_host`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

NORM_L2 = 4                # cv2's values
NORM_HAMMING = 6
MAX_ROWS = 65536
MAX_K = 8
_DTYPE = {NORM_L2: np.float32, NORM_HAMMING: np.uint8}
_MAX_D = {NORM_L2: 512, NORM_HAMMING: 256}


def _norm_name(norm):
    return "NORM_L2" if norm == NORM_L2 else "NORM_HAMMING"


class BFMatcher:
    """`cv2.BFMatcher(normType, crossCheck)` with `.match(queryDescriptors, trainDescriptors)` and `.knnMatch(..., k)`."""

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

    def _pair(self, des0, des1, who):
        """-> (q, t, M, N, D) of a call, every refusal made; D is 0 when a side is empty"""
        q, t = self._rows(des0, "queryDescriptors"), self._rows(des1, "trainDescriptors")
        M, N = len(q), len(t)
        if M == 0 or N == 0:
            return q, t, M, N, 0
        D = q.shape[1]
        if t.shape[1] != D:
            raise ValueError(f"BFMatcher.{who}: queryDescriptors have D = {D}, trainDescriptors D = {t.shape[1]}")
        if not 1 <= D <= _MAX_D[self.normType]:
            raise ValueError(f"BFMatcher.{who}: D {D} outside 1..{_MAX_D[self.normType]} ({_norm_name(self.normType)})")
        if M > MAX_ROWS or N > MAX_ROWS:
            raise ValueError(f"BFMatcher.{who}: {M} x {N} rows, at most {MAX_ROWS} a side")
        return q, t, M, N, D

    def match_arrays(self, des0, des1, mask=None):
        """-> (ij int32 [K,2] (queryIdx, trainIdx) in query order, dist float32 [K])."""
        if mask is not None:
            raise ValueError("BFMatcher.match: a mask is not supported")
        q, t, M, N, D = self._pair(des0, des1, "match")
        if M == 0 or N == 0:
            return np.empty((0, 2), np.int32), np.empty(0, np.float32)
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

    # ---- the k nearest neighbours -----------------------------------------------------------------------------------------
    def _check_k(self, k, who):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
            raise ValueError(f"BFMatcher.{who}: k {k!r} outside 1..{MAX_K}")
        if self.crossCheck and int(k) > 1:
            raise ValueError(f"BFMatcher.{who}: k {k} with crossCheck=True (cv2 takes k == 1 only)")
        return int(k)

    def knn_match_arrays(self, des0, des1, k, mask=None, splits=0):
        """-> (idx int32 [M,k] padded with -1, dist float32 [M,k] padded with +inf, cnt int32 [M]): per query row its valid train
        rows in ascending order of (distance, trainIdx), the first min(k, valid) of them.  crossCheck is not applied here
        (`knnMatch` applies it for k == 1); `splits`: see sslam_bf_knn_match_host, 0 = chosen by the host plan."""
        if mask is not None:
            raise ValueError("BFMatcher.knnMatch: a mask is not supported")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
            raise ValueError(f"BFMatcher.knnMatch: k {k!r} outside 1..{MAX_K}")
        k = int(k)
        q, t, M, N, D = self._pair(des0, des1, "knnMatch")
        idx, dist, cnt = np.full((M, k), -1, np.int32), np.full((M, k), np.inf, np.float32), np.zeros(M, np.int32)
        if M == 0 or N == 0:
            return idx, dist, cnt
        ctx = self.ctx or _native.default_context()
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_knn_match_host(ctx.handle, self.normType, D, P(q), M, P(t), N, k, int(splits),
                                                            P(idx), P(dist), P(cnt)), "sslam_bf_knn_match_host")
        return idx, dist, cnt

    def knnMatch(self, queryDescriptors, trainDescriptors, k, mask=None, compactResult=False):
        """-> list of M lists of DMatch(queryIdx, trainIdx, imgIdx 0, distance), nearest first; a query row without a neighbour
        has an empty list, dropped when `compactResult` is set.  With crossCheck only k == 1 is taken and a list holds the
        mutual match or nothing."""
        from .slam.core.types import DMatch
        if mask is not None:
            raise ValueError("BFMatcher.knnMatch: a mask is not supported")
        k = self._check_k(k, "knnMatch")
        if self.crossCheck:
            M = len(self._rows(queryDescriptors, "queryDescriptors"))
            ij, dist = self.match_arrays(queryDescriptors, trainDescriptors)
            out = [[] for _ in range(M)]
            for (i, j), d in zip(ij.tolist(), dist.tolist()):
                out[i].append(DMatch(i, j, 0, d))
        else:
            idx, dist, cnt = self.knn_match_arrays(queryDescriptors, trainDescriptors, k)
            out = [[DMatch(i, j, 0, d) for j, d in zip(js[:c], ds[:c])]
                   for i, (js, ds, c) in enumerate(zip(idx.tolist(), dist.tolist(), cnt.tolist()))]
        return [m for m in out if m] if compactResult else out

    def knn_match_dev(self, ctx, D: int, q_dev, M: int, t_dev, N: int, k: int, idx_out_dev, dist_out_dev, cnt_out_dev,
                      info_out_dev, m_dev=None, n_dev=None, splits=0):
        """Device-resident k-NN (crossCheck is not applied): device pointers as for `match_dev`; idx [M,k] int32, dist [M,k]
        float32, cnt [M] int32 and info [4] int32 = {m, n, k, splits used} stay on the device, rows at and beyond the device
        count m are not written.  Enqueued on ctx's stream."""
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_knn_match_dev(ctx.handle, self.normType, int(D), P(q_dev), int(M), P(m_dev), P(t_dev),
                                                           int(N), P(n_dev), int(k), int(splits), P(idx_out_dev), P(dist_out_dev),
                                                           P(cnt_out_dev), P(info_out_dev)), "sslam_bf_knn_match_dev")

    # ---- Lowe's ratio test on the two nearest --------------------------------------------------------------------------------
    @staticmethod
    def _check_ratio(ratio):
        r = float(ratio)
        if not (np.isfinite(r) and r > 0):
            raise ValueError(f"BFMatcher.ratio_match: ratio {ratio!r} is not finite and > 0")
        return r

    def ratio_match_arrays(self, des0, des1, ratio=0.75, splits=0):
        """-> (ij int32 [K,2], dist float32 [K]) in query order: the nearest neighbour of every query row that has two and
        passes `d1 < ratio * d2` (doubles, one multiply).  crossCheck is not applied."""
        ratio = self._check_ratio(ratio)
        q, t, M, N, D = self._pair(des0, des1, "ratio_match")
        if M == 0 or N == 0:
            return np.empty((0, 2), np.int32), np.empty(0, np.float32)
        ctx = self.ctx or _native.default_context()
        ij = np.empty((M, 2), np.int32)
        dist = np.empty(M, np.float32)
        k = C.c_int32(0)
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_ratio_match_host(ctx.handle, self.normType, D, P(q), M, P(t), N, ratio, int(splits),
                                                              P(ij), P(dist), C.byref(k)), "sslam_bf_ratio_match_host")
        return ij[:k.value].copy(), dist[:k.value].copy()

    def ratio_match(self, queryDescriptors, trainDescriptors, ratio=0.75):
        """-> list of DMatch: `[m for m, n in knnMatch(q, t, k=2) if m.distance < ratio * n.distance]` (rows with fewer than
        two neighbours dropped), computed on the device."""
        from .slam.core.types import DMatch
        ij, dist = self.ratio_match_arrays(queryDescriptors, trainDescriptors, ratio)
        if len(ij) == 0:
            return []
        qi, ti = ij.T.tolist()
        return [DMatch(a, b, 0, d) for a, b, d in zip(qi, ti, dist.tolist())]

    def ratio_match_dev(self, ctx, D: int, q_dev, M: int, t_dev, N: int, ij_out_dev, dist_out_dev, info_out_dev,
                        ratio=0.75, m_dev=None, n_dev=None, splits=0):
        """Device-resident ratio test; the outputs have `match_dev`'s layout - pairs [M,2], distances [M], info {K, m, n, 0} -,
        so `ij_out_dev` and `info_out_dev` are what `epipolar.filter_matches_dev` takes.  Enqueued on ctx's stream."""
        P = _native.ptr
        _native.check(_native.lib().sslam_bf_ratio_match_dev(ctx.handle, self.normType, int(D), P(q_dev), int(M), P(m_dev), P(t_dev),
                                                             int(N), P(n_dev), self._check_ratio(ratio), int(splits), P(ij_out_dev),
                                                             P(dist_out_dev), P(info_out_dev)), "sslam_bf_ratio_match_dev")
