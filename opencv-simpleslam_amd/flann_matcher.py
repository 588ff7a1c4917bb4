"""`cv2.FlannBasedMatcher(indexParams, searchParams)` on the HIP backend, for `--matcher flann`.

The reference builds `cv2.FlannBasedMatcher(dict(algorithm=1, trees=5), dict(checks=50))` (slam/core/features_utils.py:46-52)
and `feature_matcher` calls `.match(des0, des1)` on it (:177).  `FlannBasedMatcher(index_params, search_params)` here is the
object to return from `_get_opencv_matcher` instead: `match`, `knnMatch` and the ratio test run on the brute-force kernels
of bf_matcher.py.

STATED DEPARTURE: the search is EXACT.  FLANN's answer is approximate and a function of its randomised tree build; it can
never be closer than the exact neighbour, which is its limit for `checks -> infinity`.  A brute-force call on this device
costs less than any tree build, so no index is built: the parameters are kept on the object and otherwise ignored.

Descriptor types: float32 rows are matched with NORM_L2 for any `algorithm` but FLANN_INDEX_LSH; uint8 rows with
NORM_HAMMING, and only with `algorithm = FLANN_INDEX_LSH` - with any other algorithm uint8 rows raise a TypeError, as cv2's
KD-tree index refuses them (from memory of OpenCV 4.x; unconfirmed here).

Out of scope: `radiusMatch`, masks, train collections (`add` / `train`), NORM_L1 / NORM_HAMMING2 / NORM_L2SQR, k > 8.
"""
from __future__ import annotations

import numpy as np

from . import bf_matcher

FLANN_INDEX_KDTREE = 1         # cv2's / FLANN's values
FLANN_INDEX_LSH = 6


class FlannBasedMatcher:
    """`cv2.FlannBasedMatcher(indexParams, searchParams)` with `.match`, `.knnMatch` and `.ratio_match`; exact search."""

    def __init__(self, indexParams=None, searchParams=None, ctx=None):
        self.indexParams = dict(indexParams) if indexParams is not None else dict(algorithm=FLANN_INDEX_KDTREE, trees=4)
        self.searchParams = dict(searchParams) if searchParams is not None else dict(checks=32)
        self.ctx = ctx

    def _bf(self, des0, des1):
        """the brute-force matcher of the descriptors' type (NORM_L2 for an empty side: no rows, no result)"""
        lsh = self.indexParams.get("algorithm", FLANN_INDEX_KDTREE) == FLANN_INDEX_LSH
        for name, des in (("queryDescriptors", des0), ("trainDescriptors", des1)):
            if hasattr(des, "detach"):
                des = des.detach().to("cpu").numpy()
            des = np.asarray(des)
            if des.size == 0 or des.dtype == object:
                continue
            if des.dtype == np.uint8 and not lsh:
                raise TypeError(f"FlannBasedMatcher: {name} is uint8 and indexParams['algorithm'] is "
                                f"{self.indexParams.get('algorithm', FLANN_INDEX_KDTREE)}: cv2's KD-tree index refuses uint8 rows; "
                                f"binary descriptors take algorithm = FLANN_INDEX_LSH ({FLANN_INDEX_LSH})")
            if des.dtype == np.float32 and lsh:
                raise TypeError(f"FlannBasedMatcher: {name} is float32 and indexParams['algorithm'] is FLANN_INDEX_LSH "
                                f"({FLANN_INDEX_LSH}), which takes uint8 rows")
        return bf_matcher.BFMatcher(bf_matcher.NORM_HAMMING if lsh else bf_matcher.NORM_L2, crossCheck=False, ctx=self.ctx)

    def match(self, queryDescriptors, trainDescriptors, mask=None):
        """-> list of DMatch, the exact nearest train row of every query row (no cross-check), ascending queryIdx."""
        if mask is not None:
            raise ValueError("FlannBasedMatcher.match: a mask is not supported")
        return self._bf(queryDescriptors, trainDescriptors).match(queryDescriptors, trainDescriptors)

    def knnMatch(self, queryDescriptors, trainDescriptors, k, mask=None, compactResult=False):
        """-> list of M lists of DMatch, the exact k nearest, k = 1..8 (bf_matcher.BFMatcher.knnMatch)."""
        if mask is not None:
            raise ValueError("FlannBasedMatcher.knnMatch: a mask is not supported")
        return self._bf(queryDescriptors, trainDescriptors).knnMatch(queryDescriptors, trainDescriptors, k, compactResult=compactResult)

    def ratio_match(self, queryDescriptors, trainDescriptors, ratio=0.75):
        """-> list of DMatch: `[m for m, n in knnMatch(q, t, 2) if m.distance < ratio * n.distance]` on the device."""
        return self._bf(queryDescriptors, trainDescriptors).ratio_match(queryDescriptors, trainDescriptors, ratio)
