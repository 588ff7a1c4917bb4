"""ORB on the HIP backend.

Stands in for `cv2.ORB_create(nfeatures, ...)` as the reference's default configuration uses it (`--detector orb --matcher bf`):
`_get_opencv_detector` builds `cv2.ORB_create(max_features)` (slam/core/features_utils.py:33-55) and `feature_extractor` calls
`.detectAndCompute(img, None)` on it.  `ORB_create(...)` here is that object; with `bf_matcher.BFMatcher(NORM_HAMMING,
crossCheck=True)` behind it the branch runs without OpenCV, and `detect_dev` -> `BFMatcher.match_dev` ->
`epipolar.filter_matches_dev` runs it without a host round trip.

Semantics: include/sslam_hip.h (`sslam_orb_create`) and tests/orb_ref.py, which restates OpenCV's `ORB_Impl::detectAndCompute`
and names what could not be confirmed without cv2.  THE STATED DEVIATION: for patchSize 31 OpenCV samples a learned table of
256 point pairs that is not available here; the default pattern is the one OpenCV generates for every other patch size
(`makeRandomPattern`, cv::RNG(0x34985739)).  Keypoints are meant to equal cv2's; descriptors are self-consistent - all that
frame-to-frame matching needs - but NOT interchangeable with descriptors computed by cv2.  `pattern=` (int8 [512, 2], x and y
in -15..15) takes the learned table from a user who has it.

Refused with a ValueError: firstLevel != 0, WTA_K != 2, patchSize != 31, a mask, nfeatures < 1, scaleFactor outside (1, 2],
nlevels outside 1..16, edgeThreshold < 3, a scoreType other than HARRIS_SCORE / FAST_SCORE, fastThreshold outside 1..254, an
image larger than max_w x max_h (never clipped).  The order of the output is defined: level ascending, response descending,
then y, then x.  Ties at a cut are kept, so more than nfeatures rows can come back.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native
from ._detector import Detector

HARRIS_SCORE = 0           # cv2's values
FAST_SCORE = 1
MAX_LEVELS = 16
MAX_FEATURES = 1 << 20
MAX_SIDE = 16384


class ORB(Detector):
    """`cv2.ORB` with `detectAndCompute(image, mask=None)`.  The device instance is made at the first call."""
    NAME, PREFIX = "ORB", "orb"
    ROWS = ((2,), np.float32), ((4,), np.float32), ((32,), np.uint8)

    def __init__(self, nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=HARRIS_SCORE,
                 patchSize=31, fastThreshold=20, *, pattern=None, max_h=2160, max_w=4096, ctx=None):
        nfeatures, nlevels, edgeThreshold, fastThreshold = int(nfeatures), int(nlevels), int(edgeThreshold), int(fastThreshold)
        if firstLevel != 0:
            raise ValueError(f"ORB_create: firstLevel {firstLevel} is not supported (only 0)")
        if WTA_K != 2:
            raise ValueError(f"ORB_create: WTA_K {WTA_K} is not supported (only 2)")
        if patchSize != 31:
            raise ValueError(f"ORB_create: patchSize {patchSize} is not supported (only 31)")
        if not 1 <= nfeatures <= MAX_FEATURES:
            raise ValueError(f"ORB_create: nfeatures {nfeatures} outside 1..{MAX_FEATURES}")
        if not 1.0 < float(np.float32(scaleFactor)) <= 2.0:
            raise ValueError(f"ORB_create: scaleFactor {scaleFactor} outside (1, 2]")
        if not 1 <= nlevels <= MAX_LEVELS:
            raise ValueError(f"ORB_create: nlevels {nlevels} outside 1..{MAX_LEVELS}")
        if edgeThreshold < 3:
            raise ValueError(f"ORB_create: edgeThreshold {edgeThreshold} below 3")
        if scoreType not in (HARRIS_SCORE, FAST_SCORE):
            raise ValueError(f"ORB_create: scoreType {scoreType} is neither HARRIS_SCORE (0) nor FAST_SCORE (1)")
        if not 1 <= fastThreshold <= 254:
            raise ValueError(f"ORB_create: fastThreshold {fastThreshold} outside 1..254")
        if not (1 <= int(max_w) <= MAX_SIDE and 1 <= int(max_h) <= MAX_SIDE):
            raise ValueError(f"ORB_create: max_w x max_h {max_w}x{max_h} outside 1..{MAX_SIDE}")
        if pattern is not None:
            pattern = np.asarray(pattern)
            if pattern.dtype != np.int8 or pattern.shape != (512, 2):
                raise ValueError(f"ORB_create: pattern must be int8 [512, 2], got {pattern.dtype} {pattern.shape}")
            if np.abs(pattern.astype(np.int32)).max() > 15:
                raise ValueError("ORB_create: a pattern coordinate is outside -15..15")
            pattern = np.ascontiguousarray(pattern)
        self.nfeatures, self.scaleFactor, self.nlevels, self.edgeThreshold = nfeatures, float(scaleFactor), nlevels, edgeThreshold
        self.scoreType, self.fastThreshold, self.pattern = int(scoreType), fastThreshold, pattern
        self._setup(max_h, max_w, ctx)

    def _create(self, L, handle_ref):
        return L.sslam_orb_create(self.ctx.handle, self.max_w, self.max_h, self.nfeatures, float(np.float32(self.scaleFactor)), self.nlevels,
                                  self.edgeThreshold, self.scoreType, self.fastThreshold, _native.ptr(self.pattern), handle_ref)

    def detect_arrays(self, img, mask=None):
        """-> (xy float32 [N,2], aux float32 [N,4] = size, angle, response, octave, desc uint8 [N,32])."""
        return self._detect_host(img, mask)

    def detectAndCompute(self, image, mask=None):
        """-> (list of KeyPoint with every field set, descriptors uint8 [N, 32]); ([], None) without a keypoint.  KeyPoint is
        cv2.KeyPoint where OpenCV is installed, else the duck type of slam/core/types.py."""
        from .slam.core.types import KeyPoint
        xy, aux, desc = self.detect_arrays(image, mask)
        if len(xy) == 0:
            return [], None
        kps = [KeyPoint(x, y, s, a, r, int(o), -1) for (x, y), (s, a, r, o) in zip(xy.tolist(), aux.tolist())]
        return kps, desc

    def detect_dev(self, img_dev, h: int, w: int, c: int, xy_out_dev, aux_out_dev, desc_out_dev, n_out_dev):
        """Device-resident call: the `*_dev` arguments are device pointers (ints) - the image uint8 [h, w, c], xy float32
        [capacity, 2], aux float32 [capacity, 4], desc uint8 [capacity, 32], the count int32 [1] - and everything stays on the
        device: `desc_out_dev` / `n_out_dev` are what `BFMatcher.match_dev` takes as `q_dev` / `m_dev` (with `chain_rows`, not
        the capacity, as its M), `xy_out_dev` what `epipolar.filter_matches_dev` takes as `xy1_dev`.  Enqueued on the instance's context stream, no synchronisation."""
        self._check_dev_size(h, w)
        P = _native.ptr
        _native.check(_native.lib().sslam_orb_detect_dev(self._instance(), P(img_dev), int(h), int(w), int(c), P(xy_out_dev),
                                                         P(aux_out_dev), P(desc_out_dev), P(n_out_dev)), "sslam_orb_detect_dev")

    # test hooks (include/sslam_hip.h: sslam_orb_level_info, sslam_orb_stage_read)
    def level_info(self, level: int):
        v = np.zeros(8, np.int32)
        _native.check(_native.lib().sslam_orb_level_info(self._instance(), int(level), _native.ptr(v)), "sslam_orb_level_info")
        return dict(zip(("w", "h", "stride", "rows", "stored", "quota", "cand_cap", "border"), v.tolist()))

    def stage_read(self, level: int):
        """-> dict(img, blur uint8 [rows, stride], cand int32 [K, 3] (x, y, score), resp float32 [K] (NaN: dropped by the first
        cut), cut1 int, cut2 float32) of a stored level of the last frame."""
        i = self.level_info(level)
        img, blur = np.empty((i["rows"], i["stride"]), np.uint8), np.empty((i["rows"], i["stride"]), np.uint8)
        cand, n, cuts = np.zeros((max(i["cand_cap"], 1), 4), np.int32), C.c_int32(0), np.zeros(2, np.int32)
        P = _native.ptr
        _native.check(_native.lib().sslam_orb_stage_read(self._instance(), int(level), P(img), P(blur), P(cand), C.byref(n), P(cuts)),
                      "sslam_orb_stage_read")
        cand = cand[:n.value]
        return dict(img=img, blur=blur, cand=cand[:, :3].copy(), resp=cand[:, 3].copy().view(np.float32), cut1=int(cuts[0]),
                    cut2=cuts[1:2].view(np.float32)[0])


def ORB_create(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=HARRIS_SCORE,
               patchSize=31, fastThreshold=20, *, pattern=None, max_h=2160, max_w=4096, ctx=None):
    """`cv2.ORB_create` with the same positional arguments -> ORB."""
    return ORB(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold,
               pattern=pattern, max_h=max_h, max_w=max_w, ctx=ctx)


def default_pattern():
    """The default sampling pattern, int8 [512, 2] (needs the library, not a device)."""
    out = np.zeros((512, 2), np.int8)
    _native.check(_native.lib().sslam_orb_default_pattern(_native.ptr(out)), "sslam_orb_default_pattern")
    return out
