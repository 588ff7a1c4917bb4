"""SIFT on the HIP backend.

Stands in for `cv2.SIFT_create(nfeatures, ...)` as the reference's OpenCV branch uses it (`--detector sift`):
`_get_opencv_detector` builds `cv2.SIFT_create(nfeatures=max_features)` (slam/core/features_utils.py:33-55) and
`feature_extractor` calls `.detectAndCompute(img, None)` on it.  `SIFT_create(...)` here is that object; with
`bf_matcher.BFMatcher(NORM_L2, crossCheck=True)` behind it the pair runs without OpenCV, and `detect_dev` ->
`BFMatcher.match_dev` -> `epipolar.filter_matches_dev` runs it without a host round trip.

Semantics: include/sslam_hip.h (`sslam_sift_create`) and tests/sift_ref.py, which restates OpenCV's
`SIFT_Impl::detectAndCompute` and names what could not be confirmed without cv2.  The arithmetic is defined (float32 one
operation at a time, the two histograms as exact integer sums), so the kernels equal the restatement bit for bit; the order of
the output is defined too: x, y ascending, size descending, angle ascending.  Duplicates are dropped before the quota and ties
at the quota are kept, so more than nfeatures rows can come back.

Refused with a ValueError: a mask, nfeatures < 0, nOctaveLayers outside 1..8, non-positive thresholds, sigma outside (0.5, 8],
a descriptorType other than float32, enable_precise_upscale, an image larger than max_w x max_h (never clipped); a non-uint8
image with a TypeError.  A frame with more extrema than `max_candidates` or more keypoints than `max_keypoints` is voided and
raises `_native.NativeError`; it is never truncated.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._detector import CapacityDetector

MAX_OCTAVE_LAYERS = 8
MAX_FEATURES = 1 << 20
MAX_SIDE = 16384
CV_32F = 5                 # cv2's value


class SIFT(CapacityDetector):
    """`cv2.SIFT` with `detectAndCompute(image, mask=None)`.  The device instance is made at the first call."""
    NAME, PREFIX = "SIFT", "sift"
    ROWS = ((2,), np.float32), ((3,), np.float32), ((), np.int32), ((128,), np.float32)

    def __init__(self, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, descriptorType=CV_32F,
                 enable_precise_upscale=False, *, max_h=2160, max_w=4096, max_candidates=0, max_keypoints=0, ctx=None):
        nfeatures, nOctaveLayers = int(nfeatures), int(nOctaveLayers)
        if not 0 <= nfeatures <= MAX_FEATURES:
            raise ValueError(f"SIFT_create: nfeatures {nfeatures} outside 0..{MAX_FEATURES}")
        if not 1 <= nOctaveLayers <= MAX_OCTAVE_LAYERS:
            raise ValueError(f"SIFT_create: nOctaveLayers {nOctaveLayers} outside 1..{MAX_OCTAVE_LAYERS}")
        if not (float(contrastThreshold) > 0 and np.isfinite(contrastThreshold)):
            raise ValueError(f"SIFT_create: contrastThreshold {contrastThreshold} is not positive")
        if not (float(edgeThreshold) > 0 and np.isfinite(edgeThreshold)):
            raise ValueError(f"SIFT_create: edgeThreshold {edgeThreshold} is not positive")
        if not 0.5 < float(sigma) <= 8:
            raise ValueError(f"SIFT_create: sigma {sigma} outside (0.5, 8]")
        if descriptorType != CV_32F:
            raise ValueError(f"SIFT_create: descriptorType {descriptorType} is not supported (only CV_32F = {CV_32F})")
        if enable_precise_upscale:
            raise ValueError("SIFT_create: enable_precise_upscale is not supported")
        if not (1 <= int(max_w) <= MAX_SIDE and 1 <= int(max_h) <= MAX_SIDE):
            raise ValueError(f"SIFT_create: max_w x max_h {max_w}x{max_h} outside 1..{MAX_SIDE}")
        if int(max_candidates) < 0 or int(max_keypoints) < 0:
            raise ValueError(f"SIFT_create: max_candidates {max_candidates} / max_keypoints {max_keypoints} is negative (0: the default)")
        self.nfeatures, self.nOctaveLayers = nfeatures, nOctaveLayers
        self.contrastThreshold, self.edgeThreshold, self.sigma = float(contrastThreshold), float(edgeThreshold), float(sigma)
        self.max_candidates, self.max_keypoints = int(max_candidates), int(max_keypoints)
        self._setup(max_h, max_w, ctx)

    def _create(self, L, handle_ref):
        return L.sslam_sift_create(self.ctx.handle, self.max_w, self.max_h, self.nfeatures, self.nOctaveLayers,
                                   self.contrastThreshold, self.edgeThreshold, self.sigma, self.max_candidates,
                                   self.max_keypoints, handle_ref)

    def detect_arrays(self, img, mask=None):
        """-> (xy float32 [N,2], aux float32 [N,3] = size, angle, response, octave int32 [N], desc float32 [N,128])."""
        return self._detect_host(img, mask)

    def detectAndCompute(self, image, mask=None):
        """-> (list of KeyPoint with every field set, descriptors float32 [N, 128]); ([], None) without a keypoint.  KeyPoint is
        cv2.KeyPoint where OpenCV is installed, else the duck type of slam/core/types.py."""
        from .slam.core.types import KeyPoint
        xy, aux, octave, desc = self.detect_arrays(image, mask)
        if len(xy) == 0:
            return [], None
        kps = [KeyPoint(x, y, s, a, r, o, -1) for (x, y), (s, a, r), o in zip(xy.tolist(), aux.tolist(), octave.tolist())]
        return kps, desc

    def detect_dev(self, img_dev, h: int, w: int, c: int, xy_out_dev, aux_out_dev, octave_out_dev, desc_out_dev, n_out_dev):
        """Device-resident call: the `*_dev` arguments are device pointers (ints) - the image uint8 [h, w, c], xy float32
        [capacity, 2], aux float32 [capacity, 3], octave int32 [capacity], desc float32 [capacity, 128], the count int32 [1] -
        and everything stays on the device: `desc_out_dev` / `n_out_dev` are what `BFMatcher.match_dev` takes as `q_dev` /
        `m_dev` (NORM_L2, D = 128, `chain_rows` as its M), `xy_out_dev` what `epipolar.filter_matches_dev` takes as `xy1_dev`.
        Enqueued on the instance's context stream, no synchronisation; a voided frame writes the count 0 and sets `overflow()`."""
        self._check_dev_size(h, w)
        P = _native.ptr
        _native.check(_native.lib().sslam_sift_detect_dev(self._instance(), P(img_dev), int(h), int(w), int(c), P(xy_out_dev),
                                                          P(aux_out_dev), P(octave_out_dev), P(desc_out_dev), P(n_out_dev)),
                      "sslam_sift_detect_dev")

    # test hooks (include/sslam_hip.h: sslam_sift_octave_info, sslam_sift_stage_read)
    def octave_info(self, octave: int):
        v = np.zeros(8, np.int32)
        _native.check(_native.lib().sslam_sift_octave_info(self._instance(), int(octave), _native.ptr(v)), "sslam_sift_octave_info")
        return dict(zip(("w", "h", "octaves", "layers", "interior", "threshold", "max_candidates", "max_keypoints"), v.tolist()))

    def stage_read(self, octave: int):
        """-> dict(gauss float32 [L + 3, h, w], dog float32 [L + 2, h, w] of the octave; of the whole last frame: cand int32
        [K, 4] (octave, layer, r, c), ref int32 [K, 8], hist float32 [K, 40], counts int32 [4])."""
        i = self.octave_info(octave)
        L = i["layers"]
        gauss, dog = np.empty((L, i["h"], i["w"]), np.float32), np.empty((L - 1, i["h"], i["w"]), np.float32)
        cap = max(i["max_candidates"], 1)
        cand, ref, hist = np.zeros((cap, 4), np.int32), np.zeros((cap, 8), np.int32), np.zeros((cap, 40), np.float32)
        counts = np.zeros(4, np.int32)
        P = _native.ptr
        _native.check(_native.lib().sslam_sift_stage_read(self._instance(), int(octave), P(gauss), P(dog), P(cand), P(ref), P(hist),
                                                          P(counts)), "sslam_sift_stage_read")
        k = min(int(counts[0]), cap)
        return dict(gauss=gauss, dog=dog, cand=cand[:k].copy(), ref=ref[:k].copy(), hist=hist[:k].copy(), counts=counts)


def SIFT_create(nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, descriptorType=CV_32F,
                enable_precise_upscale=False, *, max_h=2160, max_w=4096, max_candidates=0, max_keypoints=0, ctx=None):
    """`cv2.SIFT_create` with the same positional arguments -> SIFT."""
    return SIFT(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma, descriptorType, enable_precise_upscale,
                max_h=max_h, max_w=max_w, max_candidates=max_candidates, max_keypoints=max_keypoints, ctx=ctx)
