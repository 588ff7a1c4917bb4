"""AKAZE on the HIP backend.

Stands in for `cv2.AKAZE_create()` as the reference's OpenCV branch uses it (`--detector akaze`): `_get_opencv_detector`
builds `cv2.AKAZE_create()` (slam/core/features_utils.py:39) and `feature_extractor` calls `.detectAndCompute(img, None)` on
it.  `AKAZE_create(...)` here is that object; with `bf_matcher.BFMatcher(NORM_HAMMING, crossCheck=True)` behind it the pair
runs without OpenCV, `detect_dev` -> `BFMatcher.match_dev(ctx, 61, ...)` -> `epipolar.filter_matches_dev` runs it without a
host round trip, and its 61-byte rows are what the Hamming branch of `reproject_and_match_2d3d` takes.

Semantics: include/sslam_hip.h (`sslam_akaze_create`) and tests/akaze_ref.py, which restates OpenCV's AKAZEFeatures and names
what could not be confirmed without cv2.  The arithmetic is defined (float32 one operation at a time, filter taps in ascending
order, the orientation windows and the M-LDB cell sums as exact integer sums, suppression as a predicate), so the kernels equal
the restatement bit for bit; the order of the output is defined too: class_id, then the candidate's row, then its column.
Ties at the `max_points` cut are kept, so more than max_points rows can come back.

Refused with a ValueError: a mask, a descriptor_type other than DESCRIPTOR_MLDB, descriptor_size != 0, descriptor_channels
!= 3, a diffusivity other than DIFF_PM_G2, a threshold that is not finite and positive, nOctaves / nOctaveLayers outside 1..8,
max_points other than -1 or >= 1, an image larger than max_w x max_h (never clipped); a non-uint8 image with a TypeError.  A
frame with more candidates than `max_candidates` or more keypoints than `max_keypoints` is voided and raises
`_native.NativeError`; it is never truncated.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._detector import CapacityDetector

# cv2's values
DESCRIPTOR_KAZE_UPRIGHT, DESCRIPTOR_KAZE, DESCRIPTOR_MLDB_UPRIGHT, DESCRIPTOR_MLDB = 2, 3, 4, 5
DIFF_PM_G1, DIFF_PM_G2, DIFF_WEICKERT, DIFF_CHARBONNIER = 0, 1, 2, 3
MAX_OCTAVES = MAX_OCTAVE_LAYERS = 8
MAX_POINTS = 1 << 20
MAX_SIDE = 16384
DESC_BYTES = 61
_INFO = ("w", "h", "levels", "octaves", "octave", "sigma_size", "border", "one_workgroup", "fed_steps", "interior", "max_candidates",
         "max_keypoints")


class AKAZE(CapacityDetector):
    """`cv2.AKAZE` with `detectAndCompute(image, mask=None)`.  The device instance is made at the first call."""
    NAME, PREFIX = "AKAZE", "akaze"
    ROWS = ((2,), np.float32), ((3,), np.float32), ((2,), np.int32), ((DESC_BYTES,), np.uint8)

    def __init__(self, descriptor_type=DESCRIPTOR_MLDB, descriptor_size=0, descriptor_channels=3, threshold=0.001, nOctaves=4, nOctaveLayers=4,
                 diffusivity=DIFF_PM_G2, max_points=-1, *, max_h=2160, max_w=4096, max_candidates=0, max_keypoints=0, ctx=None):
        if descriptor_type != DESCRIPTOR_MLDB:
            raise ValueError(f"AKAZE_create: descriptor_type {descriptor_type} is not supported (only DESCRIPTOR_MLDB = {DESCRIPTOR_MLDB})")
        if descriptor_size != 0:
            raise ValueError(f"AKAZE_create: descriptor_size {descriptor_size} is not supported (only 0: the full 486 bits)")
        if descriptor_channels != 3:
            raise ValueError(f"AKAZE_create: descriptor_channels {descriptor_channels} is not supported (only 3)")
        if not (float(threshold) > 0 and np.isfinite(threshold)):
            raise ValueError(f"AKAZE_create: threshold {threshold} is not positive and finite")
        nOctaves, nOctaveLayers, max_points = int(nOctaves), int(nOctaveLayers), int(max_points)
        if not 1 <= nOctaves <= MAX_OCTAVES:
            raise ValueError(f"AKAZE_create: nOctaves {nOctaves} outside 1..{MAX_OCTAVES}")
        if not 1 <= nOctaveLayers <= MAX_OCTAVE_LAYERS:
            raise ValueError(f"AKAZE_create: nOctaveLayers {nOctaveLayers} outside 1..{MAX_OCTAVE_LAYERS}")
        if diffusivity != DIFF_PM_G2:
            raise ValueError(f"AKAZE_create: diffusivity {diffusivity} is not supported (only DIFF_PM_G2 = {DIFF_PM_G2})")
        if not (max_points == -1 or 1 <= max_points <= MAX_POINTS):
            raise ValueError(f"AKAZE_create: max_points {max_points} is neither -1 nor in 1..{MAX_POINTS}")
        if not (1 <= int(max_w) <= MAX_SIDE and 1 <= int(max_h) <= MAX_SIDE):
            raise ValueError(f"AKAZE_create: max_w x max_h {max_w}x{max_h} outside 1..{MAX_SIDE}")
        if int(max_candidates) < 0 or int(max_keypoints) < 0:
            raise ValueError(f"AKAZE_create: max_candidates {max_candidates} / max_keypoints {max_keypoints} is negative (0: the default)")
        self.descriptor_type, self.descriptor_size, self.descriptor_channels = int(descriptor_type), 0, 3
        self.threshold, self.nOctaves, self.nOctaveLayers = float(threshold), nOctaves, nOctaveLayers
        self.diffusivity, self.max_points = int(diffusivity), max_points
        self.max_candidates, self.max_keypoints = int(max_candidates), int(max_keypoints)
        self._setup(max_h, max_w, ctx)

    def _create(self, L, handle_ref):
        return L.sslam_akaze_create(self.ctx.handle, self.max_w, self.max_h, self.descriptor_type, self.descriptor_size,
                                    self.descriptor_channels, self.threshold, self.nOctaves, self.nOctaveLayers, self.diffusivity,
                                    self.max_points, self.max_candidates, self.max_keypoints, handle_ref)

    def detect_arrays(self, img, mask=None):
        """-> (xy float32 [N,2], aux float32 [N,3] = size, angle, response, lvl int32 [N,2] = octave, class_id, desc uint8 [N,61])."""
        return self._detect_host(img, mask)

    def detectAndCompute(self, image, mask=None):
        """-> (list of KeyPoint with every field set, descriptors uint8 [N, 61]); ([], None) without a keypoint.  KeyPoint is
        cv2.KeyPoint where OpenCV is installed, else the duck type of slam/core/types.py."""
        from .slam.core.types import KeyPoint
        xy, aux, lvl, desc = self.detect_arrays(image, mask)
        if len(xy) == 0:
            return [], None
        kps = [KeyPoint(x, y, s, a, r, o, c) for (x, y), (s, a, r), (o, c) in zip(xy.tolist(), aux.tolist(), lvl.tolist())]
        return kps, desc

    def detect_dev(self, img_dev, h: int, w: int, c: int, xy_out_dev, aux_out_dev, lvl_out_dev, desc_out_dev, n_out_dev):
        """Device-resident call: the `*_dev` arguments are device pointers (ints) - the image uint8 [h, w, c], xy float32
        [capacity, 2], aux float32 [capacity, 3], lvl int32 [capacity, 2], desc uint8 [capacity, 61], the count int32 [1] - and
        everything stays on the device: `desc_out_dev` / `n_out_dev` are what `BFMatcher.match_dev` takes as `q_dev` / `m_dev`
        (NORM_HAMMING, D = 61, `chain_rows` as its M), `xy_out_dev` what `epipolar.filter_matches_dev` takes as `xy1_dev`.
        Enqueued on the instance's context stream, no synchronisation; a voided frame writes the count 0 and sets `overflow()`."""
        self._check_dev_size(h, w)
        P = _native.ptr
        _native.check(_native.lib().sslam_akaze_detect_dev(self._instance(), P(img_dev), int(h), int(w), int(c), P(xy_out_dev), P(aux_out_dev),
                                                           P(lvl_out_dev), P(desc_out_dev), P(n_out_dev)), "sslam_akaze_detect_dev")

    # test hooks (include/sslam_hip.h: sslam_akaze_level_info, sslam_akaze_stage_read)
    def level_info(self, level: int):
        v = np.zeros(12, np.int32)
        _native.check(_native.lib().sslam_akaze_level_info(self._instance(), int(level), _native.ptr(v)), "sslam_akaze_level_info")
        return dict(zip(_INFO, v.tolist()))

    def stage_read(self, level: int):
        """-> dict(Lt, Lflow (None at level 0), Lx, Ly, Ldet float32 [h, w] of the level; of the whole last frame: kcontrast float32
        [octaves], cand int32 [K, 4] (level, r, c, response bits), cflag int32 [K], kp uint32 [M, 8], kflag int32 [M], counts int32 [4])."""
        i = self.level_info(level)
        planes = [np.empty((i["h"], i["w"]), np.float32) for _ in range(5)]
        nc, nk = max(i["max_candidates"], 1), max(i["max_keypoints"], 1)
        kc, cand, cflag = np.zeros(8, np.float32), np.zeros((nc, 4), np.int32), np.zeros(nc, np.int32)
        kp, kflag, counts = np.zeros((nk, 8), np.uint32), np.zeros(nk, np.int32), np.zeros(4, np.int32)
        P = _native.ptr
        _native.check(_native.lib().sslam_akaze_stage_read(self._instance(), int(level), *[P(p) for p in planes], P(kc), P(cand), P(cflag), P(kp),
                                                           P(kflag), P(counts)), "sslam_akaze_stage_read")
        c, k = min(int(counts[0]), nc), min(int(counts[1]), nk)
        return dict(Lt=planes[0], Lflow=planes[1] if level > 0 else None, Lx=planes[2], Ly=planes[3], Ldet=planes[4], kcontrast=kc[:i["octaves"]].copy(),
                    cand=cand[:c].copy(), cflag=cflag[:c].copy(), kp=kp[:k].copy(), kflag=kflag[:k].copy(), counts=counts)


def AKAZE_create(descriptor_type=DESCRIPTOR_MLDB, descriptor_size=0, descriptor_channels=3, threshold=0.001, nOctaves=4, nOctaveLayers=4,
                 diffusivity=DIFF_PM_G2, max_points=-1, *, max_h=2160, max_w=4096, max_candidates=0, max_keypoints=0, ctx=None):
    """`cv2.AKAZE_create` with the same positional arguments -> AKAZE."""
    return AKAZE(descriptor_type, descriptor_size, descriptor_channels, threshold, nOctaves, nOctaveLayers, diffusivity, max_points,
                 max_h=max_h, max_w=max_w, max_candidates=max_candidates, max_keypoints=max_keypoints, ctx=ctx)
