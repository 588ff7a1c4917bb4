"""What the drop-in feature detectors (`orb.ORB`, `sift.SIFT`, `akaze.AKAZE`) share: the lazily made device instance and its
release, the image refusals, the host entry with its output arrays made once, the row bound of the device chain and the size
check of the device entry.  A subclass supplies `NAME` (as its messages spell it), `PREFIX` (of its C entries, `sslam_<PREFIX>_*`),
`ROWS` (the trailing shape and dtype of every output array, in the C entry's order), `_create(lib, handle_ref)` and - for a
detector whose lists have capacities - `CapacityDetector` as its base, which adds `candidate_capacity` and `overflow()`.  The
constructors (their validation and messages), `detect_arrays`, `detectAndCompute`, `detect_dev` and the test hooks stay with
each detector: their arguments and outputs differ."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native


class Detector:
    NAME = PREFIX = ""
    ROWS = ()
    HAS_CANDIDATES = False                 # sslam_<PREFIX>_capacity also reports the candidate capacity

    def _setup(self, max_h, max_w, ctx):
        """The state every detector has; called at the end of a constructor, touches no library."""
        self.max_h, self.max_w = int(max_h), int(max_w)
        self.ctx = ctx
        self.handle = None
        self.capacity = 0                  # rows of every output array
        self._out = None                   # the host entry's output arrays, made once ([capacity] rows, pages touched as used)

    def _entry(self, name):
        return getattr(_native.lib(), f"sslam_{self.PREFIX}_{name}"), f"sslam_{self.PREFIX}_{name}"

    def _instance(self):
        if self.handle is None:
            self.ctx = self.ctx or _native.default_context()
            h = C.c_void_p()
            _native.check(self._create(_native.lib(), C.byref(h)), f"sslam_{self.PREFIX}_create")
            self.handle = h
            rows, cand = C.c_int(0), C.c_int(0)
            fn, who = self._entry("capacity")
            _native.check(fn(h, C.byref(rows), C.byref(cand)) if self.HAS_CANDIDATES else fn(h, C.byref(rows)), who)
            self.capacity = int(rows.value)
            if self.HAS_CANDIDATES:
                self.candidate_capacity = int(cand.value)
        return self.handle

    def close(self):
        if getattr(self, "handle", None):
            self._entry("destroy")[0](self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _image(self, img, mask):
        """`img` as the contiguous uint8 [h, w, c] the library takes; anything else is refused, never cast or clipped."""
        who = f"{self.NAME}.detectAndCompute"
        if mask is not None:
            raise ValueError(f"{who}: a mask is not supported")
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise TypeError(f"{who}: image is {img.dtype}, want uint8")
        if img.ndim == 2:
            img = img[:, :, None]
        if img.ndim != 3 or img.shape[2] not in (1, 3, 4) or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError(f"{who}: image must be [h, w] or [h, w, 1 | 3 | 4], got shape {img.shape}")
        if img.shape[0] > self.max_h or img.shape[1] > self.max_w:
            raise ValueError(f"{who}: image {img.shape[1]}x{img.shape[0]} is larger than the instance's "
                             f"{self.max_w}x{self.max_h} (max_w x max_h)")
        return np.ascontiguousarray(img)

    def _detect_host(self, img, mask):
        """The host entry: -> a copy of the first N rows of every output array, in the order of `ROWS`."""
        img = self._image(img, mask)
        h = self._instance()
        if self._out is None:
            self._out = tuple(np.empty((self.capacity, *tail), dtype) for tail, dtype in self.ROWS)
        n = C.c_int32(0)
        P = _native.ptr
        fn, who = self._entry("detect_host")
        _native.check(fn(h, P(img), img.shape[0], img.shape[1], img.shape[2], *[P(a) for a in self._out], C.byref(n)), who)
        return tuple(a[:n.value].copy() for a in self._out)

    @property
    def chain_rows(self) -> int:
        """The row bound to hand `BFMatcher.match_dev` (M, N) and `epipolar.filter_matches_dev` (n_max) for this instance's
        device outputs: min(capacity, 65 536), the matcher's limit.  The arrays themselves hold `capacity` rows; the matcher
        clamps the device count to the bound, so of a frame with more keypoints than that (ORB: ties on a large frame, never a
        quota) only the first 65 536 in output order take part in the match."""
        from .bf_matcher import MAX_ROWS
        self._instance()
        return min(self.capacity, MAX_ROWS)

    def _check_dev_size(self, h, w):
        if not (1 <= int(h) <= self.max_h and 1 <= int(w) <= self.max_w):
            raise ValueError(f"{self.NAME}.detect_dev: image {w}x{h} is larger than the instance's {self.max_w}x{self.max_h}")


class CapacityDetector(Detector):
    """A detector whose candidate and keypoint lists have capacities (`max_candidates`, `max_keypoints`): a frame that exceeds
    one is voided, never truncated."""
    HAS_CANDIDATES = True

    def _setup(self, max_h, max_w, ctx):
        super()._setup(max_h, max_w, ctx)
        self.candidate_capacity = 0

    def overflow(self) -> int:
        """The sticky word: bit 0 - a frame had more candidates (SIFT: extrema) than `max_candidates`, bit 1 - more keypoints
        than `max_keypoints`; such a frame was voided.  Synchronises the stream."""
        v = C.c_int(0)
        fn, who = self._entry("overflow")
        _native.check(fn(self._instance(), C.byref(v)), who)
        return int(v.value)
