"""Pyramidal Lucas-Kanade on the HIP backend.

Stands in for the KLT front end of the reference's tracking loop (slam/monocular/main4.py:241-252, :395-433):

    img1_gray = cv2.cvtColor(img1, cv2.COLOR_BGR2GRAY); img2_gray = ...
    next_pts, st, err = cv2.calcOpticalFlowPyrLK(img1_gray, img2_gray, prev_pts, None, **lk_params)
    back_pts, st_back, _ = cv2.calcOpticalFlowPyrLK(img2_gray, img1_gray, next_pts, None, **lk_params)
    ... status / err / forward-backward masks ... pts0, pts1

as

    klt = optical_flow.KLTTracker((W, H))            # once; main4's parameters are the defaults
    klt.push(img2)                                   # once per frame: grey, pyramid, derivatives stay on the device
    pts0, pts1, counts = klt.track(prev_pts)         # counts = (raw, st1, err_ok, fb_ok, kept) of the [KLT] log line

`calc_optical_flow_pyr_lk` is the literal stand-in for the cv2 call (it builds both pyramids on every call) and `bgr_to_gray`
the grey conversion on its own.  The kernels are csrc/klt_kernels.hip.  Parity with cv2 is unpinned (tests/klt_ref.py restates
the functions and names what could not be confirmed).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

MAX_SIDE = 16384
MIN_WIN, MAX_WIN = 3, 31
MAX_LEVEL = 10
MAX_POINTS = 1 << 20
OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8
TERM_CRITERIA_COUNT, TERM_CRITERIA_EPS = 1, 2
MASK_STATUS, MASK_ERR, MASK_FB, MASK_KEPT = 1, 2, 4, 8


def _check_image(img):
    """-> (contiguous uint8 image, H, W, C) with 1, 3 or 4 channels (no library call)."""
    if not isinstance(img, np.ndarray):
        img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError("optical flow expects a uint8 image (16-bit and float images are outside this backend's scope)")
    if img.ndim == 2:
        H, W, Cn = img.shape[0], img.shape[1], 1
    elif img.ndim == 3:
        H, W, Cn = img.shape
    else:
        raise ValueError(f"unsupported image shape {img.shape}")
    if Cn not in (1, 3, 4):
        raise ValueError(f"{Cn} channels (want 1, 3 or 4)")
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"image size {W}x{H} outside 1..{MAX_SIDE}")
    return np.ascontiguousarray(img), H, W, Cn


def _check_window(winSize, maxLevel):
    ww, wh = (int(v) for v in winSize)
    if not (ww & 1 and wh & 1):
        raise ValueError(f"winSize {ww}x{wh} has an even side (this backend takes odd sides)")
    if not (MIN_WIN <= ww <= MAX_WIN and MIN_WIN <= wh <= MAX_WIN):
        raise ValueError(f"winSize {ww}x{wh} outside {MIN_WIN}..{MAX_WIN}")
    maxLevel = int(maxLevel)
    if not 0 <= maxLevel <= MAX_LEVEL:
        raise ValueError(f"maxLevel {maxLevel} outside 0..{MAX_LEVEL}")
    return ww, wh, maxLevel


def _check_points(pts, what="prev_pts"):
    """[N,2] or [N,1,2] -> contiguous float32 [N,2]."""
    p = np.asarray(pts, np.float32)
    if p.size == 0:
        return np.empty((0, 2), np.float32)
    if not ((p.ndim == 2 and p.shape[1] == 2) or (p.ndim == 3 and p.shape[1:] == (1, 2))):
        raise ValueError(f"{what} must be [N,2] or [N,1,2], got {p.shape}")
    return np.ascontiguousarray(p.reshape(-1, 2))


def _check_criteria(criteria):
    typ, count, eps = criteria
    typ, count, eps = int(typ), int(count), float(eps)
    if not np.isfinite(eps):
        raise ValueError("criteria epsilon is not finite")
    return typ, count, eps


def bgr_to_gray(img, ctx=None):
    """`cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)` for uint8 [H,W,3] (BGR) or [H,W,4] (BGRA) on the device -> uint8 [H,W];
    a 2-D image passes through."""
    img, H, W, Cn = _check_image(img)
    if img.ndim == 2:
        return img
    ctx = ctx or _native.default_context()
    out = np.empty((H, W), np.uint8)
    P = _native.ptr
    _native.check(_native.lib().sslam_klt_gray_host(ctx.handle, P(img), H, W, Cn, P(out)), "sslam_klt_gray_host")
    return out


class _Instance:
    """sslam_klt: two frames' pyramids on the device and the tracker over them."""

    def __init__(self, size, winSize, maxLevel, max_points, ctx):
        self.handle = None
        W, H = (int(v) for v in size)
        if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
            raise ValueError(f"image size {W}x{H} outside 1..{MAX_SIDE}")
        ww, wh, maxLevel = _check_window(winSize, maxLevel)
        max_points = int(max_points)
        if not 1 <= max_points <= MAX_POINTS:
            raise ValueError(f"capacity of {max_points} points outside 1..{MAX_POINTS}")
        self.size, self.win, self.max_level, self.max_points = (W, H), (ww, wh), maxLevel, max_points
        self.ctx = ctx or _native.default_context()
        self.pushes = 0
        h = C.c_void_p()
        _native.check(_native.lib().sslam_klt_create(self.ctx.handle, W, H, max_points, ww, wh, maxLevel, C.byref(h)), "sslam_klt_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            _native.lib().sslam_klt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _alive(self):
        if not self.handle:
            raise RuntimeError("the tracker is closed")

    def _check_frame(self, H, W):
        if (W, H) != self.size:
            raise ValueError(f"frame size {W}x{H} is not the tracker's {self.size[0]}x{self.size[1]}")

    def push(self, img):
        img, H, W, Cn = _check_image(img)                # (a view's copy must live across the call: `img` holds it)
        self._check_frame(H, W)
        self._alive()
        _native.check(_native.lib().sslam_klt_push_host(self.handle, _native.ptr(img), H, W, Cn), "sslam_klt_push_host")
        self.pushes += 1

    def push_dev(self, img_dev, H, W, Cn):
        """Enqueue only: uint8 [H][W][Cn] at device address `img_dev`, which must stay untouched until the stream passed it."""
        H, W, Cn = int(H), int(W), int(Cn)
        if Cn not in (1, 3, 4):
            raise ValueError(f"{Cn} channels (want 1, 3 or 4)")
        self._check_frame(H, W)
        self._alive()
        _native.check(_native.lib().sslam_klt_push_dev(self.handle, _native.ptr(int(img_dev)), H, W, Cn), "sslam_klt_push_dev")
        self.pushes += 1

    def _check_n(self, n):
        if n > self.max_points:
            raise ValueError(f"{n} points exceed the tracker's capacity of {self.max_points}")
        if self.pushes < 2:
            raise RuntimeError("track needs two pushed frames")
        self._alive()

    def flow(self, prev_pts, init_pts, criteria, flags, min_eig, reverse=False):
        """previous -> current (or the reverse) -> (next_pts [N,2] float32, status [N] uint8, err [N] float32)."""
        n = len(prev_pts)
        self._check_n(n)
        typ, count, eps = criteria
        nxt, st, err = np.empty((n, 2), np.float32), np.empty(n, np.uint8), np.empty(n, np.float32)
        P = _native.ptr
        _native.check(_native.lib().sslam_klt_track_host(self.handle, int(bool(reverse)), n, P(prev_pts), P(init_pts), int(flags), typ, count,
                                                         eps, float(min_eig), P(nxt), P(st), P(err)), "sslam_klt_track_host")
        return nxt, st, err

    def flow_fb(self, prev_pts, criteria, min_eig, err_thresh, fb_thresh):
        """-> (pts0 [K,2], pts1 [K,2], counts (raw, st1, err_ok, fb_ok, kept), next_pts [N,2], mask [N] uint8)."""
        n = len(prev_pts)
        self._check_n(n)
        typ, count, eps = criteria
        p0, p1, nxt = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32), np.empty((n, 2), np.float32)
        counts, mask = np.zeros(5, np.int32), np.empty(n, np.uint8)
        P = _native.ptr
        _native.check(_native.lib().sslam_klt_track_fb_host(self.handle, n, P(prev_pts), typ, count, eps, float(min_eig), float(err_thresh),
                                                            float(fb_thresh), P(nxt), P(p0), P(p1), P(counts), P(mask)),
                      "sslam_klt_track_fb_host")
        kept = int(counts[4])
        return p0[:kept].copy(), p1[:kept].copy(), tuple(int(v) for v in counts), nxt, mask

    def flow_dev(self, n, prev_dev, init_dev, criteria, flags, min_eig, next_dev, status_dev, err_dev, reverse=False):
        """Enqueue only: `flow` on device addresses (prev / init / next float32 [n,2], status uint8 [n], err float32 [n])."""
        self._check_n(int(n))
        typ, count, eps = criteria
        P = _native.ptr
        _native.check(_native.lib().sslam_klt_track_dev(self.handle, int(bool(reverse)), int(n), P(int(prev_dev)),
                                                        P(int(init_dev)) if init_dev else None, int(flags), typ, count, eps, float(min_eig),
                                                        P(int(next_dev)), P(int(status_dev)), P(int(err_dev))), "sslam_klt_track_dev")

    def flow_fb_dev(self, n, prev_dev, criteria, min_eig, err_thresh, fb_thresh, pts0_dev, pts1_dev, counts_dev, next_dev=0, mask_dev=0):
        """Enqueue only: `flow_fb` on device addresses; pts0 / pts1 float32 [n,2] (the first counts[4] pairs are written), counts
        int32 [5], optional next float32 [n,2] and mask uint8 [n].  Everything stays on the device for the next stage."""
        self._check_n(int(n))
        typ, count, eps = criteria
        P = _native.ptr
        _native.check(_native.lib().sslam_klt_track_fb_dev(self.handle, int(n), P(int(prev_dev)), typ, count, eps, float(min_eig),
                                                           float(err_thresh), float(fb_thresh), P(int(next_dev)) if next_dev else None,
                                                           P(int(pts0_dev)), P(int(pts1_dev)), P(int(counts_dev)),
                                                           P(int(mask_dev)) if mask_dev else None), "sslam_klt_track_fb_dev")

    def info(self, previous=False):
        """(effective maxLevel, W, H) of the current or the previous frame."""
        self._alive()
        top, w, h = C.c_int(), C.c_int(), C.c_int()
        _native.check(_native.lib().sslam_klt_info(self.handle, int(bool(previous)), C.byref(top), C.byref(w), C.byref(h)), "sslam_klt_info")
        return top.value, w.value, h.value

    def levels(self, previous=False):
        """Test hook -> {"gray": uint8 [H,W], "levels": [uint8 [h_l,w_l]], "dx": [int16 ...], "dy": [int16 ...]} of the current
        or the previous frame (level 0 IS the grey image)."""
        top, w, h = self.info(previous)
        out = {"levels": [], "dx": [], "dy": []}
        P = _native.ptr
        for level in range(top + 1):
            img, dx, dy = np.empty((h, w), np.uint8), np.empty((h, w), np.int16), np.empty((h, w), np.int16)
            _native.check(_native.lib().sslam_klt_levels_read(self.handle, int(bool(previous)), level, P(img), P(dx), P(dy)),
                          "sslam_klt_levels_read")
            out["levels"].append(img); out["dx"].append(dx); out["dy"].append(dy)
            w, h = (w + 1) // 2, (h + 1) // 2
        out["gray"] = out["levels"][0]
        return out


class KLTTracker(_Instance):
    """The KLT front end of one camera.  size: (W, H) of the frames; the defaults are main4's (`:242-252`).  `push(img)` once per
    frame (BGR, BGRA or grey uint8), `track(prev_pts)` from the frame before the last push to the last one."""

    def __init__(self, size, winSize=(21, 21), maxLevel=3, criteria=(TERM_CRITERIA_EPS | TERM_CRITERIA_COUNT, 30, 1e-3),
                 minEigThreshold=1e-4, err_thresh=12.0, fb_thresh=1.5, ctx=None, max_points=4096):
        self.handle = None
        self.criteria = _check_criteria(criteria)
        self.min_eig, self.err_thresh, self.fb_thresh = float(minEigThreshold), float(err_thresh), float(fb_thresh)
        super().__init__(size, winSize, maxLevel, max_points, ctx)

    def push(self, img):
        """An array that `undistort.Undistorter.remap` of the same context just returned is read where the remap kernel left
        it instead of being uploaded again."""
        from . import undistort
        dev = undistort.device_copy(img, self.ctx) if isinstance(img, np.ndarray) else None
        if dev is not None:
            _, H, W, Cn = _check_image(img)
            self.push_dev(dev, H, W, Cn)
            self.ctx.sync()                              # (the Undistorter reuses that buffer two remaps later)
        else:
            super().push(img)

    def track(self, prev_pts, with_masks=False):
        """main4.py:402-433 -> (pts0 [K,2], pts1 [K,2], (raw, st1, err_ok, fb_ok, kept)); with_masks adds next_pts [N,2] and the
        per-point mask bytes (MASK_STATUS | MASK_ERR | MASK_FB | MASK_KEPT)."""
        pts = _check_points(prev_pts)
        if self.pushes < 2:
            raise RuntimeError("track needs two pushed frames")
        if len(pts) == 0:
            e = np.empty((0, 2), np.float32)
            res = (e, e.copy(), (0, 0, 0, 0, 0))
            return res + (e.copy(), np.empty(0, np.uint8)) if with_masks else res
        p0, p1, counts, nxt, mask = self.flow_fb(pts, self.criteria, self.min_eig, self.err_thresh, self.fb_thresh)
        return (p0, p1, counts, nxt, mask) if with_masks else (p0, p1, counts)


_instances = {}              # (id(ctx), W, H, ww, wh, maxLevel) -> (ctx, _Instance) of `calc_optical_flow_pyr_lk`
_INSTANCES_KEEP = 4


def _instance(ctx, W, H, ww, wh, maxLevel, n):
    key = (id(ctx), W, H, ww, wh, maxLevel)
    entry = _instances.get(key)
    if entry is not None and entry[0] is ctx and entry[1].handle and entry[1].max_points >= n:
        _instances[key] = _instances.pop(key)            # most recent last
        return entry[1]
    if entry is not None:
        _instances.pop(key)[1].close()
    cap = 4096
    while cap < n:
        cap *= 2
    inst = _Instance((W, H), (ww, wh), maxLevel, cap, ctx)
    _instances[key] = (ctx, inst)
    while len(_instances) > _INSTANCES_KEEP:
        _instances.pop(next(iter(_instances)))[1].close()
    return inst


def calc_optical_flow_pyr_lk(prev_img, next_img, prev_pts, next_pts=None, winSize=(21, 21), maxLevel=3,
                             criteria=(TERM_CRITERIA_COUNT | TERM_CRITERIA_EPS, 30, 0.01), flags=0, minEigThreshold=1e-4, ctx=None):
    """The literal stand-in for `cv2.calcOpticalFlowPyrLK(prev_img, next_img, prev_pts, next_pts, ...)` with cv2's defaults
    -> (next_pts [N,1,2] float32, status [N,1] uint8, err [N,1] float32).  Images: uint8, grey, BGR or BGRA (cv2 takes grey; a
    colour image is converted as cv2.cvtColor would).  Both pyramids are built on every call; a frame loop keeps them with
    `KLTTracker`.  Instances are cached per (context, size, window, levels)."""
    prev_img, H, W, C0 = _check_image(prev_img)
    next_img, H1, W1, C1 = _check_image(next_img)
    if (H, W) != (H1, W1):
        raise ValueError(f"the two images differ in size: {W}x{H} and {W1}x{H1}")
    ww, wh, maxLevel = _check_window(winSize, maxLevel)
    flags = int(flags)
    if flags & ~(OPTFLOW_USE_INITIAL_FLOW | OPTFLOW_LK_GET_MIN_EIGENVALS):
        raise ValueError(f"flags {flags}: only OPTFLOW_USE_INITIAL_FLOW (4) and OPTFLOW_LK_GET_MIN_EIGENVALS (8) are known")
    criteria = _check_criteria(criteria)
    pts = _check_points(prev_pts)
    init = None
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        if next_pts is None:
            raise ValueError("OPTFLOW_USE_INITIAL_FLOW needs next_pts")
        init = _check_points(next_pts, "next_pts")
        if init.shape != pts.shape:
            raise ValueError(f"next_pts holds {len(init)} points, prev_pts {len(pts)}")
    n = len(pts)
    if n == 0:
        return np.empty((0, 1, 2), np.float32), np.empty((0, 1), np.uint8), np.empty((0, 1), np.float32)
    if n > MAX_POINTS:
        raise ValueError(f"{n} points exceed the backend's capacity of {MAX_POINTS}")
    ctx = ctx or _native.default_context()
    inst = _instance(ctx, W, H, ww, wh, maxLevel, n)
    _Instance.push(inst, prev_img)
    _Instance.push(inst, next_img)
    nxt, st, err = inst.flow(pts, init, criteria, flags, minEigThreshold)
    return nxt.reshape(n, 1, 2), st.reshape(n, 1), err.reshape(n, 1)
