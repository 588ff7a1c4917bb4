"""Lens undistortion on the HIP backend.

Stands in for the three OpenCV calls the reference's frame loop makes when the camera has distortion
(slam/monocular/main_revamped.py:310-316, :324):

    new_K, _ = cv2.getOptimalNewCameraMatrix(K, D, (W0, H0), alpha=0, newImgSize=(W0, H0))
    mapx, mapy = cv2.initUndistortRectifyMap(K, D, None, new_K, (W0, H0), cv2.CV_32FC1)
    img = cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR)                 # every frame

as

    und = undistort.Undistorter(K, D, (W0, H0)); K = und.new_K; img = und.remap(img)

`get_optimal_new_camera_matrix` is numpy (a one-off on 81 points, fp64); the maps and the per-frame remap are kernels
(csrc/undistort_kernels.hip).  The array `Undistorter.remap` returns is the caller's and READ-ONLY: its bytes are also still on
the device, and `feature_extractor` handed exactly that array reads them there instead of uploading the image again
(feature_ring.py).  Parity with cv2 is unpinned (tests/undistort_ref.py restates the functions and names what could not be
confirmed).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _native

MAX_SIDE = 16384
GRID = 9                     # getOptimalNewCameraMatrix samples a 9 x 9 grid of image points
INVERSE_ITERS = 5            # undistortPoints' default criteria: five fixed-point iterations


def _coefficients(D):
    """D flattened -> float64 [4 | 5 | 8] (None / empty: four zeros).  12 / 14 coefficients (thin prism, tilt) are outside
    this backend's scope."""
    d = np.zeros(4) if D is None else np.asarray(D, np.float64).reshape(-1)
    if d.size == 0:
        d = np.zeros(4)
    if d.size in (12, 14):
        raise NotImplementedError(f"{d.size} distortion coefficients: the thin-prism / tilt terms of OpenCV's model are outside "
                                  "this backend's scope (4, 5 or 8 coefficients)")
    if d.size not in (4, 5, 8):
        raise ValueError(f"{d.size} distortion coefficients (want 4, 5 or 8: k1 k2 p1 p2 [k3 [k4 k5 k6]])")
    return np.ascontiguousarray(d)


def _k8(d):
    k = np.zeros(8)
    k[:d.size] = d
    return k


def _size(size):
    W, H = (int(v) for v in size)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"image size {W}x{H} outside 1..{MAX_SIDE}")
    return W, H


def _matrix3(M, what):
    M = np.asarray(M, np.float64)
    if M.shape != (3, 3):
        raise ValueError(f"{what} must be 3 x 3, got {M.shape}")
    return np.ascontiguousarray(M)


def _undistort_grid(K, k, W, H, P):
    """The 9 x 9 grid of image points (x (W - 1) / 8 in float32: exact for every legal size) through cv2.undistortPoints in
    double (five iterations of the inverse model, no early exit); P None: normalised coordinates, else projected by P
    -> [81, 2] float64."""
    j = np.arange(GRID, dtype=np.float32)
    gx = j * np.float32(W - 1) / np.float32(GRID - 1)
    gy = j * np.float32(H - 1) / np.float32(GRID - 1)
    u = np.tile(gx, GRID).astype(np.float64)
    v = np.repeat(gy, GRID).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x0 = (u - cx) / fx
    y0 = (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    for _ in range(INVERSE_ITERS):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        neg = icdist < 0                                 # OpenCV gives up on such a point: the undistorted value is x0, y0
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(neg, x0, (x0 - dx) * icdist)
        y = np.where(neg, y0, (y0 - dy) * icdist)
    if P is not None:
        x = x * P[0, 0] + P[0, 2]
        y = y * P[1, 1] + P[1, 2]
    return np.stack([x, y], 1)


def _rectangles(K, k, W, H, P):
    """inner: the largest rectangle inside the undistorted image's border (from the grid's outer rows / columns), outer: the
    grid's bounding box; each (x, y, w, h)."""
    p = _undistort_grid(K, k, W, H, P).reshape(GRID, GRID, 2)
    ix0, ix1 = p[:, 0, 0].max(), p[:, -1, 0].min()
    iy0, iy1 = p[0, :, 1].max(), p[-1, :, 1].min()
    ox0, ox1 = p[..., 0].min(), p[..., 0].max()
    oy0, oy1 = p[..., 1].min(), p[..., 1].max()
    return (ix0, iy0, ix1 - ix0, iy1 - iy0), (ox0, oy0, ox1 - ox0, oy1 - oy0)


def get_optimal_new_camera_matrix(K, D, size, alpha: float = 0.0, new_size=None):
    """`cv2.getOptimalNewCameraMatrix(K, D, size, alpha, newImgSize)` with centerPrincipalPoint=False -> (new_K [3,3] float64,
    roi (x, y, w, h)).  size / new_size: (W, H)."""
    K = _matrix3(K, "K")
    k = _k8(_coefficients(D))
    W, H = _size(size)
    nW, nH = _size(new_size) if new_size is not None and tuple(new_size) != (0, 0) else (W, H)
    alpha = float(alpha)
    inner, outer = _rectangles(K, k, W, H, None)
    fx0, fy0 = (nW - 1) / inner[2], (nH - 1) / inner[3]
    cx0, cy0 = -fx0 * inner[0], -fy0 * inner[1]
    fx1, fy1 = (nW - 1) / outer[2], (nH - 1) / outer[3]
    cx1, cy1 = -fx1 * outer[0], -fy1 * outer[1]
    M = np.eye(3)
    M[0, 0] = fx0 * (1 - alpha) + fx1 * alpha
    M[1, 1] = fy0 * (1 - alpha) + fy1 * alpha
    M[0, 2] = cx0 * (1 - alpha) + cx1 * alpha
    M[1, 2] = cy0 * (1 - alpha) + cy1 * alpha
    inner, _ = _rectangles(K, k, W, H, M)
    x, y = int(np.ceil(inner[0])), int(np.ceil(inner[1]))
    w, h = int(np.floor(inner[2])), int(np.floor(inner[3]))
    x1, y1 = min(x + w, nW), min(y + h, nH)              # r &= Rect(0, 0, nW, nH)
    x, y = max(x, 0), max(y, 0)
    roi = (x, y, x1 - x, y1 - y) if x1 > x and y1 > y else (0, 0, 0, 0)
    return M, roi


def _check_image(img):
    """-> (H, W, C) of a uint8 image with 1, 3 or 4 channels (no library call, no copy)."""
    if not isinstance(img, np.ndarray):
        img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError("remap expects a uint8 image (cv2.imread output)")
    if img.ndim == 2:
        Hs, Ws, Cn = img.shape[0], img.shape[1], 1
    elif img.ndim == 3:
        Hs, Ws, Cn = img.shape
    else:
        raise ValueError(f"unsupported image shape {img.shape}")
    if Cn not in (1, 3, 4):
        raise ValueError(f"{Cn} channels (want 1, 3 or 4)")
    if not (1 <= Hs <= MAX_SIDE and 1 <= Ws <= MAX_SIDE):
        raise ValueError(f"image size {Ws}x{Hs} outside 1..{MAX_SIDE}")
    return img, Hs, Ws, Cn


def _check_maps(mapx, mapy):
    for m in (mapx, mapy):
        if not isinstance(m, np.ndarray) or m.dtype != np.float32:
            raise TypeError("maps must be float32 arrays (cv2.CV_32FC1)")
    if mapx.ndim != 2 or mapx.shape != mapy.shape:
        raise ValueError(f"maps must be two [H, W] arrays of one shape, got {mapx.shape} and {mapy.shape}")
    _size((mapx.shape[1], mapx.shape[0]))


_returned = {}               # id(array remap() returned) -> (weak reference to it, weak reference to its Undistorter)


def device_copy(img, ctx):
    """The device address that holds `img`'s bytes if `img` is exactly the array the `Undistorter` of context `ctx` returned
    last (still read-only, so the content is the one produced), else None.  The flag is read NOW: a caller who switched it
    off, wrote into the array and switched it on again is not seen (the array owns its data) - the same trust the ring
    places in its descriptor arrays; INTEGRATION.md says so."""
    entry = _returned.get(id(img))
    if entry is None or entry[0]() is not img or img.flags.writeable:
        return None
    und = entry[1]()
    if und is None or und.ctx is not ctx or und.handle is None or und._last is None or und._last[0]() is not img:
        return None
    return und._last[1]


class Undistorter:
    """Maps of one camera on the device and the remap through them.  size: (W, H) of the undistorted image."""

    def __init__(self, K, D, size, alpha: float = 0.0, R=None, new_K=None, ctx=None):
        self.handle = None
        K = _matrix3(K, "K")
        d = _coefficients(D)
        W, H = _size(size)
        Rm = None if R is None else _matrix3(R, "R")
        if new_K is None:
            new_K, self.roi = get_optimal_new_camera_matrix(K, d, (W, H), alpha)
        else:
            new_K, self.roi = _matrix3(new_K, "new_K").copy(), None
        self.K, self.D, self.new_K, self.size = K, d, new_K, (W, H)
        self._init_buffers(ctx)
        h = C.c_void_p()
        P = _native.ptr
        nk = np.ascontiguousarray(new_K, np.float64).reshape(9)      # (a copy must live across the call)
        _native.check(_native.lib().sslam_undistort_create(self.ctx.handle, P(K.reshape(9)), P(d), int(d.size),
                                                           P(Rm.reshape(9)) if Rm is not None else None, P(nk), W, H, C.byref(h)),
                      "sslam_undistort_create")
        self.handle = h

    def _init_buffers(self, ctx):
        self.ctx = ctx or _native.default_context()
        self._src, self._src_cap = 0, 0                  # the uploaded source image
        self._dst, self._dst_cap = [0, 0], [0, 0]        # two results: the one being extracted and the one being produced
        self._turn = 0
        self._last = None                                # (weak reference to the last returned array, its device address)

    @classmethod
    def from_maps(cls, mapx, mapy, ctx=None):
        """The instance of `cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR)` for any float32 maps [H, W]."""
        _check_maps(mapx, mapy)
        self = cls.__new__(cls)
        self.handle = None
        H, W = mapx.shape
        self.K = self.D = self.new_K = self.roi = None
        self.size = (W, H)
        self._init_buffers(ctx)
        h = C.c_void_p()
        P = _native.ptr
        mx, my = np.ascontiguousarray(mapx), np.ascontiguousarray(mapy)      # (a view's copy must live across the call)
        _native.check(_native.lib().sslam_undistort_create_from_maps(self.ctx.handle, P(mx), P(my), W, H, C.byref(h)),
                      "sslam_undistort_create_from_maps")
        self.handle = h
        return self

    def close(self):
        if getattr(self, "handle", None):
            _native.lib().sslam_undistort_destroy(self.handle)       # (drains the stream: the buffers below are idle)
            self.handle = None
            self._last = None
            for p in [self._src, *self._dst]:
                if p:
                    self.ctx.free(p)
            self._src, self._dst = 0, [0, 0]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def maps(self):
        """(mapx, mapy) float32 [H, W], as cv2.initUndistortRectifyMap(..., cv2.CV_32FC1) returns them."""
        W, H = self.size
        mx, my = np.empty((H, W), np.float32), np.empty((H, W), np.float32)
        P = _native.ptr
        _native.check(_native.lib().sslam_undistort_maps_read(self.handle, P(mx), P(my), None, None), "sslam_undistort_maps_read")
        return mx, my

    def fixed_maps(self):
        """(ixy int16 [H, W, 2], alpha uint16 [H, W]): cv2.convertMaps' fixed-point form, alpha = fy * 32 + fx."""
        W, H = self.size
        ixy, al = np.empty((H, W, 2), np.int16), np.empty((H, W), np.uint16)
        P = _native.ptr
        _native.check(_native.lib().sslam_undistort_maps_read(self.handle, None, None, P(ixy), P(al)), "sslam_undistort_maps_read")
        return ixy, al

    def remap_dev(self, src_dev, Hs, Ws, Cn, dst_dev):
        """Enqueue only: src_dev uint8 [Hs][Ws][Cn] -> dst_dev uint8 [H][W][Cn] (16-byte aligned), both on the device."""
        P = _native.ptr
        _native.check(_native.lib().sslam_undistort_remap_dev(self.handle, P(int(src_dev)), int(Hs), int(Ws), int(Cn),
                                                              P(int(dst_dev))), "sslam_undistort_remap_dev")

    def remap_host(self, img):
        """The library's host entry (its own staging, nothing remembered) -> a fresh writable array."""
        img, Hs, Ws, Cn = _check_image(img)
        W, H = self.size
        src = np.ascontiguousarray(img)
        out = np.empty((H, W) if img.ndim == 2 else (H, W, Cn), np.uint8)
        P = _native.ptr
        _native.check(_native.lib().sslam_undistort_remap_host(self.handle, P(src), Hs, Ws, Cn, P(out)), "sslam_undistort_remap_host")
        return out

    def remap(self, img):
        """`cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR)` (BORDER_CONSTANT, value 0) -> a fresh READ-ONLY array of the
        caller's; the device keeps the same bytes until the call after the next one."""
        img, Hs, Ws, Cn = _check_image(img)
        ctx = self.ctx
        W, H = self.size
        src = np.ascontiguousarray(img)
        if src.nbytes > self._src_cap:
            if self._src:
                ctx.sync(); ctx.free(self._src)
            self._src_cap = src.nbytes
            self._src = ctx.malloc(self._src_cap)
        t = self._turn = self._turn ^ 1
        nbytes = H * W * Cn
        if nbytes > self._dst_cap[t]:
            if self._dst[t]:
                ctx.sync(); ctx.free(self._dst[t])
            self._dst_cap[t] = H * W * 4
            self._dst[t] = ctx.malloc(self._dst_cap[t])
        out = np.empty((H, W) if img.ndim == 2 else (H, W, Cn), np.uint8)
        ctx.h2d_async(self._src, src)
        self.remap_dev(self._src, Hs, Ws, Cn, self._dst[t])
        ctx.d2h(out, self._dst[t])                       # (synchronises: `src` has been read, `out` is complete)
        out.setflags(write=False)
        key = id(out)
        self._last = (weakref.ref(out, lambda ref, key=key: _returned.get(key, (None,))[0] is ref and _returned.pop(key, None)),
                      self._dst[t])
        _returned[key] = (self._last[0], weakref.ref(self))
        return out


# `remap` holds STRONG references to the last few callers' map pairs, a copy of each and a device instance per pair: at
# 640 x 480 about 2.5 MB of host memory and 4.3 MB of device memory per entry, at most _BY_MAPS_KEEP entries
_by_maps = []                # [(mapx, mapy, copy of mapx, copy of mapy, context, Undistorter)] of `remap`, most recent first
_BY_MAPS_KEEP = 4


def remap(img, mapx, mapy, ctx=None):
    """The literal stand-in for `cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR)`.  One instance is kept per pair of map arrays:
    the pair is recognised by identity AND by a read of both arrays against the copies remembered with it (an array edited in
    place is a new pair)."""
    _check_image(img)                                    # (again in und.remap: here it comes before an instance is built)
    _check_maps(mapx, mapy)
    ctx = ctx or _native.default_context()
    for i, (mx, my, cx, cy, c, und) in enumerate(_by_maps):
        if mx is mapx and my is mapy and c is ctx and und.handle is not None:
            if np.array_equal(mx, cx, equal_nan=True) and np.array_equal(my, cy, equal_nan=True):
                if i:
                    _by_maps.insert(0, _by_maps.pop(i))
                return und.remap(img)
            _by_maps.pop(i)[5].close()                   # the arrays were edited in place: a new pair
            break
    und = Undistorter.from_maps(mapx, mapy, ctx)
    _by_maps.insert(0, (mapx, mapy, mapx.copy(), mapy.copy(), ctx, und))
    for old in _by_maps[_BY_MAPS_KEEP:]:
        old[5].close()
    del _by_maps[_BY_MAPS_KEEP:]
    return und.remap(img)
