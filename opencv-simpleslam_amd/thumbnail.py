"""Keyframe thumbnails on the HIP backend: cv2.resize and a baseline JPEG encoder.

Stands in for the two OpenCV calls of `make_thumb` (slam/core/keyframe_utils.py:26-30):

    th = cv2.resize(bgr, hw)
    ok, enc = cv2.imencode('.jpg', th, [int(cv2.IMWRITE_JPEG_QUALITY), 70])

as

    th = thumbnail.resize(bgr, hw)
    ok, enc = thumbnail.imencode_jpg(th, 70)

or, without the resized image ever leaving the device, `Thumbnailer(max_src_wh, hw, 70).encode(bgr)`.  Resize, colour conversion,
4:2:0 subsampling, the forward DCT, quantisation, Huffman coding, byte stuffing and the header all run in csrc/thumb_kernels.hip;
csrc/thumb_plan.hpp holds the tables and the block layout.  A one-channel image gives a one-component JPEG, three or four
channels are B G R (A) as cv2 holds them, alpha dropped.  Parity with cv2 is unpinned (tests/thumb_ref.py restates every stage,
names what could not be confirmed; tests/test_thumb_ref.py measures the streams against Pillow's libjpeg-turbo).

Not built: INTER_AREA and the other interpolations, progressive or optimised-Huffman JPEG, chroma layouts other than 4:2:0, restart
intervals, EXIF, decoding, PNG.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

MAX_DST = 4096
MAX_SRC = 16384
BLOCK_BYTES = 416
STAGES = {"resized": 0, "y": 1, "cb": 2, "cr": 3, "coef": 4, "bitoff": 5}


def _check_create(max_src_wh, thumb_wh, quality):
    (mw, mh), (w, h), q = (int(v) for v in max_src_wh), (int(v) for v in thumb_wh), int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality {q} outside 1..100")
    if not (1 <= w <= MAX_DST and 1 <= h <= MAX_DST):
        raise ValueError(f"thumbnail size {w}x{h} outside 1..{MAX_DST}")
    if not (1 <= mw <= MAX_SRC and 1 <= mh <= MAX_SRC):
        raise ValueError(f"source size {mw}x{mh} outside 1..{MAX_SRC}")
    return (mw, mh), (w, h), q


def _check_image(img, max_wh=None):
    """-> (contiguous-able array, Hs, Ws, C) of a uint8 image with 1, 3 or 4 channels (no library call)."""
    if not isinstance(img, np.ndarray):
        img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError("expected a uint8 image (cv2.imread output)")
    if img.ndim == 2:
        Hs, Ws, Cn = img.shape[0], img.shape[1], 1
    elif img.ndim == 3:
        Hs, Ws, Cn = img.shape
    else:
        raise ValueError(f"unsupported image shape {img.shape}")
    if Cn not in (1, 3, 4):
        raise ValueError(f"{Cn} channels (want 1, 3 or 4)")
    if not (1 <= Hs <= MAX_SRC and 1 <= Ws <= MAX_SRC):
        raise ValueError(f"source size {Ws}x{Hs} outside 1..{MAX_SRC}")
    if max_wh is not None and (Ws > max_wh[0] or Hs > max_wh[1]):
        raise ValueError(f"source {Ws}x{Hs} is larger than the instance's {max_wh[0]}x{max_wh[1]}")
    return img, Hs, Ws, Cn


def geometry(w, h, channels):
    """The layout of one encode (thumb_plan.hpp: thumb_geom): padded planes and the number of 8 x 8 blocks."""
    ncomp = 1 if channels == 1 else 3
    mcu = 8 if ncomp == 1 else 16
    mcux, mcuy = -(-w // mcu), -(-h // mcu)
    return dict(ncomp=ncomp, yw=mcux * mcu, yh=mcuy * mcu, cw=0 if ncomp == 1 else mcux * 8, ch=0 if ncomp == 1 else mcuy * 8,
                blocks=mcux * mcuy * (1 if ncomp == 1 else 6))


class Thumbnailer:
    """One thumbnail size and quality on the device; any source up to max_src_wh = (W, H)."""

    def __init__(self, max_src_wh, thumb_wh=(640, 360), quality=70, ctx=None):
        self.handle = None
        self.max_src_wh, self.thumb_wh, self.quality = _check_create(max_src_wh, thumb_wh, quality)
        self.ctx = ctx or _native.default_context()
        h = C.c_void_p()
        _native.check(_native.lib().sslam_thumb_create(self.ctx.handle, *self.max_src_wh, *self.thumb_wh, self.quality, C.byref(h)),
                      "sslam_thumb_create")
        self.handle = h
        cap = C.c_int(0)
        _native.check(_native.lib().sslam_thumb_capacity(self.handle, C.byref(cap)), "sslam_thumb_capacity")
        self.capacity = int(cap.value)
        self._out = np.empty(self.capacity, np.uint8)
        self._last_c = 0

    def close(self):
        if getattr(self, "handle", None):
            _native.lib().sslam_thumb_destroy(self.handle)           # (drains the stream)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, img) -> bytes:
        """`cv2.imencode('.jpg', cv2.resize(img, thumb_wh), [cv2.IMWRITE_JPEG_QUALITY, quality])[1].tobytes()`"""
        img, Hs, Ws, Cn = _check_image(img, self.max_src_wh)
        src = np.ascontiguousarray(img)
        n = C.c_int(0)
        P = _native.ptr
        _native.check(_native.lib().sslam_thumb_encode_host(self.handle, P(src), Hs, Ws, Cn, P(self._out), self.capacity, C.byref(n)),
                      "sslam_thumb_encode_host")
        self._last_c = Cn
        return self._out[:n.value].tobytes()

    def encode_dev(self, src_dev, Hs, Ws, Cn, out_dev, nbytes_dev):
        """Enqueue only: src_dev uint8 [Hs][Ws][Cn] -> the stream at out_dev (`capacity` bytes) and its int32 length at nbytes_dev,
        all on the device."""
        if Cn not in (1, 3, 4):
            raise ValueError(f"{Cn} channels (want 1, 3 or 4)")
        P = _native.ptr
        _native.check(_native.lib().sslam_thumb_encode_dev(self.handle, P(int(src_dev)), int(Hs), int(Ws), int(Cn), P(int(out_dev)),
                                                           P(int(nbytes_dev))), "sslam_thumb_encode_dev")
        self._last_c = int(Cn)

    def resize(self, img):
        """`cv2.resize(img, thumb_wh)` (INTER_LINEAR) -> a fresh array with the image's channels."""
        img, Hs, Ws, Cn = _check_image(img, self.max_src_wh)
        src = np.ascontiguousarray(img)
        w, h = self.thumb_wh
        out = np.empty((h, w) if img.ndim == 2 else (h, w, Cn), np.uint8)
        P = _native.ptr
        _native.check(_native.lib().sslam_thumb_resize_host(self.handle, P(src), Hs, Ws, Cn, P(out)), "sslam_thumb_resize_host")
        return out

    def stage_read(self, which):
        """For tests, of the last encode: 'resized' | 'y' | 'cb' | 'cr' | 'coef' (int16 [blocks, 64], zigzag) | 'bitoff'."""
        k = STAGES[which] if isinstance(which, str) else int(which)
        if not self._last_c:
            raise ValueError("no encode yet")
        w, h = self.thumb_wh
        g = geometry(w, h, self._last_c)
        if k in (2, 3) and g["ncomp"] == 1:
            raise ValueError("the last encode had one component, there is no chroma plane")
        out = {0: lambda: np.empty((h, w) if self._last_c == 1 else (h, w, self._last_c), np.uint8),
               1: lambda: np.empty((g["yh"], g["yw"]), np.uint8), 2: lambda: np.empty((g["ch"], g["cw"]), np.uint8),
               3: lambda: np.empty((g["ch"], g["cw"]), np.uint8), 4: lambda: np.empty((g["blocks"], 64), np.int16),
               5: lambda: np.empty(g["blocks"], np.uint32)}[k]()
        _native.check(_native.lib().sslam_thumb_stage_read(self.handle, k, _native.ptr(out)), "sslam_thumb_stage_read")
        return out


_instances = {}              # (id(ctx), max source W, H, thumbnail w, h, quality) -> (ctx, Thumbnailer), most recent last
_INSTANCES_KEEP = 4


def cached(src_wh, thumb_wh, quality, ctx=None):
    """The `Thumbnailer` kept for (context, source size, thumbnail size, quality): made on first use, the least recently used of
    more than four closed."""
    ctx = ctx or _native.default_context()
    key = (id(ctx), *src_wh, *thumb_wh, quality)
    entry = _instances.get(key)
    if entry is not None and entry[0] is ctx and entry[1].handle is not None:
        _instances[key] = _instances.pop(key)
        return entry[1]
    if entry is not None:
        _instances.pop(key)[1].close()
    inst = Thumbnailer(src_wh, thumb_wh, quality, ctx)
    _instances[key] = (ctx, inst)
    while len(_instances) > _INSTANCES_KEEP:
        _instances.pop(next(iter(_instances)))[1].close()
    return inst


def resize(img, wh, ctx=None):
    """The literal stand-in for `cv2.resize(img, (w, h))` (uint8, INTER_LINEAR).  Instances are cached per (context, source size,
    size, quality)."""
    img, Hs, Ws, Cn = _check_image(img)
    src_wh, wh, _ = _check_create((Ws, Hs), wh, 95)
    return cached(src_wh, wh, 95, ctx).resize(img)


def imencode_jpg(img, quality=95, ctx=None):
    """The literal stand-in for `cv2.imencode('.jpg', img, [cv2.IMWRITE_JPEG_QUALITY, quality])` -> (True, uint8 [n]).  The
    image is encoded at its own size (the resize of the pipeline is the identity then)."""
    img, Hs, Ws, Cn = _check_image(img)
    src_wh, wh, q = _check_create((Ws, Hs), (Ws, Hs), quality)
    data = cached(src_wh, wh, q, ctx).encode(img)
    return True, np.frombuffer(data, np.uint8)
