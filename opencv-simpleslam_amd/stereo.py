"""Semi-global stereo matching on the HIP backend: `cv2.StereoSGBM_create(...).compute` and the prototype's keypoint lift.

Stands in for the stereo leg of the reference's prototype (refrences/sfm_lightglue_aliked.py:109-121, :357-396):

    stereo = cv2.StereoSGBM_create(minDisparity=0, numDisparities=32, blockSize=11, P1=8 * 11 * 11, P2=32 * 11 * 11)
    disparity = stereo.compute(gray_left, gray_right).astype(np.float32) / 16.0
    q1_l, q1_r, q2_l, q2_r, in_bounds = calculate_right_features(q1, q2, disparity1, disparity2)
    Q1, Q2 = get_stereo_3d_pts(q1_l, q1_r, q2_l, q2_r)          # cv2.triangulatePoints(Proj, Proj_r, ...)

as `stereo.StereoSGBM_create(...)` with cv2's positional order and the prototype's four function names.  8-bit input, MODE_SGBM
(single pass, five paths), no speckle filter; the arithmetic is all integers, defined stage by stage in tests/stereo_ref.py, which
csrc/stereo_kernels.hip equals bit for bit.  Parity with cv2 itself is unpinned (the restatement's UNCONFIRMED list).

Stated departures: `disp12MaxDiff <= 0` does not disable the left-right check (it runs with 1); `compute` takes 2-D images only
and `compute_stereo_disparity` converts colour to grey first, which is the prototype's call order and NOT cv2's per-channel cost;
a keypoint outside the image is unmasked where the prototype would raise or wrap.

Not built: MODE_HH, MODE_SGBM_3WAY, MODE_HH4, the speckle filter, 16-bit input, StereoBM.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3
MAX_SIDE = 16384
MAX_COST = 32767
MAX_WORKSPACE = 4 << 30
STAGES = {"pf_left": 0, "pf_right": 1, "C": 2, "S": 3, "raw": 4, "right": 5, "checked": 6}
_MODE_NAMES = {MODE_HH: "MODE_HH", MODE_SGBM_3WAY: "MODE_SGBM_3WAY", MODE_HH4: "MODE_HH4"}


def normalise(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio):
    """The parameters the kernels run with (stereo_plan.hpp: sgbm_normalise)."""
    P1e = P1 if P1 > 0 else 2
    return dict(minD=minDisparity, D=numDisparities, bs=blockSize, P1=P1e, P2=max(P2 if P2 > 0 else 5, P1e + 1),
                d12=disp12MaxDiff if disp12MaxDiff > 0 else 1, uniq=uniquenessRatio if uniquenessRatio >= 0 else 10,
                ftzero=max(preFilterCap, 15) | 1, maxD=minDisparity + numDisparities, invalid=(minDisparity - 1) * 16)


def _piece(nbytes):
    return (nbytes + 8 + 255) // 256 * 256


def workspace_bytes(max_w, max_h, maxD, D):
    """Bytes of device memory one instance owns (stereo_plan.hpp: sgbm_extents): staging, grey and prefiltered planes, three int16
    volumes [max_h][max_w - maxD][D] (row sums, C, S), the selection's key and four int16 images."""
    px, cols = max_w * max_h, max(max_w - maxD, 0)
    return (2 * _piece(px * 4) + 4 * _piece(px) + 3 * _piece(max_h * cols * D * 2) + _piece(max_h * cols * 4) + 4 * _piece(px * 2))


def _check_params(args):
    minD, D, bs, P1, P2, d12, cap, uniq, spw, spr, mode = args
    if mode != MODE_SGBM:
        raise NotImplementedError(f"mode {mode} ({_MODE_NAMES.get(mode, 'unknown')}) is not built (only MODE_SGBM = 0)")
    if spw > 0:
        raise NotImplementedError(f"speckleWindowSize {spw}: the speckle filter is not built (want 0)")
    if minD < 0:
        raise ValueError(f"minDisparity {minD} < 0")
    if D < 16 or D > 256 or D % 16:
        raise ValueError(f"numDisparities {D} is not a multiple of 16 in 16..256")
    if bs < 1 or bs > 11 or bs % 2 == 0:
        raise ValueError(f"blockSize {bs} is not odd in 1..11")
    if cap < 0 or cap > 63:
        raise ValueError(f"preFilterCap {cap} outside 0..63")
    if uniq > 100:
        raise ValueError(f"uniquenessRatio {uniq} > 100")
    p = normalise(minD, D, bs, P1, P2, d12, cap, uniq)
    per_pixel = ((2 * p["ftzero"]) >> 2) + (255 >> 2)
    if bs * bs * per_pixel + p["P2"] > MAX_COST:
        raise ValueError(f"P2 {p['P2']} with blockSize {bs}: the largest block cost {bs * bs * per_pixel} (= {bs}^2 x {per_pixel} per pixel) "
                         f"+ P2 exceeds {MAX_COST}")
    return p


def _check_size(w, h, p):
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError(f"image size {w}x{h} outside 1..{MAX_SIDE}")
    ws = workspace_bytes(w, h, p["maxD"], p["D"])
    if ws > MAX_WORKSPACE:
        raise ValueError(f"workspace of {ws} bytes exceeds {MAX_WORKSPACE}")


def _check_grey_pair(left, right):
    for name, img in (("left", left), ("right", right)):
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8:
            raise TypeError(f"{name}: expected a uint8 image (cv2.imread output)")
        if img.ndim == 3:
            raise ValueError(f"{name}: compute takes 2-D uint8 images, got shape {img.shape}; compute_stereo_disparity(img_l, img_r, stereo) "
                             "converts colour to grey first, as the prototype does")
        if img.ndim != 2:
            raise ValueError(f"{name}: unsupported image shape {img.shape}")
    if left.shape != right.shape:
        raise ValueError(f"left {left.shape} and right {right.shape} differ in size")


class _Instance:
    """One parameter set on the device for images up to max_wh = (W, H)."""

    def __init__(self, max_wh, args, ctx=None):
        self.handle = None
        self.params = _check_params(args)
        self.max_wh = (int(max_wh[0]), int(max_wh[1]))
        _check_size(*self.max_wh, self.params)
        self.ctx = ctx or _native.default_context()
        h = C.c_void_p()
        _native.check(_native.lib().sslam_sgbm_create(self.ctx.handle, *self.max_wh, *args, C.byref(h)), "sslam_sgbm_create")
        self.handle = h
        self._last = None

    def close(self):
        if getattr(self, "handle", None):
            _native.lib().sslam_sgbm_destroy(self.handle)            # (drains the stream)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if self.handle is None:
            raise ValueError("the instance was closed (the cache keeps the four most recent (context, size, parameters)): compute again")
        return self.handle

    def _check_fit(self, H, W):
        if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
            raise ValueError(f"image size {W}x{H} outside 1..{MAX_SIDE}")
        if W > self.max_wh[0] or H > self.max_wh[1]:
            raise ValueError(f"image {W}x{H} is larger than the instance's {self.max_wh[0]}x{self.max_wh[1]}")

    def compute(self, left, right, channels=1):
        H, W = left.shape[:2]
        self._check_fit(H, W)
        out = np.empty((H, W), np.int16)
        left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)      # (a view's copy must live across the call)
        P = _native.ptr
        _native.check(_native.lib().sslam_sgbm_compute_host(self._live(), P(left), P(right), H, W, channels, P(out)), "sslam_sgbm_compute_host")
        self._last = (H, W)
        return out

    def compute_dev(self, left_dev, right_dev, H, W, channels, disp_dev):
        if channels not in (1, 3, 4):
            raise ValueError(f"{channels} channels (want 1, 3 or 4)")
        self._check_fit(int(H), int(W))
        P = _native.ptr
        _native.check(_native.lib().sslam_sgbm_compute_dev(self._live(), P(int(left_dev)), P(int(right_dev)), int(H), int(W), int(channels),
                                                           P(int(disp_dev))), "sslam_sgbm_compute_dev")
        self._last = (int(H), int(W))

    def stage_read(self, which):
        k = STAGES[which] if isinstance(which, str) else int(which)
        if self._last is None:
            raise ValueError("no compute yet")
        H, W = self._last
        W1 = max(W - self.params["maxD"], 0)
        out = (np.empty((H, W), np.uint8) if k < 2 else np.empty((H, W1, self.params["D"]), np.int16) if k < 4 else np.empty((H, W), np.int16))
        _native.check(_native.lib().sslam_sgbm_stage_read(self._live(), k, _native.ptr(out)), "sslam_sgbm_stage_read")
        return out


_instances = {}              # (id(ctx), W, H, the eleven parameters) -> (ctx, _Instance), most recent last
_INSTANCES_KEEP = 4


def cached(wh, args, ctx=None):
    """The instance kept for (context, size, parameters): made on first use, the least recently used of more than four closed.
    The key holds the exact (W, H): a stream of frames of one size keeps one instance, a stream of ever-changing sizes frees and
    allocates a slab (about 100 MB at 1241 x 376, D = 32) per new size - make one `_Instance` of the largest size for that.  A
    `StereoSGBM` whose last instance was evicted says so (ValueError) when its `stage_read` is called."""
    ctx = ctx or _native.default_context()
    key = (id(ctx), int(wh[0]), int(wh[1]), *args)
    entry = _instances.get(key)
    if entry is not None and entry[0] is ctx and entry[1].handle is not None:
        _instances[key] = _instances.pop(key)
        return entry[1]
    if entry is not None:
        _instances.pop(key)[1].close()
    inst = _Instance(wh, args, ctx)
    _instances[key] = (ctx, inst)
    while len(_instances) > _INSTANCES_KEEP:
        _instances.pop(next(iter(_instances)))[1].close()
    return inst


class StereoSGBM:
    """What `cv2.StereoSGBM_create` returns: `.compute(left, right)` -> int16 [H, W] in sixteenths of a pixel."""

    def __init__(self, args, ctx=None):
        self.args = tuple(int(v) for v in args)
        self.params = _check_params(self.args)
        self.ctx = ctx
        self._last = None

    def compute(self, left, right):
        _check_grey_pair(left, right)
        H, W = left.shape
        _check_size(W, H, self.params)
        self._last = cached((W, H), self.args, self.ctx)
        return self._last.compute(left, right, 1)

    def compute_dev(self, left_dev, right_dev, H, W, disp_dev, channels=1):
        """Enqueue only: uint8 [H][W][channels] device images -> int16 [H][W] at disp_dev."""
        _check_size(int(W), int(H), self.params)
        self._last = cached((int(W), int(H)), self.args, self.ctx)
        self._last.compute_dev(left_dev, right_dev, H, W, channels, disp_dev)

    def stage_read(self, which):
        """For tests, of the last compute: 'pf_left' | 'pf_right' | 'C' | 'S' | 'raw' | 'right' | 'checked'."""
        if self._last is None:
            raise ValueError("no compute yet")
        return self._last.stage_read(which)


def StereoSGBM_create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                      speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM, ctx=None):
    """`cv2.StereoSGBM_create` with cv2's positional order.  Refusals (ValueError / NotImplementedError) come before the library is
    touched; the device instance is made at the first compute, per image size."""
    return StereoSGBM((minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio, speckleWindowSize,
                       speckleRange, mode), ctx)


def _grey_pair_channels(img_l, img_r):
    for name, img in (("img_l", img_l), ("img_r", img_r)):
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8:
            raise TypeError(f"{name}: expected a uint8 image (cv2.imread output)")
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (1, 3, 4)):
            raise ValueError(f"{name}: unsupported image shape {img.shape}")
    if img_l.shape != img_r.shape:
        raise ValueError(f"left {img_l.shape} and right {img_r.shape} differ in size")
    return 1 if img_l.ndim == 2 else img_l.shape[2]


def compute_stereo_disparity(img_l, img_r, stereo):
    """The prototype's `compute_stereo_disparity`: grey of both images (on the device, BGR2GRAY), compute, `/ 16` in float32."""
    c = _grey_pair_channels(img_l, img_r)
    H, W = img_l.shape[:2]
    _check_size(W, H, stereo.params)
    stereo._last = cached((W, H), stereo.args, stereo.ctx)
    return stereo._last.compute(img_l, img_r, c).astype(np.float32) / np.float32(16.0)


def _to_sixteenths(disp):
    """float32 disparity of compute_stereo_disparity (or the int16 image itself) -> int16 sixteenths, exact"""
    disp = np.asarray(disp)
    if disp.ndim != 2:
        raise ValueError(f"disparity of shape {disp.shape} (want [H, W])")
    if disp.dtype == np.int16:
        return np.ascontiguousarray(disp)
    return np.ascontiguousarray(np.rint(disp.astype(np.float32) * np.float32(16.0)).astype(np.int16))


def _lift(q, disp, q_right, P_left, P_right, min_disp, max_disp, ctx, want_X):
    q = np.ascontiguousarray(np.asarray(q, np.float32).reshape(-1, 2))
    n = len(q)
    d, xr, mask = np.empty(n, np.float32), np.empty((n, 2), np.float32), np.zeros(n, np.uint8)
    X = np.empty((n, 3), np.float64) if want_X else None
    if n == 0:
        return d, mask.astype(bool), xr, X
    ctx = ctx or _native.default_context()
    P = _native.ptr
    if q_right is not None:
        q_right = np.ascontiguousarray(np.asarray(q_right, np.float32).reshape(-1, 2))
        if len(q_right) != n:
            raise ValueError(f"{n} left and {len(q_right)} right points")
        disp16, H, W = None, 0, 0
    else:
        disp16 = _to_sixteenths(disp)
        H, W = disp16.shape
    Pl = None if P_left is None else np.ascontiguousarray(np.asarray(P_left, np.float64).reshape(12))
    Pr = None if P_right is None else np.ascontiguousarray(np.asarray(P_right, np.float64).reshape(12))
    _native.check(_native.lib().sslam_stereo_lift_host(ctx.handle, n, P(q), P(q_right), P(disp16), H, W, P(Pl), P(Pr), float(min_disp),
                                                       float(max_disp), P(d), P(xr), P(X), P(mask)), "sslam_stereo_lift_host")
    return d, mask.astype(bool), xr, X


def lift(q, disp, Proj, Proj_r, min_disp=0.0, max_disp=100.0, ctx=None):
    """Keypoints through a disparity image to 3-D in one call: -> (d float32 [n], mask bool [n], xy_right float32 [n, 2], X float64
    [n, 3], NaN where the mask is clear).  `disp` is a compute's int16 image or its float32 `/ 16` form."""
    return _lift(q, disp, None, Proj, Proj_r, min_disp, max_disp, ctx, True)


def lift_dev(ctx, n_max, n_dev, xy_dev, disp_dev, H, W, Proj, Proj_r, min_disp, max_disp, d_out_dev, xy_right_out_dev, X_out_dev, mask_out_dev):
    """Enqueue only, device pointers; n_dev (0: none) is a device-resident count, nothing is written beyond it."""
    P = _native.ptr
    Pl = np.ascontiguousarray(np.asarray(Proj, np.float64).reshape(12))
    Pr = np.ascontiguousarray(np.asarray(Proj_r, np.float64).reshape(12))
    opt = lambda a: P(int(a)) if a else None
    _native.check(_native.lib().sslam_stereo_lift_dev(ctx.handle, int(n_max), opt(n_dev), P(int(xy_dev)), None, P(int(disp_dev)), int(H), int(W),
                                                      P(Pl), P(Pr), float(min_disp), float(max_disp), opt(d_out_dev), opt(xy_right_out_dev),
                                                      opt(X_out_dev), P(int(mask_out_dev))), "sslam_stereo_lift_dev")


def apply_disparity_check(q, disp, min_disp, max_disp):
    """The prototype's `apply_disparity_check`: -> (disp_vals, mask) of `disp[int(y), int(x)]` per keypoint, numpy on the host (the
    device form of the same lookup is the lift entry, which `calculate_right_features` runs on)."""
    q_idx = np.asarray(q).astype(int)
    disp_vals = disp.T[q_idx[:, 0], q_idx[:, 1]]
    mask = (disp_vals > min_disp) & (disp_vals < max_disp)
    return disp_vals, mask


def calculate_right_features(q1, q2, disparity1, disparity2, min_disp=0.0, max_disp=100.0, ctx=None):
    """The prototype's `calculate_right_features` -> (q1_l, q1_r, q2_l, q2_r, in_bounds), the lookups on the lift entry."""
    q1, q2 = np.asarray(q1), np.asarray(q2)
    _, m1, r1, _ = _lift(q1, disparity1, None, None, None, min_disp, max_disp, ctx, False)
    _, m2, r2, _ = _lift(q2, disparity2, None, None, None, min_disp, max_disp, ctx, False)
    in_bounds = m1 & m2
    return q1[in_bounds], r1[in_bounds].astype(q1.dtype), q2[in_bounds], r2[in_bounds].astype(q2.dtype), in_bounds


def get_stereo_3d_pts(q1_l, q1_r, q2_l, q2_r, Proj, Proj_r, ctx=None):
    """The prototype's `get_stereo_3d_pts` -> (Q1_3d, Q2_3d) float64 [n, 3]: `cv2.triangulatePoints(Proj, Proj_r, ...)` and the
    division by w, on the lift entry with the right pixels given (NaN where |w| <= 1e-12)."""
    Q1 = _lift(q1_l, None, q1_r, Proj, Proj_r, 0.0, 0.0, ctx, True)[3]
    Q2 = _lift(q2_l, None, q2_r, Proj, Proj_r, 0.0, 0.0, ctx, True)[3]
    return Q1, Q2
