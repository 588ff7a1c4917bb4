"""numpy restatement of the four OpenCV functions behind lens undistortion (test infrastructure; never imported by the product):

    get_optimal_new_camera_matrix   cv2.getOptimalNewCameraMatrix(K, D, size, alpha, newImgSize), centerPrincipalPoint=False
    init_undistort_rectify_map      cv2.initUndistortRectifyMap(K, D, R, newK, size, CV_32FC1), two variants (below)
    convert_maps                    cv2.convertMaps(mapx, mapy, CV_16SC2): int16 pixel + 5-bit fractions
    remap_linear                    cv2.remap(img, ixy, alpha, INTER_LINEAR), BORDER_CONSTANT value 0, on that fixed-point form

PARITY WITH cv2 IS UNPINNED: cv2 is not installed where this was written, and everything below was restated from memory of
OpenCV 4.x's calib3d / imgproc sources.  What could not be confirmed:

  * the 9 x 9 grid of `icvGetRectangles`: taken as x * (width - 1) / (N - 1) (older versions: x * width / (N - 1)), evaluated
    in float32 - exact for every size up to 16384, so float32 against double makes no difference THERE; the points and the
    rectangles themselves are taken as doubles (CV_64FC2, Rect_<double>, as remembered of 4.5 and later; before that they were
    float32, which moves new_K in its 7th digit - `undistort_grid(round_f32=True)` shows that form);
  * `undistortPoints`' inverse of the model: FIVE fixed-point iterations, no convergence test (the default criteria), a point
    whose inverse radial factor turns negative keeps its starting value;
  * the viewport scale (newW - 1) / inner.width (older versions: newW / inner.width);
  * the ROI's rounding: ceil of the inner rectangle's corner, floor of its size, then the intersection with the new image
    (older versions round the double rectangle to the nearest integers);
  * `initUndistortRectifyMap` has a SIMD row path in OpenCV (AVX2, four pixels at a time) whose operation order may differ
    from the scalar loop restated here; the scalar loop multiplies by the reciprocal 1 / w (variant `rowsum`);
  * `remap`'s weight table: OpenCV builds the bilinear weights as int16 with a scale of 32768 and saturates the single entry
    that equals 32768 (fx = fy = 0) to 32767; whether its pass that makes every table row sum to 32768 again restores that
    entry was not confirmed.  The weights here are exact, (32 - fx)(32 - fy) 32 ... fx fy 32 with sum 2^15, so an identity map
    reproduces the image exactly (tests/test_undistort_ref.py asserts it); a saturated entry of 32767 would give
    (S * 32767 + 16384) >> 15, which is S as well for every uint8 S - the two tables are indistinguishable at 8 bits there.

`init_undistort_rectify_map` variants: `rowsum` walks each row by repeated addition (_x += ir[0]) as OpenCV's scalar loop does
and multiplies by 1 / w; `direct` evaluates u ir[0] + (v ir[1] + ir[2]) and divides - the order of the kernel, operation for
operation (the kernel is compiled without fused multiply-adds, and OpenCV inverts newK R by LU where both variants here use
the library's cofactors).  The tests measure how often the two variants round to different float32 values.
"""
import numpy as np

GRID = 9
INVERSE_ITERS = 5


def k8(D):
    k = np.zeros(8)
    d = np.zeros(0) if D is None else np.asarray(D, np.float64).reshape(-1)
    assert d.size in (0, 4, 5, 8), d.size
    k[:d.size] = d
    return k


def distort_normalised(x, y, k):
    """OpenCV's forward model on normalised coordinates -> (xd, yd)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    xy2 = 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    return x * kr + p1 * xy2 + p2 * (r2 + 2 * x2), y * kr + p1 * (r2 + 2 * y2) + p2 * xy2


def undistort_normalised(x0, y0, k, iters=INVERSE_ITERS):
    """undistortPoints' fixed-count iterative inverse on normalised coordinates (fp64)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    x, y = x0.copy(), y0.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        neg = icdist < 0
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = np.where(neg, x0, (x0 - dx) * icdist)
        y = np.where(neg, y0, (y0 - dy) * icdist)
    return x, y


def grid_points(W, H):
    """the 9 x 9 grid of image points, float32 arithmetic -> (u, v) float64 [81]"""
    j = np.arange(GRID, dtype=np.float32)
    gx = j * np.float32(W - 1) / np.float32(GRID - 1)
    gy = j * np.float32(H - 1) / np.float32(GRID - 1)
    return np.tile(gx, GRID).astype(np.float64), np.repeat(gy, GRID).astype(np.float64)


def undistort_grid(K, k, W, H, P=None, round_f32=False):
    u, v = grid_points(W, H)
    x, y = undistort_normalised((u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], k)
    if P is not None:
        x = x * P[0, 0] + P[0, 2]
        y = y * P[1, 1] + P[1, 2]
    p = np.stack([x, y], 1)
    return p.astype(np.float32).astype(np.float64) if round_f32 else p


def rectangles(K, k, W, H, P=None):
    """(inner, outer), each (x, y, w, h): the largest rectangle inside the undistorted border / the grid's bounding box"""
    p = undistort_grid(K, k, W, H, P).reshape(GRID, GRID, 2)
    ix0, ix1 = p[:, 0, 0].max(), p[:, -1, 0].min()
    iy0, iy1 = p[0, :, 1].max(), p[-1, :, 1].min()
    ox0, ox1, oy0, oy1 = p[..., 0].min(), p[..., 0].max(), p[..., 1].min(), p[..., 1].max()
    return (ix0, iy0, ix1 - ix0, iy1 - iy0), (ox0, oy0, ox1 - ox0, oy1 - oy0)


def get_optimal_new_camera_matrix(K, D, size, alpha=0.0, new_size=None):
    K = np.asarray(K, np.float64)
    k = k8(D)
    W, H = size
    nW, nH = new_size if new_size else size
    inner, outer = rectangles(K, k, W, H)
    fx0, fy0 = (nW - 1) / inner[2], (nH - 1) / inner[3]
    cx0, cy0 = -fx0 * inner[0], -fy0 * inner[1]
    fx1, fy1 = (nW - 1) / outer[2], (nH - 1) / outer[3]
    cx1, cy1 = -fx1 * outer[0], -fy1 * outer[1]
    M = np.eye(3)
    M[0, 0] = fx0 * (1 - alpha) + fx1 * alpha
    M[1, 1] = fy0 * (1 - alpha) + fy1 * alpha
    M[0, 2] = cx0 * (1 - alpha) + cx1 * alpha
    M[1, 2] = cy0 * (1 - alpha) + cy1 * alpha
    inner, _ = rectangles(K, k, W, H, M)
    x, y, w, h = int(np.ceil(inner[0])), int(np.ceil(inner[1])), int(np.floor(inner[2])), int(np.floor(inner[3]))
    x1, y1 = min(x + w, nW), min(y + h, nH)
    x, y = max(x, 0), max(y, 0)
    roi = (x, y, x1 - x, y1 - y) if x1 > x and y1 > y else (0, 0, 0, 0)
    return M, roi


def inverse3(A):
    """3 x 3 inverse by cofactors, every product and difference in the order the library's host side writes them (so that
    `direct` and the kernel start from the same nine doubles) -> [9]"""
    m = [float(v) for v in np.asarray(A, np.float64).reshape(9)]
    c0, c1, c2 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = m[0] * c0 + m[1] * c1 + m[2] * c2
    return np.array([c0 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                     c1 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                     c2 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det])


def init_undistort_rectify_map(K, D, R, new_K, size, variant="direct"):
    """-> (mapx, mapy) float32 [H, W]"""
    K = np.asarray(K, np.float64)
    k = k8(D)
    W, H = size
    A = np.asarray(new_K, np.float64)
    if R is not None:
        Rm = np.asarray(R, np.float64)
        A = np.array([[A[r, 0] * Rm[0, c] + A[r, 1] * Rm[1, c] + A[r, 2] * Rm[2, c] for c in range(3)] for r in range(3)])
    ir = inverse3(A)
    u = np.arange(W, dtype=np.float64)[None, :]
    v = np.arange(H, dtype=np.float64)[:, None]
    if variant == "direct":
        X = u * ir[0] + (v * ir[1] + ir[2])
        Y = u * ir[3] + (v * ir[4] + ir[5])
        Wh = u * ir[6] + (v * ir[7] + ir[8])
        x, y = X / Wh, Y / Wh
    elif variant == "rowsum":
        def walk(a, b, c):               # _x = i * b + c at the row's start, then _x += a per pixel: sequential additions
            steps = np.full((H, W), a)
            steps[:, 0] = (v * b + c)[:, 0]
            return np.add.accumulate(steps, axis=1)
        X, Y, Wh = walk(ir[0], ir[1], ir[2]), walk(ir[3], ir[4], ir[5]), walk(ir[6], ir[7], ir[8])
        w = 1.0 / Wh
        x, y = X * w, Y * w
    else:
        raise ValueError(variant)
    xd, yd = distort_normalised(x, y, k)
    mapx = (K[0, 0] * xd + K[0, 2]).astype(np.float32)
    mapy = (K[1, 1] * yd + K[1, 2]).astype(np.float32)
    return mapx, mapy


def _fixed(m):
    with np.errstate(over="ignore", invalid="ignore"):
        t = m.astype(np.float32) * np.float32(32)
        ok = np.abs(t) < np.float32(2147483648.0)            # False for NaN, inf and |t| >= 2^31
    s = np.rint(np.where(ok, t, np.float32(0))).astype(np.int64)      # round half to even
    return s, ok


def convert_maps(mapx, mapy):
    """-> (ixy int16 [H, W, 2], alpha uint16 [H, W] = fy * 32 + fx); a coordinate without a fixed-point form makes the
    record (-32768, -32768, 0)."""
    sx, okx = _fixed(mapx)
    sy, oky = _fixed(mapy)
    ok = okx & oky
    ix = np.where(ok, np.clip(sx >> 5, -32768, 32767), -32768)
    iy = np.where(ok, np.clip(sy >> 5, -32768, 32767), -32768)
    al = np.where(ok, (sy & 31) * 32 + (sx & 31), 0)
    return np.stack([ix, iy], -1).astype(np.int16), al.astype(np.uint16)


def remap_linear(img, ixy, alpha):
    """-> uint8 [H, W(, C)]: integer bilinear blend of the four neighbours, each one outside the source counting as 0"""
    img = np.asarray(img)
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.int64)
    Hs, Ws, _ = src.shape
    ix, iy = ixy[..., 0].astype(np.int64), ixy[..., 1].astype(np.int64)
    fx, fy = (alpha & 31).astype(np.int64), (alpha >> 5).astype(np.int64)

    def sample(x, y):
        inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
        return src[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)] * inside[..., None]

    acc = (sample(ix, iy) * ((32 - fx) * (32 - fy) * 32)[..., None] + sample(ix + 1, iy) * (fx * (32 - fy) * 32)[..., None]
           + sample(ix, iy + 1) * ((32 - fx) * fy * 32)[..., None] + sample(ix + 1, iy + 1) * (fx * fy * 32)[..., None])
    out = ((acc + (1 << 14)) >> 15).astype(np.uint8)
    return out[..., 0] if img.ndim == 2 else out


def neighbour_bound(img, ixy, y, x):
    """The largest byte difference destination pixel (y, x) can show when ONE of its float map entries sits on the other side of
    a float32 step: its fixed-point coordinate then moves by 1 / 32 px along that axis, the samples that can carry weight before
    or after lie in source rows iy - 1 .. iy + 1 and columns ix - 1 .. ix + 1 (one outside the source is the border's 0), and a
    bilinear blend moves by at most (their largest difference) / 32; + 1 for the two roundings.  -> per channel"""
    src = np.asarray(img)
    src = src.reshape(src.shape[0], src.shape[1], -1).astype(np.int64)
    Hs, Ws, _ = src.shape
    ix, iy = int(ixy[y, x, 0]), int(ixy[y, x, 1])
    win = np.zeros((3, 3, src.shape[2]), np.int64)
    for r in range(3):
        for c in range(3):
            yy, xx = iy - 1 + r, ix - 1 + c
            if 0 <= yy < Hs and 0 <= xx < Ws:
                win[r, c] = src[yy, xx]
    return (win.max(axis=(0, 1)) - win.min(axis=(0, 1))) / 32.0 + 1
