"""Numpy restatement of `cv2.calcOpticalFlowPyrLK` for 8-bit images (OpenCV's lkpyramid.cpp, LKTrackerInvoker), of the grey
conversion in front of it and of the forward-backward gate of the reference's KLT front end (slam/monocular/main4.py:402-433).

PARITY UNPINNED: cv2 is absent here, so nothing below was compared with it.  Written from memory of OpenCV 4.x and not confirmed:
  * the grey conversion's coefficient set: 15-bit (B 3735, G 19235, R 9798, + 2^14, >> 15: recent 4.x) is the default here, the
    14-bit set (1868, 9617, 4899, + 2^13, >> 14) is `bits=14`; frames with three equal planes (KITTI) give that plane either way;
  * `pyrDown`'s 8-bit path as separable [1 4 6 4 1] with one rounding (sum + 128) >> 8, and the stop rule of
    `buildOpticalFlowPyramid` (a level whose width <= winSize.width or height <= winSize.height is not built);
  * the Scharr pair unscaled in int16, reflect-101 at the image edge, and the derivative buffer's border of zeros;
  * the order of the bounds tests, the places where status / err are written, the two exits of the iteration;
  * the ORDER of OpenCV's float accumulations (it adds the integer products into float32 one by one, or eight at a time in its
    SIMD paths, which differ from each other); see "defined arithmetic";
  * what `err` holds where OpenCV never writes it (status cleared by the min-eigenvalue test or in mid-iteration): cv2 leaves the
    buffer as allocated; here it is 0;
  * that a point up to winSize outside the image passes the bounds test and may track on the reflected border (status 1): only
    beyond that margin, or not finite, is it answered with status 0 and err 0;
  * `criteria`: without the COUNT bit 30 iterations, without the EPS bit epsilon 0.01, as OpenCV sets them.

DEFINED ARITHMETIC (where this deliberately differs from cv2's bits, by no more than cv2's own builds differ from each other).
Every sum over the window is a sum of exact integers: it is taken exactly in int64 and converted to float32 once, round to
nearest (through float64, which holds it exactly: sums stay below 2^53).  Every float operation after that is one IEEE
float32 operation in the written order, no fused multiply-add; `sqrt` and the divisions are correctly rounded.  As in OpenCV,
`delta . delta` is a float64 sum of float64 products compared with the float64 epsilon^2, and |delta + prevDelta| and minEig
are compared with the float64 constants 0.01 and minEigThreshold.  A coordinate that is not finite, or outside int range,
takes the out-of-image branch (OpenCV's cvFloor of it is undefined).  The kernel performs the same operations one for one,
so the GPU tests compare bits.
"""
import numpy as np

OPTFLOW_USE_INITIAL_FLOW = 4
OPTFLOW_LK_GET_MIN_EIGENVALS = 8
TERM_COUNT, TERM_EPS = 1, 2
W_BITS = 14
FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(1.1920929e-07)
F = np.float32

# exit reasons of a point at one level (klt_scenes counts them at level 0)
EXIT_NONE, EXIT_OUTSIDE, EXIT_MIN_EIG, EXIT_EPS, EXIT_OSCILLATION, EXIT_BUDGET, EXIT_LEFT_IMAGE = range(7)


def bgr_to_gray(img, bits=15):
    """cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) for uint8 [H,W,3|4] (fixed point, rounding constant included); [H,W] passes."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    cb, cg, cr = {15: (3735, 19235, 9798), 14: (1868, 9617, 4899)}[bits]
    v = img.astype(np.int32)
    return ((v[..., 0] * cb + v[..., 1] * cg + v[..., 2] * cr + (1 << (bits - 1))) >> bits).astype(np.uint8)


def reflect101(i, n):
    """BORDER_REFLECT_101 index of i (any integer array) into 0..n-1; a length of 1 gives 0."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def pyr_down(img):
    """cv2.pyrDown of uint8 [H,W] -> [(H+1)//2, (W+1)//2]."""
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int32)
    v = img.astype(np.int32)
    cols = reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)          # [ow, 5]
    rows = reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)          # [oh, 5]
    hx = (v[:, cols] * k).sum(-1)                                                          # [h, ow]
    s = (hx[rows, :] * k[None, :, None]).sum(1)                                            # [oh, ow]
    return ((s + 128) >> 8).astype(np.uint8)


def scharr(img):
    """(dx, dy) int16 [H,W]: dx = [3 10 3] down the rows x [-1 0 1] along the row, dy its transpose; reflect-101 at the edge."""
    h, w = img.shape
    v = img.astype(np.int32)
    r = reflect101(np.arange(-1, h + 1), h)
    c = reflect101(np.arange(-1, w + 1), w)
    p = v[r][:, c]                                                                         # [h+2, w+2]
    sm_r = 3 * p[:-2] + 10 * p[1:-1] + 3 * p[2:]                                           # smoothed down the rows [h, w+2]
    sm_c = 3 * p[:, :-2] + 10 * p[:, 1:-1] + 3 * p[:, 2:]                                  # smoothed along the row [h+2, w]
    dx = sm_r[:, 2:] - sm_r[:, :-2]
    dy = sm_c[2:] - sm_c[:-2]
    return dx.astype(np.int16), dy.astype(np.int16)


def level_sizes(h, w, win, max_level):
    """[(h, w)] of the levels buildOpticalFlowPyramid builds; win = (width, height)."""
    out = [(h, w)]
    for _ in range(max_level):
        h, w = (h + 1) // 2, (w + 1) // 2
        if w <= win[0] or h <= win[1]:
            break
        out.append((h, w))
    return out


class Pyramid:
    """grey, levels[l] uint8, dx[l] / dy[l] int16, and the padded forms the tracker reads: levels by winSize with
    reflect-101, derivatives by winSize with zeros."""

    def __init__(self, img, win=(21, 21), max_level=3, bits=15):
        self.win = (int(win[0]), int(win[1]))
        self.gray = bgr_to_gray(img, bits)
        self.levels = [np.ascontiguousarray(self.gray)]
        for h, w in level_sizes(*self.gray.shape, self.win, max_level)[1:]:
            self.levels.append(pyr_down(self.levels[-1]))
            assert self.levels[-1].shape == (h, w)
        self.dx, self.dy, self.pad_img, self.pad_dx, self.pad_dy = [], [], [], [], []
        pw, ph = self.win
        for lv in self.levels:
            dx, dy = scharr(lv)
            self.dx.append(dx); self.dy.append(dy)
            h, w = lv.shape
            r = reflect101(np.arange(-ph, h + ph), h)
            c = reflect101(np.arange(-pw, w + pw), w)
            self.pad_img.append(lv[r][:, c].astype(np.int32))
            self.pad_dx.append(np.pad(dx.astype(np.int32), ((ph, ph), (pw, pw))))
            self.pad_dy.append(np.pad(dy.astype(np.int32), ((ph, ph), (pw, pw))))

    @property
    def max_level(self):
        return len(self.levels) - 1


def criteria_values(criteria):
    """(maxCount, epsilon^2 float64) as calcOpticalFlowPyrLK derives them from (type, maxCount, epsilon)."""
    typ, count, eps = int(criteria[0]), int(criteria[1]), float(criteria[2])
    count = min(max(count, 0), 100) if typ & TERM_COUNT else 30
    eps = min(max(eps, 0.0), 10.0) if typ & TERM_EPS else 0.01
    return count, eps * eps


def _i64_to_f32(s):
    return s.astype(np.float64).astype(np.float32)


def _inside(fx, fy, w, h, win):
    """The bounds test on floor(p): not (< -win or >= size); non-finite is outside."""
    with np.errstate(invalid="ignore"):
        return (fx >= F(-win[0])) & (fx < F(w)) & (fy >= F(-win[1])) & (fy < F(h))


def _weights(fx, fy):
    """integer origin and the four 2^14 weights of positions (fx, fy) float32 [n] that passed `_inside`."""
    flx, fly = np.floor(fx), np.floor(fy)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    a, b = fx - flx, fy - fly                                          # float32
    one, sc = F(1), F(1 << W_BITS)
    w00 = np.rint((one - a) * (one - b) * sc).astype(np.int64)
    w01 = np.rint(a * (one - b) * sc).astype(np.int64)
    w10 = np.rint((one - a) * b * sc).astype(np.int64)
    w11 = (1 << W_BITS) - w00 - w01 - w10
    return ix, iy, (w00, w01, w10, w11)


def _sample(pad, ix, iy, wts, win, shift):
    """CV_DESCALE(sum of four weighted neighbours, shift) on the window at integer origin (ix, iy) [n] -> int64 [n, wh, ww].
    `pad` is padded by win: the load touches ix .. ix + win inclusive, inside it for every ix in [-win, size - 1]."""
    ww, wh = win
    r = (iy + wh)[:, None, None] + np.arange(wh)[None, :, None]
    c = (ix + ww)[:, None, None] + np.arange(ww)[None, None, :]
    w00, w01, w10, w11 = (w[:, None, None] for w in wts)
    v = pad[r, c] * w00 + pad[r, c + 1] * w01 + pad[r + 1, c] * w10 + pad[r + 1, c + 1] * w11
    return (v + (1 << (shift - 1))) >> shift


def calc_optical_flow_pyr_lk(prev, nxt, prev_pts, next_pts=None, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01), flags=0,
                             minEigThreshold=1e-4, return_exits=False):
    """prev / nxt: uint8 images or `Pyramid`s of one size; prev_pts [N,2] or [N,1,2] float32
    -> (next_pts [N,1,2] float32, status [N,1] uint8, err [N,1] float32), and with return_exits the level-0 exit reason [N]."""
    win = (int(winSize[0]), int(winSize[1]))
    P = prev if isinstance(prev, Pyramid) else Pyramid(prev, win, maxLevel)
    Q = nxt if isinstance(nxt, Pyramid) else Pyramid(nxt, win, maxLevel)
    assert P.win == win and Q.win == win and P.gray.shape == Q.gray.shape
    top = min(P.max_level, Q.max_level, int(maxLevel))
    max_count, eps2 = criteria_values(criteria)
    min_eig_thr = float(minEigThreshold)
    ww, wh = win
    pts = np.asarray(prev_pts, np.float32).reshape(-1, 2)
    n = len(pts)
    half = np.array([(ww - 1) * 0.5, (wh - 1) * 0.5], np.float32)
    out = np.zeros((n, 2), np.float32)
    if flags & OPTFLOW_USE_INITIAL_FLOW:
        guess = np.asarray(next_pts, np.float32).reshape(-1, 2)
        assert guess.shape == pts.shape
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)
    exits = np.zeros(n, np.int32)
    den_eig = F(2 * ww * wh)
    den_err = F(32 * ww * wh)
    for level in range(top, -1, -1):
        h, w = P.levels[level].shape
        scale = F(1.0 / (1 << level))
        prev_l = pts * scale
        if level == top:
            out = (guess * scale) if flags & OPTFLOW_USE_INITIAL_FLOW else prev_l.copy()
        else:
            out = out * F(2)
        pf = prev_l - half
        ok = _inside(pf[:, 0], pf[:, 1], w, h, win)
        if level == 0:
            status[~ok] = 0; err[~ok] = 0; exits[~ok] = EXIT_OUTSIDE
        idx = np.nonzero(ok)[0]
        if not len(idx):
            continue
        ix, iy, wts = _weights(pf[idx, 0], pf[idx, 1])
        Ipat = _sample(P.pad_img[level], ix, iy, wts, win, W_BITS - 5)
        Ix = _sample(P.pad_dx[level], ix, iy, wts, win, W_BITS)
        Iy = _sample(P.pad_dy[level], ix, iy, wts, win, W_BITS)
        A11 = _i64_to_f32((Ix * Ix).sum((1, 2))) * FLT_SCALE
        A12 = _i64_to_f32((Ix * Iy).sum((1, 2))) * FLT_SCALE
        A22 = _i64_to_f32((Iy * Iy).sum((1, 2))) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        dif = A11 - A22
        root = np.sqrt(dif * dif + F(4) * A12 * A12)
        min_eig = (A22 + A11 - root) / den_eig
        if flags & OPTFLOW_LK_GET_MIN_EIGENVALS:
            err[idx] = min_eig
        rej = (min_eig.astype(np.float64) < min_eig_thr) | (D < FLT_EPSILON)
        if level == 0:
            status[idx[rej]] = 0; exits[idx[rej]] = EXIT_MIN_EIG
        keep = ~rej
        idx, Ipat, Ix, Iy, A11, A12, A22 = idx[keep], Ipat[keep], Ix[keep], Iy[keep], A11[keep], A12[keep], A22[keep]
        Dinv = F(1) / D[keep]
        cur = out[idx] - half                                          # nextPt, window-corner form
        prev_delta = np.zeros((len(idx), 2), np.float32)
        live = np.ones(len(idx), bool)                                 # still iterating
        if level == 0:
            exits[idx] = EXIT_BUDGET
        for j in range(max_count):
            li = np.nonzero(live)[0]
            if not len(li):
                break
            ins = _inside(cur[li, 0], cur[li, 1], w, h, win)
            gone = li[~ins]
            live[gone] = False
            if level == 0:
                status[idx[gone]] = 0; exits[idx[gone]] = EXIT_LEFT_IMAGE
            li = li[ins]
            if not len(li):
                break
            jx, jy, wts = _weights(cur[li, 0], cur[li, 1])
            diff = _sample(Q.pad_img[level], jx, jy, wts, win, W_BITS - 5) - Ipat[li]
            b1 = _i64_to_f32((diff * Ix[li]).sum((1, 2))) * FLT_SCALE
            b2 = _i64_to_f32((diff * Iy[li]).sum((1, 2))) * FLT_SCALE
            delta = np.stack([(A12[li] * b2 - A22[li] * b1) * Dinv[li], (A12[li] * b1 - A11[li] * b2) * Dinv[li]], 1)
            cur[li] = cur[li] + delta
            out[idx[li]] = cur[li] + half
            d64 = delta.astype(np.float64)
            small = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1] <= eps2
            osc = np.zeros(len(li), bool)
            if j > 0:
                s = np.abs(delta + prev_delta[li]).astype(np.float64)
                osc = ~small & (s[:, 0] < 0.01) & (s[:, 1] < 0.01)
                o = li[osc]
                out[idx[o]] = out[idx[o]] - delta[osc] * F(0.5)
            live[li[small | osc]] = False
            if level == 0:
                exits[idx[li[small]]] = EXIT_EPS; exits[idx[li[osc]]] = EXIT_OSCILLATION
            prev_delta[li] = delta
        if level == 0 and not flags & OPTFLOW_LK_GET_MIN_EIGENVALS:
            k = np.nonzero(status[idx] == 1)[0]
            fin = out[idx[k]] - half
            ins = _inside(fin[:, 0], fin[:, 1], w, h, win)
            status[idx[k[~ins]]] = 0
            k, fin = k[ins], fin[ins]
            if len(k):
                jx, jy, wts = _weights(fin[:, 0], fin[:, 1])
                diff = _sample(Q.pad_img[level], jx, jy, wts, win, W_BITS - 5) - Ipat[k]
                err[idx[k]] = _i64_to_f32(np.abs(diff).sum((1, 2))) / den_err
    res = (out.reshape(n, 1, 2).astype(np.float32), status.reshape(n, 1), err.reshape(n, 1))
    return res + (exits,) if return_exits else res


def track_forward_backward(prev, nxt, prev_pts, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 1e-3), minEigThreshold=1e-4,
                           err_thresh=12.0, fb_thresh=1.5):
    """The body of the reference's KLT front end (main4.py:402-433) with its two cv2 calls replaced by the restatement
    -> (pts0 [K,2], pts1 [K,2], (raw, st1, err_ok, fb_ok, kept)).  The thresholds compare in float32, as numpy compares a
    float32 array with a Python float."""
    kw = dict(winSize=winSize, maxLevel=maxLevel, criteria=criteria, minEigThreshold=minEigThreshold)
    prev_pts = np.asarray(prev_pts, np.float32).reshape(-1, 1, 2)
    raw_count = prev_pts.shape[0]
    pts0 = np.empty((0, 2), np.float32); pts1 = np.empty((0, 2), np.float32)
    next_pts, st, err = calc_optical_flow_pyr_lk(prev, nxt, prev_pts, None, **kw)
    status_mask = st.reshape(-1) == 1
    status_count = int(status_mask.sum())
    good = status_mask.copy()
    err_mask = err.reshape(-1) < F(err_thresh)
    good &= err_mask
    err_count = int((status_mask & err_mask).sum())
    fb_count = err_count
    if good.any():
        back_pts, st_back, _ = calc_optical_flow_pyr_lk(nxt, prev, next_pts, None, **kw)
        st_back_mask = st_back.reshape(-1) == 1
        with np.errstate(invalid="ignore", over="ignore"):
            fb_err = np.linalg.norm(back_pts - prev_pts, axis=2).reshape(-1)
            fb_mask = st_back_mask & (fb_err < F(fb_thresh))
        good &= fb_mask
        fb_count = int((status_mask & err_mask & fb_mask).sum())
    if good.any():
        pts0 = prev_pts[good].reshape(-1, 2)
        pts1 = next_pts[good].reshape(-1, 2)
    return pts0, pts1, (raw_count, status_count, err_count, fb_count, len(pts0))
