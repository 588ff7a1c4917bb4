"""A numpy restatement of the semi-global stereo matcher that csrc/stereo_kernels.hip runs: 8-bit input, MODE_SGBM (single pass,
five paths), no speckle filter, integers only.  Every stage is defined here and the device must equal it bit for bit.

Written from memory of OpenCV 4.x `stereosgbm.cpp` and never compared with `cv2`, so parity with cv2 itself is unpinned and
`UNCONFIRMED` lists what could not be checked.  The stages, for an H x W pair and `D = numDisparities`:

    prefilter   two uint8 planes [H, W]: the clipped horizontal Sobel of the left and of the right image
    C           int16 [H, W - maxD, D]: the block cost of column maxD + xc at disparity minD + d
    S           int16 [H, W - maxD, D]: the five path costs summed, saturated at 32767
    raw         int16 [H, W]: the selected disparity in sixteenths, INVALID where rejected or not computed
    right       int16 [H, W]: the right view's integer disparity, INVALID where no accepted left pixel lands
    checked     int16 [H, W]: raw after the left-right check
    final       int16 [H, W]: the 3 x 3 median of checked

Vectorised over rows x d per step; the scenes of tests/stereo_scenes.py take a few hundredths of a second each."""
import numpy as np

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3
MAX_SIDE = 16384
MAX_COST = 32767
MAX_WORKSPACE = 4 << 30
STAGES = {"pf_left": 0, "pf_right": 1, "C": 2, "S": 3, "raw": 4, "right": 5, "checked": 6}
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (1, 1), (1, -1))        # (dy, dx) of ->, <-, down, down-right, down-left

UNCONFIRMED = (
    "disp12MaxDiff <= 0 is taken as 1 and the left-right check always runs (cv2's documentation says a non-positive value disables it; "
    "the code, as recalled, does not)",
    "the right view's empty value is INVALID = (minDisparity - 1) * 16 and the check's probe accepts any value >= minDisparity, so "
    "for minDisparity >= 2 an empty right pixel is compared like a disparity (recalled from the code, not confirmed)",
    "the defaults P1 -> 2, P2 -> max(5, P1 + 1), uniquenessRatio < 0 -> 10 and ftzero = max(preFilterCap, 15) | 1",
    "the prefilter plane's first and last column hold ftzero, and its rows are replicated at the top and bottom edge",
    "the Birchfield-Tomasi half-sample values are (a + b) / 2 in integers and a plane's cost is shifted right by 2",
    "the block window replicates coordinates at the edges of the computed region (columns maxD .. W - 1), not of the image",
    "a path that enters the computed region starts from L = 0, m = 0; an out-of-range d - 1 / d + 1 term is 32767 + P1",
    "the five directions of the single-pass mode are ->, <-, down, down-right, down-left, and S saturates at 32767",
    "the lowest d wins a tie of min S; in the right view the largest x wins a tie of cost (a backward sweep with a strict >)",
    "the sub-pixel step divides with C's truncation and is skipped at d* = 0 and d* = D - 1",
    "the final medianBlur(disp, disp, 3) runs over the whole image, INVALID values included, with replicated borders",
    "3- and 4-channel input: this backend converts to grey first (the prototype's call order); cv2 sums a cost per channel",
)


class Params:
    """The normalised parameter set (csrc/stereo_plan.hpp: sgbm_normalise)."""

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                 speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM):
        self.minD, self.D, self.bs = int(minDisparity), int(numDisparities), int(blockSize)
        self.P1 = int(P1) if P1 > 0 else 2
        self.P2 = max(int(P2) if P2 > 0 else 5, self.P1 + 1)
        self.d12 = int(disp12MaxDiff) if disp12MaxDiff > 0 else 1
        self.uniq = int(uniquenessRatio) if uniquenessRatio >= 0 else 10
        self.ftzero = max(int(preFilterCap), 15) | 1
        self.maxD = self.minD + self.D
        self.invalid = (self.minD - 1) * 16
        self.raw = (int(minDisparity), int(numDisparities), int(blockSize), int(P1), int(P2), int(disp12MaxDiff), int(preFilterCap),
                    int(uniquenessRatio), int(speckleWindowSize), int(speckleRange), int(mode))

    def max_pixel_cost(self):
        """the Sobel plane spans 0 .. 2 ftzero, the intensity plane 0 .. 255, each shifted right by 2"""
        return ((2 * self.ftzero) >> 2) + (255 >> 2)

    def max_block_cost(self):
        return self.bs * self.bs * self.max_pixel_cost()


def check_create(max_w, max_h, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                 uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM):
    """-> None, or the message of the refusal (csrc/stereo_plan.hpp: sgbm_check_create, the same text)."""
    if mode != MODE_SGBM:
        return f"mode {mode} is not built (only MODE_SGBM = 0)"
    if speckleWindowSize > 0:
        return f"speckleWindowSize {speckleWindowSize}: the speckle filter is not built (want 0)"
    if minDisparity < 0:
        return f"minDisparity {minDisparity} < 0"
    if numDisparities < 16 or numDisparities > 256 or numDisparities % 16:
        return f"numDisparities {numDisparities} is not a multiple of 16 in 16..256"
    if blockSize < 1 or blockSize > 11 or blockSize % 2 == 0:
        return f"blockSize {blockSize} is not odd in 1..11"
    if preFilterCap < 0 or preFilterCap > 63:
        return f"preFilterCap {preFilterCap} outside 0..63"
    if uniquenessRatio > 100:
        return f"uniquenessRatio {uniquenessRatio} > 100"
    if not (1 <= max_w <= MAX_SIDE and 1 <= max_h <= MAX_SIDE):
        return f"image size {max_w}x{max_h} outside 1..{MAX_SIDE}"
    p = Params(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio)
    if p.max_block_cost() + p.P2 > MAX_COST:
        return (f"P2 {p.P2} with blockSize {p.bs}: the largest block cost {p.max_block_cost()} (= {p.bs}^2 x {p.max_pixel_cost()} per pixel) "
                f"+ P2 exceeds {MAX_COST}")
    ws = workspace_bytes(max_w, max_h, p.maxD, p.D)
    if ws > MAX_WORKSPACE:
        return f"workspace of {ws} bytes exceeds {MAX_WORKSPACE}"
    return None


def check_image(w, h, c, max_w, max_h):
    if c not in (1, 3, 4):
        return f"{c} channels (want 1, 3 or 4)"
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        return f"image size {w}x{h} outside 1..{MAX_SIDE}"
    if w > max_w or h > max_h:
        return f"image {w}x{h} is larger than the instance's {max_w}x{max_h}"
    return None


def _piece(nbytes):
    """one piece of an instance's slab (csrc/geom_slab.hpp: Slab::take)"""
    return (nbytes + 8 + 255) // 256 * 256


def workspace_bytes(max_w, max_h, maxD, D):
    """bytes of instance memory, in the order stereo_kernels.hip takes them"""
    px = max_w * max_h
    vol = max_h * max(max_w - maxD, 0) * D * 2
    return (2 * _piece(px * 4)          # staging of the host entry's two images
            + 2 * _piece(px)            # grey planes of a 3- / 4-channel pair
            + 2 * _piece(px)            # prefiltered planes
            + 3 * _piece(vol)           # row sums, C, S
            + _piece(max_h * max(max_w - maxD, 0) * 4)     # the selection's (cost, d) key
            + 4 * _piece(px * 2))       # raw, right, checked, final


def path_count(direction, H, W1):
    """paths of one direction over an H x W1 region (csrc/stereo_plan.hpp: sgbm_path_count)"""
    return H if direction < 2 else (W1 if direction == 2 else W1 + H - 1)


def path_start(direction, p, H, W1):
    """-> (y0, x0, length) of path p: every pixel of the region lies on exactly one path of a direction"""
    if direction == 0:
        return p, 0, W1
    if direction == 1:
        return p, W1 - 1, W1
    if direction == 2:
        return 0, p, H
    if direction == 3:
        y0, x0 = (0, p) if p < W1 else (p - W1 + 1, 0)
        return y0, x0, min(H - y0, W1 - x0)
    y0, x0 = (0, p) if p < W1 else (p - W1 + 1, W1 - 1)
    return y0, x0, min(H - y0, x0 + 1)


def bgr_to_grey(img):
    """BGR2GRAY in 15 fractional bits, an alpha channel ignored (csrc/feat_device.hpp: bgr_to_grey)"""
    if img.ndim == 2:
        return img
    b, g, r = (img[:, :, i].astype(np.int64) for i in range(3))
    return ((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def prefilter(img, ftzero):
    H, W = img.shape
    I = img.astype(np.int32)
    up, dn = I[np.maximum(np.arange(H) - 1, 0)], I[np.minimum(np.arange(H) + 1, H - 1)]
    out = np.full((H, W), ftzero, np.int32)
    if W > 2:
        g = 2 * (I[:, 2:] - I[:, :-2]) + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2])
        out[:, 1:-1] = np.clip(g, -ftzero, ftzero) + ftzero
    return out.astype(np.uint8)


def _half_range(P):
    """per pixel the min and max of the value and its two half-sample neighbours (replicated at the row ends)"""
    P = P.astype(np.int32)
    W = P.shape[1]
    l, r = P[:, np.maximum(np.arange(W) - 1, 0)], P[:, np.minimum(np.arange(W) + 1, W - 1)]
    hl, hr = (P + l) // 2, (P + r) // 2
    return P, np.minimum(P, np.minimum(hl, hr)), np.maximum(P, np.maximum(hl, hr))


def pixel_cost(planes_l, planes_r, p):
    """int32 [H, W1, D]: column maxD + xc against the right column maxD + xc - minD - d, summed over the planes"""
    H, W = planes_l[0].shape
    W1 = W - p.maxD
    x = p.maxD + np.arange(W1)[:, None]
    xr = x - p.minD - np.arange(p.D)[None, :]                 # [W1, D], 1 .. W - 1
    out = np.zeros((H, W1, p.D), np.int32)
    for L, R in zip(planes_l, planes_r):
        u, umin, umax = (a[:, x] for a in _half_range(L))      # [H, W1, 1]
        v, vmin, vmax = (a[:, xr] for a in _half_range(R))     # [H, W1, D]
        c0 = np.maximum(0, np.maximum(u - vmax, vmin - u))
        c1 = np.maximum(0, np.maximum(v - umax, umin - v))
        out += np.minimum(c0, c1) >> 2
    return out


def block_cost(pc, bs):
    H, W1, _ = pc.shape
    r = bs // 2
    rows = sum(pc[np.clip(np.arange(H) + k, 0, H - 1)] for k in range(-r, r + 1))
    return sum(rows[:, np.clip(np.arange(W1) + k, 0, W1 - 1)] for k in range(-r, r + 1)).astype(np.int16)


def path_step(Cp, Lq, mq, P1, P2):
    """one step of a path for any number of pixels: Cp, Lq int32 [n, D], mq int32 [n] -> L int32 [n, D]"""
    big = np.full((Lq.shape[0], 1), MAX_COST, np.int32)
    lo = np.concatenate([big, Lq[:, :-1]], 1) + P1
    hi = np.concatenate([Lq[:, 1:], big], 1) + P1
    return Cp + np.minimum(np.minimum(Lq, mq[:, None] + P2), np.minimum(lo, hi)) - mq[:, None]


def aggregate(C, P1, P2):
    """int16 S [H, W1, D]: a direction is swept along its axis, all pixels of a row (or a column) at once"""
    H, W1, D = C.shape
    C = C.astype(np.int32)
    total = np.zeros((H, W1, D), np.int32)
    for dy, dx in DIRECTIONS:
        L = np.zeros((H, W1, D), np.int32)
        if dy == 0:
            xs = range(W1) if dx > 0 else range(W1 - 1, -1, -1)
            for x in xs:
                q = x - dx
                Lq = L[:, q] if 0 <= q < W1 else np.zeros((H, D), np.int32)
                L[:, x] = path_step(C[:, x], Lq, Lq.min(1), P1, P2)
        else:
            for y in range(H):
                Lq = np.zeros((W1, D), np.int32)
                if y > 0:
                    src = np.arange(W1) - dx
                    ok = (src >= 0) & (src < W1)
                    Lq[ok] = L[y - 1, src[ok]]
                L[y] = path_step(C[y], Lq, Lq.min(1), P1, P2)
        total += L
    return np.minimum(total, MAX_COST).astype(np.int16)


def _trunc_div(n, m):
    return np.sign(n) * (np.abs(n) // m)


def select(S, p, W):
    """-> raw int16 [H, W], best d int32 [H, W1] (-1: rejected), its cost int32 [H, W1]"""
    H, W1, D = S.shape
    S = S.astype(np.int64)
    best = S.argmin(2)                                          # the lowest d of the minimum
    minS = np.take_along_axis(S, best[:, :, None], 2)[:, :, 0]
    d = np.arange(D)[None, None, :]
    reject = ((np.abs(d - best[:, :, None]) > 1) & (S * (100 - p.uniq) < minS[:, :, None] * 100)).any(2)
    lo = np.take_along_axis(S, np.maximum(best - 1, 0)[:, :, None], 2)[:, :, 0]
    hi = np.take_along_axis(S, np.minimum(best + 1, D - 1)[:, :, None], 2)[:, :, 0]
    den = np.maximum(lo + hi - 2 * minS, 1)
    sub = 16 * best + _trunc_div((lo - hi) * 16 + den, 2 * den)
    disp = np.where((best > 0) & (best < D - 1), sub, 16 * best) + 16 * p.minD
    raw = np.full((H, W), p.invalid, np.int16)
    raw[:, p.maxD:] = np.where(reject, p.invalid, disp).astype(np.int16)
    return raw, np.where(reject, -1, best).astype(np.int32), minS.astype(np.int32)


def right_view(best, minS, p, W):
    """int16 [H, W]: per right column the accepted left pixel of the smallest cost, the largest x among equals"""
    H, W1 = best.shape
    out = np.full((H, W), p.invalid, np.int16)
    cost = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    rows = np.arange(H)
    for xc in range(W1 - 1, -1, -1):                           # OpenCV's backward sweep with a strict >
        ok = best[:, xc] >= 0
        x2 = p.maxD + xc - best[:, xc] - p.minD
        take = ok & (cost[rows, np.where(ok, x2, 0)] > minS[:, xc])
        cost[rows[take], x2[take]] = minS[take, xc]
        out[rows[take], x2[take]] = (best[take, xc] + p.minD).astype(np.int16)
    return out


def lr_check(raw, right, p):
    H, W = raw.shape
    d1 = raw.astype(np.int32)
    r = right.astype(np.int32)
    x = np.arange(W)[None, :]
    bad = np.ones((H, W), bool)
    for dd in (d1 >> 4, (d1 + 15) >> 4):
        xp = x - dd
        inside = (xp >= 0) & (xp < W)
        v = np.take_along_axis(r, np.clip(xp, 0, W - 1), 1)
        bad &= inside & (v >= p.minD) & (np.abs(v - dd) > p.d12)
    bad &= raw != p.invalid
    bad[:, :min(p.maxD, W)] = False
    return np.where(bad, p.invalid, raw).astype(np.int16)


def median3(img):
    H, W = img.shape
    ys, xs = np.arange(H), np.arange(W)
    taps = [img[np.clip(ys + dy, 0, H - 1)][:, np.clip(xs + dx, 0, W - 1)] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    return np.sort(np.stack(taps), 0)[4].astype(img.dtype)


def compute_stages(left, right, p):
    """every stage of one pair as a dict (the keys of STAGES and 'final'); 2-D uint8 images of one size"""
    assert left.shape == right.shape and left.ndim == 2 and left.dtype == np.uint8 and right.dtype == np.uint8
    H, W = left.shape
    out = {"pf_left": prefilter(left, p.ftzero), "pf_right": prefilter(right, p.ftzero)}
    W1 = max(W - p.maxD, 0)
    if W1 == 0:
        out["C"] = out["S"] = np.zeros((H, 0, p.D), np.int16)
        out["raw"] = np.full((H, W), p.invalid, np.int16)
        out["right"] = out["raw"].copy()
    else:
        pc = pixel_cost((out["pf_left"], left), (out["pf_right"], right), p)
        out["C"] = block_cost(pc, p.bs)
        out["S"] = aggregate(out["C"], p.P1, p.P2)
        out["raw"], best, minS = select(out["S"], p, W)
        out["right"] = right_view(best, minS, p, W)
    out["checked"] = lr_check(out["raw"], out["right"], p)
    out["final"] = median3(out["checked"])
    return out


def compute(left, right, p):
    return compute_stages(left, right, p)["final"]


def lift(xy, disp_i16, P_left, P_right, min_disp, max_disp):
    """the keypoint lift in numpy: -> d float32 [n], mask bool [n], xy_right float32 [n, 2], X float64 [n, 3] (LAPACK's SVD of the
    DLT matrix OpenCV's triangulatePoints builds; NaN where the mask is clear)"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    H, W = disp_i16.shape
    n = len(xy)
    d = np.full(n, np.nan, np.float32)
    mask = np.zeros(n, bool)
    X = np.full((n, 3), np.nan)
    with np.errstate(invalid="ignore"):                         # (a NaN coordinate compares false: outside)
        inside = (xy[:, 0] > -1) & (xy[:, 0] < W) & (xy[:, 1] > -1) & (xy[:, 1] < H)
    xi, yi = np.where(inside, xy[:, 0], 0).astype(np.int64), np.where(inside, xy[:, 1], 0).astype(np.int64)      # int(): towards zero
    d[inside] = disp_i16[yi[inside], xi[inside]].astype(np.float32) / np.float32(16)
    mask[inside] = (d[inside] > np.float32(min_disp)) & (d[inside] < np.float32(max_disp))
    xr = np.stack([xy[:, 0] - d, xy[:, 1]], 1).astype(np.float32)
    P1, P2 = np.asarray(P_left, np.float64).reshape(3, 4), np.asarray(P_right, np.float64).reshape(3, 4)
    for i in np.flatnonzero(mask):
        A = np.stack([xy[i, 0] * P1[2] - P1[0], xy[i, 1] * P1[2] - P1[1], xr[i, 0] * P2[2] - P2[0], xr[i, 1] * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][3]
        if abs(v[3]) > 1e-12:
            X[i] = v[:3] / v[3]
        else:
            mask[i] = False
    return d, mask, xr, X
