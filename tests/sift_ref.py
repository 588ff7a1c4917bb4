"""SIFT as `cv2.SIFT_create(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma).detectAndCompute(img, None)`
computes it for 8-bit images, restated in numpy: the reference of csrc/sift_kernels.hip and csrc/sift_plan.hpp
(tests/test_sift_gpu.py, tests/test_sift_plan.py).  Everything is float32, one IEEE operation at a time in the order written
here (numpy float32 scalars and arrays round after every operation); `exp`, `pow`, `cos`, `sin` are the float64 function of the
float32 argument rounded once to float32; the two histograms are summed as 64-bit fixed-point integers (see THE HISTOGRAMS).

cv2 is not installed where this project is tested, so everything below is OpenCV 4.x `SIFT_Impl::detectAndCompute`
(features2d/src/sift.dispatch.cpp, sift.simd.hpp), `GaussianBlur` / `getGaussianKernel` on CV_32F, `resize(INTER_LINEAR)`,
`KeyPointsFilter` and `fastAtan2` RESTATED FROM MEMORY.  `UNCONFIRMED` lists what could not be checked against a real cv2.

THE HISTOGRAMS (a stated departure): OpenCV adds the contributions of the 36-bin orientation histogram and of the 4 x 4 x 8
descriptor histogram in float32 in an order that depends on its build (SIMD width).  Here every contribution is the float32
value OpenCV would add, converted to an integer at the scale 2^32 (truncated), the integers are summed - exact, so no order -
and the sum is converted back to float32 once.  The descriptor's orientation bins wrap in the integers.

THE ORDER: OpenCV's order after `retainBest` comes out of std::nth_element and is unspecified; here it is the order of
`KeyPoint_LessThan` (`removeDuplicatedSorted`): x, y ascending, size descending, angle ascending, response descending, octave
descending.  Duplicates (same pt, size, angle) are dropped before the cut; ties at the cut are kept.
"""
import math

import numpy as np

from orb_ref import ATAN_P, EPS32, F32, cv_round, gray, reflect101

UNCONFIRMED = (
    "BGR2GRAY: (B 3735 + G 19235 + R 9798 + 2^14) >> 15 (the KLT / ORB restatement)",
    "the base image: uint8 -> float32 (SIFT_FIXPT_SCALE 1), resize x2 INTER_LINEAR with source (d + 0.5) / 2 - 0.5 clamped at "
    "both ends (weights 0.25 / 0.75), firstOctave -1, enable_precise_upscale false, then GaussianBlur sqrt(max(sigma^2 - 1, 0.01))",
    "nOctaves = cvRound(log(min(cols, rows)) / log(2) - 2) + 1 on the doubled size (no lower clamp: below 1 nothing is computed)",
    "sig[i] = sqrt((sigma k^i)^2 - (sigma k^(i-1))^2) in double with k = pow(2, 1 / nOctaveLayers); nOctaveLayers + 3 layers",
    "GaussianBlur on CV_32F with ksize 0: ksize = cvRound(8 sigma + 1) | 1; taps exp(-x^2 / (2 sigma^2)) in double, normalised "
    "by the reciprocal of their double sum, rounded to float32; BORDER_REFLECT_101; row pass then column pass with a float32 "
    "intermediate; the accumulation order acc = acc + tap_k px_k for k ascending (OpenCV's SIMD filters may fuse or reorder)",
    "the next octave's base is layer nOctaveLayers decimated by INTER_NEAREST to cols / 2 x rows / 2 (integer division), which "
    "picks source pixel 2 d for every size",
    "DoG: layer i + 1 minus layer i in float32",
    "extrema: threshold = cvFloor(0.5 contrastThreshold / nOctaveLayers 255), border 5, |v| > threshold, v >= all 26 neighbours "
    "for v > 0 and <= for v < 0 (ties are all candidates)",
    "adjustLocalExtrema: 5 steps, finite differences with the scales 1/255, 0.5/255, 0.25/255 in float32, the expression "
    "order of each difference, the 3 x 3 solve as cv::LU (partial pivoting, eps 10 FLT_EPSILON, float32; OpenCV's Matx may take "
    "a closed form for 3 x 3) with a singular system taken as the zero step, the |x| < 0.5 exit, the INT_MAX / 3 guard, the move by cvRound",
    "the contrast test |contr| nOctaveLayers < contrastThreshold (float32 product compared in double) and the edge test "
    "det <= 0 or tr^2 edgeThreshold >= (edgeThreshold + 1)^2 det (float32 tr^2 and det, the products in double)",
    "pt = (c + xc) 2^octave; octave field octv + (layer << 8) + (cvRound((xi + 0.5) 255) << 16); size = sigma 2^((layer + xi) / "
    "nOctaveLayers) 2^octv 2 (powf, the product in double); response |contr|",
    "orientation: radius cvRound(4.5 scl), sigma 1.5 scl, samples with 0 < x < cols - 1 and 0 < y < rows - 1, weight "
    "exp((i^2 + j^2) (-1 / (2 sigma^2))), bin cvRound(0.1 Ori), the [1 4 6 4 1] / 16 smoothing and its expression order, peaks "
    "strictly above both neighbours and >= 0.8 max, the parabola, angle = 360 - 10 bin with |angle - 360| < FLT_EPSILON -> 0",
    "fastAtan2: the degree-7 polynomial of tests/orb_ref.py",
    "removeDuplicatedSorted (same pt, size, angle), retainBest(n): everything >= the n-th largest response, 0 = no cut",
    "firstOctave -1: pt and size halved, octave field (o & ~255) | ((o - 1) & 255)",
    "descriptor: d 4, n 8, hist_width 3 scl, radius cvRound(hist_width 1.4142135623730951f 5 0.5f) clipped to the image "
    "diagonal, cos / sin divided by hist_width, samples with rbin, cbin in (-1, 4) and 0 < r < rows - 1, 0 < c < cols - 1, weight "
    "exp((c_rot^2 + r_rot^2) (-1 / 8)), trilinear spreading in the order r, c, o, clamp at 0.2 norm, scale 512 / max(norm, "
    "FLT_EPSILON), saturate_cast<uchar> (round half to even), stored as float32; the two norms as float32 sums in index order",
)

IMG_BORDER, MAX_INTERP_STEPS, ORI_BINS, DESCR_W, DESCR_BINS = 5, 5, 36, 4, 8
MAX_OCTAVES = 16
HIST_SCALE_LOG2 = 32
FLT_EPSILON = F32(1.1920929e-07)


# ---- parameters and the plan's numbers ------------------------------------------------------------------------------------
def check_params(nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6):
    """-> the word of the refusal, or None"""
    if nfeatures < 0:
        return "nfeatures"
    if not 1 <= nOctaveLayers <= 8:
        return "nOctaveLayers"
    if not contrastThreshold > 0:
        return "contrastThreshold"
    if not edgeThreshold > 0:
        return "edgeThreshold"
    if not 0.5 < sigma <= 8:
        return "sigma"
    return None


def n_octaves(w, h):
    """on the ORIGINAL size; 0 when the doubled image is too small for one"""
    return max(cv_round(math.log(float(min(2 * w, 2 * h))) / math.log(2.0) - 2) + 1, 0)


def octave_sizes(w, h):
    out, ow, oh = [], 2 * w, 2 * h
    for _ in range(min(n_octaves(w, h), MAX_OCTAVES)):
        if ow < 1 or oh < 1:
            break
        out.append((ow, oh))
        ow, oh = ow // 2, oh // 2
    return out


def sigmas(sigma, nol):
    """[base blur, sig[1] .. sig[nol + 2]] in double"""
    out = [math.sqrt(max(sigma * sigma - 1.0, 0.01))]
    k = math.pow(2.0, 1.0 / nol)
    for i in range(1, nol + 3):
        prev = math.pow(k, float(i - 1)) * sigma
        total = prev * k
        out.append(math.sqrt(total * total - prev * prev))
    return out


def gauss_taps(sigma):
    n = cv_round(sigma * 8 + 1) | 1
    s2 = -0.5 / (sigma * sigma)
    t = [math.exp(s2 * (i - (n - 1) * 0.5) ** 2) for i in range(n)]
    inv = 1.0 / _seq_sum(t)
    return np.array([v * inv for v in t], np.float64).astype(np.float32)


def _seq_sum(v):
    s = 0.0
    for x in v:
        s += x
    return s


def threshold(contrast, nol):
    return int(math.floor(0.5 * contrast / nol * 255))


# ---- the scale space ---------------------------------------------------------------------------------------------------
def upscale2(g):
    """uint8 [h, w] -> float32 [2 h, 2 w], INTER_LINEAR (exact in float32 for 8-bit input)"""
    h, w = g.shape
    f = g.astype(np.float32)

    def taps(n):
        d = np.arange(2 * n)
        s = np.where(d % 2 == 0, d // 2 - 1, d // 2)
        fr = np.where(d % 2 == 0, F32(0.75), F32(0.25)).astype(np.float32)
        fr = np.where((s < 0) | (s >= n - 1), F32(0), fr).astype(np.float32)
        s = np.clip(s, 0, n - 1)
        return s, np.minimum(s + 1, n - 1), fr
    x0, x1, fx = taps(w)
    y0, y1, fy = taps(h)
    hz = f[:, x0] * (F32(1) - fx) + f[:, x1] * fx
    return hz[y0] * (F32(1) - fy)[:, None] + hz[y1] * fy[:, None]


def blur(img, taps):
    """row pass then column pass, acc = acc + tap_k px_k for k ascending, in img's dtype (float32: the defined form)"""
    dt = img.dtype
    taps = taps.astype(dt)
    h, w = img.shape
    r = len(taps) // 2
    ix = reflect101(np.arange(-r, w + r), w)
    acc = np.zeros((h, w), dt)
    for k in range(len(taps)):
        acc = acc + taps[k] * img[:, ix[k:k + w]]
    iy = reflect101(np.arange(-r, h + r), h)
    out = np.zeros((h, w), dt)
    for k in range(len(taps)):
        out = out + taps[k] * acc[iy[k:k + h]]
    return out


def pyramid(g, nol=3, sigma=1.6, dtype=np.float32):
    """grey uint8 -> (gauss, dog): per octave [nol + 3, h, w] and [nol + 2, h, w]"""
    sig = sigmas(sigma, nol)
    taps = [gauss_taps(s) for s in sig]
    h, w = g.shape
    sizes = octave_sizes(w, h)
    gauss, dog = [], []
    for o, (ow, oh) in enumerate(sizes):
        G = np.empty((nol + 3, oh, ow), dtype)
        if o == 0:
            G[0] = blur(upscale2(g).astype(dtype), taps[0])
        else:
            G[0] = gauss[o - 1][nol][::2, ::2][:oh, :ow]
        for i in range(1, nol + 3):
            G[i] = blur(G[i - 1], taps[i])
        gauss.append(G)
        dog.append(G[1:] - G[:-1])
    return gauss, dog


# ---- extrema and their refinement -----------------------------------------------------------------------------------------
def extrema(D, nol, thr):
    """D: [nol + 2, h, w] -> int [K, 3] (layer, r, c) in row-major order"""
    _, h, w = D.shape
    b = IMG_BORDER
    if h <= 2 * b or w <= 2 * b:
        return np.zeros((0, 3), np.int64)
    out = []
    for i in range(1, nol + 1):
        v = D[i, b:h - b, b:w - b]
        ge = np.ones(v.shape, bool)
        le = np.ones(v.shape, bool)
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    nb = D[i + dl, b + dy:h - b + dy, b + dx:w - b + dx]
                    ge &= v >= nb
                    le &= v <= nb
        ok = (np.abs(v) > F32(thr)) & (((v > 0) & ge) | ((v < 0) & le))
        ys, xs = np.nonzero(ok)
        out += [(i, y + b, x + b) for y, x in zip(ys.tolist(), xs.tolist())]
    return np.array(out, np.int64).reshape(-1, 3)


def lu_solve3(A, b):
    """cv::LU on float32 copies; a singular system gives the zero vector"""
    A = [[F32(v) for v in row] for row in A]
    b = [F32(v) for v in b]
    eps = FLT_EPSILON * F32(10)
    for i in range(3):
        k = i
        for j in range(i + 1, 3):
            if abs(A[j][i]) > abs(A[k][i]):
                k = j
        if abs(A[k][i]) < eps:
            return [F32(0)] * 3
        if k != i:
            A[i], A[k] = A[k], A[i]
            b[i], b[k] = b[k], b[i]
        d = F32(-1) / A[i][i]
        for j in range(i + 1, 3):
            alpha = A[j][i] * d
            for c in range(i + 1, 3):
                A[j][c] = A[j][c] + alpha * A[i][c]
            b[j] = b[j] + alpha * b[i]
    for i in (2, 1, 0):
        s = b[i]
        for c in range(i + 1, 3):
            s = s - A[i][c] * b[c]
        b[i] = s / A[i][i]
    return b


IMG_SCALE = F32(1) / F32(255)
DERIV_SCALE, SECOND_SCALE, CROSS_SCALE = IMG_SCALE * F32(0.5), IMG_SCALE, IMG_SCALE * F32(0.25)


def _dD(D, l, r, c):
    img, prev, nxt = D[l], D[l - 1], D[l + 1]
    return [(img[r, c + 1] - img[r, c - 1]) * DERIV_SCALE, (img[r + 1, c] - img[r - 1, c]) * DERIV_SCALE,
            (nxt[r, c] - prev[r, c]) * DERIV_SCALE]


def _hess2(D, l, r, c):
    img = D[l]
    v2 = img[r, c] * F32(2)
    dxx = (img[r, c + 1] + img[r, c - 1] - v2) * SECOND_SCALE
    dyy = (img[r + 1, c] + img[r - 1, c] - v2) * SECOND_SCALE
    dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * CROSS_SCALE
    return v2, dxx, dyy, dxy


def adjust(D, octv, layer, r, c, nol, contrast, edge, sigma, why=None):
    """-> None (the reason appended to `why`: steps, huge, left, contrast, edge), or dict(r, c, layer, xi, x, y, size, response,
    octave) in the frame of the doubled image"""
    def no(reason):
        if why is not None:
            why.append(reason)
        return None
    _, h, w = D.shape
    xi = xr = xc = F32(0)
    for step in range(MAX_INTERP_STEPS + 1):
        if step == MAX_INTERP_STEPS:
            return no("steps")
        img, prev, nxt = D[layer], D[layer - 1], D[layer + 1]
        dD = _dD(D, layer, r, c)
        v2, dxx, dyy, dxy = _hess2(D, layer, r, c)
        dss = (nxt[r, c] + prev[r, c] - v2) * SECOND_SCALE
        dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prev[r, c + 1] + prev[r, c - 1]) * CROSS_SCALE
        dys = (nxt[r + 1, c] - nxt[r - 1, c] - prev[r + 1, c] + prev[r - 1, c]) * CROSS_SCALE
        X = lu_solve3([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], dD)
        xi, xr, xc = -X[2], -X[1], -X[0]
        if abs(xi) < F32(0.5) and abs(xr) < F32(0.5) and abs(xc) < F32(0.5):
            break
        big = F32(2147483647 // 3)
        if abs(xi) > big or abs(xr) > big or abs(xc) > big:
            return no("huge")
        c += cv_round(xc)
        r += cv_round(xr)
        layer += cv_round(xi)
        if layer < 1 or layer > nol or c < IMG_BORDER or c >= w - IMG_BORDER or r < IMG_BORDER or r >= h - IMG_BORDER:
            return no("left")
    dD = _dD(D, layer, r, c)
    t = dD[0] * xc
    t = t + dD[1] * xr
    t = t + dD[2] * xi
    contr = D[layer][r, c] * IMG_SCALE + t * F32(0.5)
    if float(abs(contr) * F32(nol)) < contrast:
        return no("contrast")
    _, dxx, dyy, dxy = _hess2(D, layer, r, c)
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    if det <= 0 or float(tr * tr) * edge >= (edge + 1) * (edge + 1) * float(det):
        return no("edge")
    p2 = F32(1 << octv)
    arg = (F32(layer) + xi) / F32(nol)
    pw = F32(math.pow(2.0, float(arg)))
    return dict(r=r, c=c, layer=layer, xi=xi, x=(F32(c) + xc) * p2, y=(F32(r) + xr) * p2,
                size=F32(sigma * float(pw) * (1 << octv) * 2), response=abs(contr),
                octave=octv + (layer << 8) + (cv_round((xi + F32(0.5)) * F32(255)) << 16))


# ---- vector pieces shared by the orientation and the descriptor ----------------------------------------------------------
def fast_atan2_v(y, x):
    y, x = np.asarray(y, np.float32), np.asarray(x, np.float32)
    ax, ay = np.abs(x), np.abs(y)
    p1, p3, p5, p7 = ATAN_P
    swap = ~(ax >= ay)
    num, den = np.where(swap, ax, ay), np.where(swap, ay, ax) + EPS32
    c = (num / den).astype(np.float32)
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(swap, F32(90) - a, a)
    a = np.where(x < 0, F32(180) - a, a)
    a = np.where(y < 0, F32(360) - a, a)
    return a.astype(np.float32)


def exp32(x):
    return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def to_fixed(v):
    """float32 >= 0 -> int64 at 2^32, truncated"""
    return np.floor(np.asarray(v, np.float32).astype(np.float64) * float(1 << HIST_SCALE_LOG2)).astype(np.int64)


def from_fixed(s):
    return (np.asarray(s, np.int64).astype(np.float64) / float(1 << HIST_SCALE_LOG2)).astype(np.float32)


def _gradients(img, ys, xs):
    dx = img[ys, xs + 1] - img[ys, xs - 1]
    dy = img[ys - 1, xs] - img[ys + 1, xs]
    mag = np.sqrt(dx * dx + dy * dy)
    return fast_atan2_v(dy, dx), mag


def orientation_hist(img, px, py, radius, sigma):
    """-> float32 [36] smoothed histogram"""
    h, w = img.shape
    scale = F32(-1) / (F32(2) * sigma * sigma)
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    i, j = i.ravel(), j.ravel()
    ys, xs = py + i, px + j
    ok = (ys > 0) & (ys < h - 1) & (xs > 0) & (xs < w - 1)
    i, j, ys, xs = i[ok], j[ok], ys[ok], xs[ok]
    wgt = exp32((i * i + j * j).astype(np.float32) * scale)
    ori, mag = _gradients(img, ys, xs)
    b = np.rint(F32(ORI_BINS / 360.0) * ori).astype(np.int64)
    b = np.where(b >= ORI_BINS, b - ORI_BINS, b)
    b = np.where(b < 0, b + ORI_BINS, b)
    acc = np.zeros(ORI_BINS, np.int64)
    np.add.at(acc, b, to_fixed(wgt * mag))
    t = from_fixed(acc)
    m2, m1, p1, p2 = np.roll(t, 2), np.roll(t, 1), np.roll(t, -1), np.roll(t, -2)
    return (m2 + p2) * F32(1 / 16) + (m1 + p1) * F32(4 / 16) + t * F32(6 / 16)


def orientation_peaks(hist):
    """-> list of float32 keypoint angles"""
    thr = hist.max() * F32(0.8)
    n = ORI_BINS
    out = []
    for j in range(n):
        l, r2 = (j - 1) % n, (j + 1) % n
        if hist[j] > hist[l] and hist[j] > hist[r2] and hist[j] >= thr:
            den = hist[l] - F32(2) * hist[j]
            den = den + hist[r2]
            b = F32(j) + (F32(0.5) * (hist[l] - hist[r2])) / den
            b = F32(n) + b if b < 0 else (b - F32(n) if b >= n else b)
            ang = F32(360) - F32(360 / n) * b
            if abs(ang - F32(360)) < FLT_EPSILON:
                ang = F32(0)
            out.append(F32(ang))
    return out


def unpack_octave(field):
    octave, layer = field & 255, (field >> 8) & 255
    octave = octave if octave < 128 else octave - 256
    scale = F32(1) / F32(1 << octave) if octave >= 0 else F32(1 << -octave)
    return octave, layer, scale


def descriptor(img, px, py, ori, scl):
    """img: the Gaussian layer, (px, py) float32 in its frame, ori degrees (360 - kpt.angle), scl -> float32 [128]"""
    d, n = DESCR_W, DESCR_BINS
    h, w = img.shape
    ix, iy = cv_round(px), cv_round(py)
    rad = F32(ori) * F32(math.pi / 180)
    cos_t, sin_t = F32(math.cos(float(rad))), F32(math.sin(float(rad)))
    bins_per_deg = F32(n) / F32(360)
    exp_scale = F32(-1) / (F32(d) * F32(d) * F32(0.5))
    hist_width = F32(3) * F32(scl)
    radius = cv_round(hist_width * F32(1.4142135623730951) * F32(d + 1) * F32(0.5))
    radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
    cos_t, sin_t = cos_t / hist_width, sin_t / hist_width
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    i, j = i.ravel(), j.ravel()
    fi, fj = i.astype(np.float32), j.astype(np.float32)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin = r_rot + F32(d // 2) - F32(0.5)
    cbin = c_rot + F32(d // 2) - F32(0.5)
    ys, xs = iy + i, ix + j
    ok = (rbin > -1) & (rbin < d) & (cbin > -1) & (cbin < d) & (ys > 0) & (ys < h - 1) & (xs > 0) & (xs < w - 1)
    rbin, cbin, ys, xs, c_rot, r_rot = rbin[ok], cbin[ok], ys[ok], xs[ok], c_rot[ok], r_rot[ok]
    wgt = exp32((c_rot * c_rot + r_rot * r_rot) * exp_scale)
    o, mag = _gradients(img, ys, xs)
    obin = (o - F32(ori)) * bins_per_deg
    mag = mag * wgt
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + n, o0)
    o0 = np.where(o0 >= n, o0 - n, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    acc = np.zeros((d, d, n), np.int64)
    for dr, vr in ((0, v_r0), (1, v_r1)):
        v_c1 = vr * cbin
        v_c0 = vr - v_c1
        for dc, vc in ((0, v_c0), (1, v_c1)):
            v_o1 = vc * obin
            v_o0 = vc - v_o1
            for do, vo in ((0, v_o0), (1, v_o1)):
                rr, cc, oo = r0 + dr, c0 + dc, (o0 + do) % n
                inside = (rr >= 0) & (rr < d) & (cc >= 0) & (cc < d)
                np.add.at(acc, (rr[inside], cc[inside], oo[inside]), to_fixed(vo[inside]))
    dst = from_fixed(acc.ravel())
    nrm2 = F32(0)
    for v in dst:
        nrm2 = nrm2 + v * v
    thr = np.sqrt(nrm2) * F32(0.2)
    dst = np.minimum(dst, thr)
    nrm2 = F32(0)
    for v in dst:
        nrm2 = nrm2 + v * v
    s = F32(512) / max(np.sqrt(nrm2), FLT_EPSILON)
    return np.clip(np.rint(dst * s), 0, 255).astype(np.float32)


# ---- the whole detector ---------------------------------------------------------------------------------------------------
def sort_key(k):
    return (float(k["x"]), float(k["y"]), -float(k["size"]), float(k["angle"]), -float(k["response"]), -k["octave"])


def detect(img, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6):
    """-> dict: xy float32 [N,2], aux float32 [N,3] (size, angle, response), octave int32 [N], desc float32 [N,128], and the
    stages: sizes, gauss, dog (per octave), cand (per octave: int [K,3] layer, r, c), refined {(o, layer, r, c): dict or None},
    rejects {(o, layer, r, c): reason}, hists {(o, layer, r, c): float32 [36]}, raw (the keypoints before duplicates and the quota, in
    the frame of the doubled image), n_raw, n_unique"""
    assert check_params(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma) is None
    nol = nOctaveLayers
    g = gray(img)
    gauss, dog = pyramid(g, nol, sigma)
    thr = threshold(contrastThreshold, nol)
    cands, refined, hists, raw, rejects = [], {}, {}, [], {}
    for o, D in enumerate(dog):
        cand = extrema(D, nol, thr)
        cands.append(cand)
        for layer, r, c in cand.tolist():
            why = []
            k = adjust(D, o, layer, r, c, nol, contrastThreshold, edgeThreshold, sigma, why)
            refined[(o, layer, r, c)] = k
            if k is None:
                rejects[(o, layer, r, c)] = why[0]
                continue
            scl = k["size"] * F32(0.5) / F32(1 << o)
            hist = orientation_hist(gauss[o][k["layer"]], k["c"], k["r"], cv_round(F32(4.5) * scl), F32(1.5) * scl)
            hists[(o, layer, r, c)] = hist
            for ang in orientation_peaks(hist):
                raw.append(dict(k, angle=ang))
    kps = sorted(raw, key=sort_key)
    uniq = []
    for k in kps:
        if uniq and (uniq[-1]["x"], uniq[-1]["y"], uniq[-1]["size"], uniq[-1]["angle"]) == (k["x"], k["y"], k["size"], k["angle"]):
            continue
        uniq.append(k)
    n_unique = len(uniq)
    if nfeatures > 0 and len(uniq) > nfeatures:
        cut = sorted((k["response"] for k in uniq), reverse=True)[nfeatures - 1]
        uniq = [k for k in uniq if k["response"] >= cut]
    xy, aux, octs, desc = [], [], [], []
    for k in uniq:
        field = (k["octave"] & ~255) | ((k["octave"] - 1) & 255)
        x, y, size = k["x"] * F32(0.5), k["y"] * F32(0.5), k["size"] * F32(0.5)
        octave, layer, scale = unpack_octave(field)
        ang = F32(360) - k["angle"]
        if abs(ang - F32(360)) < FLT_EPSILON:
            ang = F32(0)
        desc.append(descriptor(gauss[octave + 1][layer], x * scale, y * scale, ang, size * scale * F32(0.5)))
        xy.append((x, y))
        aux.append((size, k["angle"], k["response"]))
        octs.append(field)
    n = len(xy)
    return dict(xy=np.array(xy, np.float32).reshape(n, 2), aux=np.array(aux, np.float32).reshape(n, 3),
                octave=np.array(octs, np.int32).reshape(n), desc=np.array(desc, np.float32).reshape(n, 128),
                sizes=octave_sizes(g.shape[1], g.shape[0]), gauss=gauss, dog=dog, cand=cands, refined=refined, hists=hists,
                raw=raw, rejects=rejects, n_raw=len(kps), n_unique=n_unique, threshold=thr)
