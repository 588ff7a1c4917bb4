"""ORB as `cv2.ORB_create(...).detectAndCompute(img, None)` computes it for 8-bit images, restated in numpy: the reference of
csrc/orb_kernels.hip and csrc/orb_plan.hpp (tests/test_orb_gpu.py, tests/test_orb_plan.py).  Every stage up to the response is
integer arithmetic; the float32 tails run one IEEE operation at a time in the order written here.

cv2 is not installed where this project is tested, so everything below is OpenCV's `ORB_Impl::detectAndCompute` (features2d/
src/orb.cpp), `FAST_t<16>` / `cornerScore<16>` (fast.cpp, fast_score.cpp), `KeyPointsFilter` (keypoint.cpp), `fastAtan2`
(mathfuncs_core), `resize(INTER_LINEAR_EXACT)` and `GaussianBlur` on uint8 (fixed-point paths) RESTATED FROM MEMORY.  What could
not be confirmed against a real cv2, each a place where keypoints or bits may differ from cv2's:

 1. INTER_LINEAR_EXACT: the coefficient width (8 fractional bits per axis here, products kept exact, one rounding at the end:
    (v + 2^15) >> 16) and how a coefficient is rounded (here round-half-up of the exact rational frac * 256, the source
    coordinate being the exact rational ((2 dx + 1) sw - dw) / (2 dw); clamped taps get coefficient 0).  OpenCV's ufixedpoint16
    path may round the coefficient from a double and may round after the horizontal pass.
 2. GaussianBlur 7x7 sigma 2 on uint8: taken as a separable 8-fractional-bit kernel, round(256 g_i) with the centre adjusted so
    the taps sum to 256 -> [18 34 49 54 49 34 18], both passes exact, one rounding (v + 2^15) >> 16.  OpenCV's widths, its
    adjustment rule and whether it rounds between the passes are unconfirmed.  OpenCV blurs the level IN PLACE inside its
    bordered pyramid, so a tap beyond the level's edge reads an unblurred border pixel there; here the blurred level gets the
    reflect-101 border of its own blurred interior.  (With the default edgeThreshold 31 no tap leaves the interior.)
 3. `KeyPointsFilter::retainBest`: taken as "if more than n, keep everything whose response is >= the n-th largest" (ties at
    the cut all kept), n = 0 keeps nothing.
 4. `fastAtan2`: the degree-7 polynomial's coefficients (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
    -0.04432655554792128, each times (float)(180 / pi) in float32), the `+ (float)DBL_EPSILON` in the divisor and the order of
    the quadrant fix-ups.  Stated accuracy 0.3 degrees.
 5. The FAST score: `cornerScore<16>` taken as the largest threshold at which the pixel is still a corner,
    max(max_k min_9 (v - c), max_k min_9 (c - v)) - 1; OpenCV computes it with a specific min/max network started at the
    detection threshold, believed to give this value.
 6. The level sizes: `cvRound(cols * (1 / scale))` with scale = (float)pow(scaleFactor, level), in float32; the scale factor
    itself is the float32 the Python binding passes.  The quotas in float32 as `ORB_Impl` spells them.
 7. `runByImageBorder(edgeThreshold)`: kept iff edge <= x < w - edge and edge <= y < h - edge.
 8. The Harris response's 3x3 derivative and its float expression order; `umax` and its symmetry fix-up; IC_Angle's sums.
 9. cos / sin of the angle: float64 libm rounded once to float32 (a device libm that differs from this one in the last float64
    bit changes a float32 only at a rounding boundary, ~1e-8 of all angles).
10. BGR2GRAY: (B 3735 + G 19235 + R 9798 + 2^14) >> 15 (the KLT front end's restatement).

THE STATED DEVIATION: for patchSize 31 OpenCV samples a learned 256-pair table (`bit_pattern_31_`) that is not available here.
The default pattern is what OpenCV generates for every OTHER patch size - `makeRandomPattern`: cv::RNG(0x34985739), 512 points,
x then y of each from uniform(-15, 16) - so descriptors are self-consistent but not interchangeable with cv2's.  `pattern=` takes
the learned table from a user who has it.

THE ORDER: OpenCV's order within a level comes out of std::nth_element and is unspecified; here it is level ascending, response
descending (by the monotone integer image of the float32), then y, then x.
"""
import math

import numpy as np

HARRIS_SCORE, FAST_SCORE = 0, 1
PATCH, HALF, HARRIS_BLOCK, REACH = 31, 15, 7, 22
MAX_LEVELS = 16
# (dx, dy) of the 16 circle pixels, clockwise from (0, 3)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
          (-3, 1), (-2, 2), (-1, 3))
F32 = np.float32


def cv_round(x):
    return int(np.rint(x))


class CvRNG:
    """cv::RNG (restated once more so that this file stands alone; tests compare it with oracle.ransac_ref.CvRNG)."""

    def __init__(self, state):
        self.state = state

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else int(self.next() % (b - a) + a)


def default_pattern():
    """makeRandomPattern(31, pattern, 512) -> int8 [512, 2] (x, y)."""
    rng = CvRNG(0x34985739)
    out = np.empty((512, 2), np.int8)
    for i in range(512):
        out[i, 0] = rng.uniform(-(PATCH // 2), PATCH // 2 + 1)
        out[i, 1] = rng.uniform(-(PATCH // 2), PATCH // 2 + 1)
    return out


def border(edge):
    return max(edge, REACH, (HARRIS_BLOCK + 2) // 2) + 1


def scale_factor(sf):
    """the float32 the binding passes, as the double ORB_Impl stores"""
    return float(F32(sf))


def level_scales(sf, nlevels):
    return [F32(scale_factor(sf) ** level) for level in range(nlevels)]


def level_sizes(w, h, sf, nlevels):
    out = []
    for s in level_scales(sf, nlevels):
        inv = F32(1) / s
        out.append((cv_round(F32(w) * inv), cv_round(F32(h) * inv)))
    return out


def quotas(nfeatures, sf, nlevels):
    factor = F32(1.0 / scale_factor(sf))
    nd = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(float(factor) ** nlevels))
    out, total = [], 0
    for _ in range(nlevels - 1):
        out.append(cv_round(nd))
        total += out[-1]
        nd = nd * factor
    out.append(max(nfeatures - total, 0))
    return out


def umax_table():
    vmax = int(math.floor(HALF * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(HALF * math.sqrt(2.0) / 2))
    u = [0] * (HALF + 2)
    for v in range(vmax + 1):
        u[v] = cv_round(math.sqrt(float(HALF * HALF - v * v)))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return u[:HALF + 1]


def gauss_taps():
    g = np.exp(-np.arange(-3, 4, dtype=np.float64) ** 2 / (2 * 2.0 * 2.0))
    k = np.rint(g / g.sum() * 256).astype(np.int64)
    k[3] += 256 - k.sum()
    return k


def gray(img):
    img = np.asarray(img)
    if img.ndim == 2 or img.shape[2] == 1:
        return img.reshape(img.shape[0], img.shape[1]).copy()
    i = img.astype(np.int64)
    return ((i[..., 0] * 3735 + i[..., 1] * 19235 + i[..., 2] * 9798 + (1 << 14)) >> 15).astype(np.uint8)


def reflect101(i, n):
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def pad101(img, b):
    h, w = img.shape
    return img[reflect101(np.arange(-b, h + b), h)][:, reflect101(np.arange(-b, w + b), w)]


def _coeffs(sn, dn):
    d = np.arange(dn, dtype=np.int64)
    num, den = (2 * d + 1) * sn - dn, 2 * dn
    s = num // den
    c = ((num - s * den) * 512 + den) // (2 * den)
    c = np.where((s < 0) | (s >= sn - 1), 0, c)
    s = np.clip(s, 0, sn - 1)
    return s, np.minimum(s + 1, sn - 1), c


def resize_exact(src, dw, dh):
    sh, sw = src.shape
    x0, x1, cx = _coeffs(sw, dw)
    y0, y1, cy = _coeffs(sh, dh)
    s = src.astype(np.int64)
    hz = (256 - cx) * s[:, x0] + cx * s[:, x1]
    v = (256 - cy)[:, None] * hz[y0] + cy[:, None] * hz[y1]
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


def blur(img):
    """7x7 sigma 2 of the level with reflect-101 at its edge"""
    k = gauss_taps()
    h, w = img.shape
    p = pad101(img, 3).astype(np.int64)
    hz = sum(k[i] * p[:, i:i + w] for i in range(7))
    v = sum(k[j] * hz[j:j + h] for j in range(7))
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


def fast_score_map(img, t):
    """[h, w] int: the FAST-9/16 score where the pixel is a corner at threshold t and at least 3 from the edge, else 0"""
    h, w = img.shape
    out = np.zeros((h, w), np.int64)
    if h < 7 or w < 7:
        return out
    i = img.astype(np.int64)
    v = i[3:h - 3, 3:w - 3]
    d = np.stack([v - i[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
    d = np.concatenate([d, d[:8]])
    best = None
    for k in range(16):
        a = d[k:k + 9]
        m = np.maximum(a.min(0), (-a).min(0))
        best = m if best is None else np.maximum(best, m)
    s = best - 1
    out[3:h - 3, 3:w - 3] = np.where(s >= t, s, 0)
    return out


def nms(score):
    h, w = score.shape
    p = np.zeros((h + 2, w + 2), score.dtype)
    p[1:-1, 1:-1] = score
    keep = score > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                keep &= score > p[dy:dy + h, dx:dx + w]
    return keep


def retain_cut(values, n, none, everything):
    """the cut of retainBest(n) on `values`: `everything` when nothing is dropped, `none` for n = 0, else the n-th largest"""
    if len(values) <= n:
        return everything
    if n == 0:
        return none
    return np.sort(values)[::-1][n - 1]


def harris_abc(P, b, x, y):
    """P: the padded level (int64), (x, y) interior coordinates -> exact (sum Ix^2, sum Ix Iy, sum Iy^2) over the 7x7 block"""
    A = B = C = 0
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            r, c = y + b + dy, x + b + dx
            ix = (P[r, c + 1] - P[r, c - 1]) * 2 + (P[r - 1, c + 1] - P[r - 1, c - 1]) + (P[r + 1, c + 1] - P[r + 1, c - 1])
            iy = (P[r + 1, c] - P[r - 1, c]) * 2 + (P[r + 1, c - 1] - P[r - 1, c - 1]) + (P[r + 1, c + 1] - P[r - 1, c + 1])
            A += ix * ix
            B += ix * iy
            C += iy * iy
    return int(A), int(B), int(C)


def harris_scale4():
    s = F32(1) / F32(4 * HARRIS_BLOCK * 255)
    return s * s * s * s


def harris_response(A, B, C):
    fa, fb, fc = F32(A), F32(B), F32(C)
    t1, t2, sm = fa * fc, fb * fb, fa + fc
    t3 = (F32(0.04) * sm) * sm
    return ((t1 - t2) - t3) * harris_scale4()


def moments(P, b, x, y, umax):
    m01 = m10 = 0
    r, c = y + b, x + b
    for u in range(-HALF, HALF + 1):
        m10 += u * int(P[r, c + u])
    for v in range(1, HALF + 1):
        vs = 0
        for u in range(-umax[v], umax[v] + 1):
            p, m = int(P[r + v, c + u]), int(P[r - v, c + u])
            vs += p - m
            m10 += u * (p + m)
        m01 += v * vs
    return m01, m10


ATAN_P = [F32(c) * F32(180 / math.pi) for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)]
EPS32 = F32(2.220446049250313e-16)


def fast_atan2(y, x):
    y, x = F32(y), F32(x)
    ax, ay = np.abs(x), np.abs(y)
    p1, p3, p5, p7 = ATAN_P
    if ax >= ay:
        c = ay / (ax + EPS32)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    else:
        c = ax / (ay + EPS32)
        c2 = c * c
        a = F32(90) - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    if x < 0:
        a = F32(180) - a
    if y < 0:
        a = F32(360) - a
    return F32(a)


def float_key(f):
    """the monotone uint32 image of float32 values"""
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def rotation(angle):
    rad = F32(angle) * F32(math.pi / 180.0)
    return F32(math.cos(float(rad))), F32(math.sin(float(rad)))


def descriptor(Pb, b, x, y, angle, pattern):
    """Pb: the padded blurred level -> uint8 [32]"""
    a, s = rotation(angle)
    px, py = pattern[:, 0].astype(np.float32), pattern[:, 1].astype(np.float32)
    ix = np.rint(px * a - py * s).astype(np.int64)
    iy = np.rint(px * s + py * a).astype(np.int64)
    t = Pb[y + b + iy, x + b + ix].astype(np.int64)
    bits = (t[0::2] < t[1::2]).astype(np.uint8)
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


def check_params(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, firstLevel=0, WTA_K=2, scoreType=0, patchSize=31,
                 fastThreshold=20):
    """-> the word of the refusal, or None"""
    if not nfeatures >= 1:
        return "nfeatures"
    if not 1.0 < scale_factor(scaleFactor) <= 2.0:
        return "scaleFactor"
    if not 1 <= nlevels <= MAX_LEVELS:
        return "nlevels"
    if not edgeThreshold >= 3:
        return "edgeThreshold"
    if firstLevel != 0:
        return "firstLevel"
    if WTA_K != 2:
        return "WTA_K"
    if scoreType not in (0, 1):
        return "scoreType"
    if patchSize != 31:
        return "patchSize"
    if not 1 <= fastThreshold <= 254:
        return "fastThreshold"
    return None


def detect(img, nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, scoreType=HARRIS_SCORE, fastThreshold=20,
           pattern=None):
    """-> dict: xy float32 [N,2], aux float32 [N,4] (size, angle, response, octave), desc uint8 [N,32], and `levels`: per level
    a dict of the stages (img / blur with their borders, cand [K,3] (x, y, score) after NMS and the border filter, live (first
    cut), resp float32 [K] (valid where live), keep (second cut), cut1, cut2) - None for a level too small to hold a keypoint."""
    assert check_params(nfeatures, scaleFactor, nlevels, edgeThreshold, 0, 2, scoreType, 31, fastThreshold) is None
    pattern = default_pattern() if pattern is None else np.asarray(pattern, np.int8)
    g = gray(img)
    h, w = g.shape
    b = border(edgeThreshold)
    sizes, scales, quota = level_sizes(w, h, scaleFactor, nlevels), level_scales(scaleFactor, nlevels), quotas(nfeatures, scaleFactor, nlevels)
    umax = umax_table()
    levels, xy, aux, desc = [], [], [], []
    cur = g
    for lv in range(nlevels):
        lw, lh = sizes[lv]
        if lw < 2 * edgeThreshold + 1 or lh < 2 * edgeThreshold + 1:
            levels.append(None)
            continue
        if lv > 0:
            cur = resize_exact(cur, lw, lh)
        P, Pb = pad101(cur, b), pad101(blur(cur), b)
        score = fast_score_map(cur, fastThreshold)
        keep = nms(score)
        keep[:edgeThreshold] = False; keep[lh - edgeThreshold:] = False
        keep[:, :edgeThreshold] = False; keep[:, lw - edgeThreshold:] = False
        ys, xs = np.nonzero(keep)
        sc = score[ys, xs]
        n1 = 2 * quota[lv] if scoreType == HARRIS_SCORE else quota[lv]
        cut1 = int(retain_cut(sc, n1, 256, 0))
        live = sc >= cut1
        Pi = P.astype(np.int64)
        resp = np.zeros(len(xs), np.float32)
        for i in np.nonzero(live)[0]:
            resp[i] = harris_response(*harris_abc(Pi, b, xs[i], ys[i])) if scoreType == HARRIS_SCORE else F32(sc[i])
        key = np.where(live, float_key(resp), 0)
        kcut = int(retain_cut(key[live], quota[lv], 0xFFFFFFFF + 1, 1))
        kept = key >= kcut
        if kcut == 1:
            cut2 = F32(-np.inf)
        elif kcut > 0xFFFFFFFF:
            cut2 = F32(np.inf)
        else:
            cut2 = resp[kept][np.argmin(key[kept])]
        levels.append(dict(w=lw, h=lh, img=P, blur=Pb, cand=np.column_stack([xs, ys, sc]).astype(np.int64), live=live, resp=resp,
                           keep=kept, cut1=cut1, cut2=cut2))
        idx = np.nonzero(kept)[0]
        idx = idx[np.lexsort((xs[idx], ys[idx], -key[idx]))]
        for i in idx:
            m01, m10 = moments(Pi, b, xs[i], ys[i], umax)
            ang = fast_atan2(F32(m01), F32(m10))
            xy.append((F32(xs[i]) * scales[lv], F32(ys[i]) * scales[lv]))
            aux.append((F32(PATCH) * scales[lv], ang, resp[i], F32(lv)))
            desc.append(descriptor(Pb, b, xs[i], ys[i], ang, pattern))
    n = len(xy)
    return dict(xy=np.array(xy, np.float32).reshape(n, 2), aux=np.array(aux, np.float32).reshape(n, 4),
                desc=np.array(desc, np.uint8).reshape(n, 32), levels=levels, sizes=sizes, quotas=quota, border=b)
