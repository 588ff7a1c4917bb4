"""AKAZE as `cv2.AKAZE_create(DESCRIPTOR_MLDB, 0, 3, threshold, nOctaves, nOctaveLayers, DIFF_PM_G2, max_points)
.detectAndCompute(img, None)` computes it for 8-bit images, restated in numpy: the reference of csrc/akaze_kernels.hip and
csrc/akaze_plan.hpp (tests/test_akaze_gpu.py, tests/test_akaze_plan.py).

cv2 is not installed where this project is tested, so everything below is OpenCV 4.x `AKAZEFeatures.cpp`,
`nldiffusion_functions.cpp` and `fed.cpp` RESTATED FROM MEMORY; `UNCONFIRMED` lists what could not be checked against a real
cv2.  Parity with cv2 is unpinned.

THE DEFINED ARITHMETIC: float32, one IEEE operation at a time in the order written here (numpy float32 scalars and arrays round
after every operation); sqrt is correctly rounded; `cos`, `sin`, `pow`, `exp` are the float64 function rounded once;
`fastAtan2` is the polynomial of tests/orb_ref.py; the 2 x 2 solve of the refinement is float64 on the float32 entries, each
offset rounded once.  The kernels equal this file bit for bit.

ORDER-FREE SUMS (stated departures; OpenCV adds in an order that depends on its build):
* the Gaussian and Scharr taps: the order is FIXED - row pass then column pass through a float32 intermediate, taps ascending,
  acc = acc + tap_k px_k (the derivative taps are -1 and +1: the difference p[+s] - p[-s]);
* the orientation windows and the M-LDB cell sums: every float32 contribution is converted to a 64-bit integer at the scale
  2^32 (truncated towards zero), the integers are summed - exact, so no order - and the sum is converted back once;
* the histogram of kcontrast and its maximum are order-free already.

THE DIFFUSION STEP on the borders: the one-sided forms are the interior expression with the missing neighbour replicated,
whose flux is then an exact zero; the sum over the plane is conserved up to rounding.

SUPPRESSION IS A PREDICATE, not a scan: a candidate of level k is dropped iff some candidate of level k - 1, k or k + 1 lies
within its radius (esigma * derivative_factor of ITS level, full-resolution pixels, squared distance <= squared radius) and has
a larger response, or an equal response and a lower (level, row, column).  Not transitive: a dropped candidate still
suppresses.  `detect` counts in `scan_differs` the candidates a scan in level / row / column order decides otherwise.

THE ORDER of the output: class_id (the level's index) ascending, then the candidate's row, then its column.  Ties at the
`max_points` cut are kept.  A frame without a border-free interior at level 0 yields nothing.
"""
import math

import numpy as np

from orb_ref import F32, cv_round, gray, reflect101
from sift_ref import fast_atan2_v

UNCONFIRMED = (
    "BGR2GRAY: (B 3735 + G 19235 + R 9798 + 2^14) >> 15 (the KLT / ORB / SIFT restatement)",
    "the image: uint8 -> float32, divided by 255 in float32 (OpenCV: convertTo with the double scale 1 / 255)",
    "octave i has size (int)(w / 2^i) x (int)(h / 2^i); an octave other than 0 below 80 x 40 ends the pyramid",
    "esigma = soffset 2^(j / nOctaveLayers + i), etime = 0.5 esigma^2, sigma_size = cvRound(esigma derivative_factor / 2^i), all in double",
    "FED: n = (int)(ceil(sqrt(3 T / tau_max + 0.25) - 0.5 - 1e-8) + 0.5), tau_k = (scale tau_max / 2) / cos^2(pi (2k + 1) / (4n + 2)) with "
    "scale = 3 T / (tau_max n (n + 1)), in double rounded to float32 (OpenCV: float32 throughout); the kappa-cycle with kappa = n / 2 "
    "through the next prime >= n + 1",
    "gaussian_2D_convolution: ksize = ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd (9 for 1.6, 5 for 1), getGaussianKernel's taps in double "
    "normalised and rounded to float32, BORDER_REPLICATE, the accumulation order",
    "kcontrast: the image blurred with sigma 1, the UNNORMALISED 3 x 3 Scharr (3, 10, 3), interior pixels only, hmax their largest gradient "
    "magnitude, bin (int)floor(300 (g / hmax)) with 300 -> 299, zeros not counted, nthreshold = (int)(npoints 0.7), k = hmax (bin / 300) of "
    "the first bin at which the running count reaches nthreshold; 0.03 when hmax is 0 or the count is never reached",
    "a new octave: the previous Lt halved by INTER_AREA as the mean of the 2 x 2 block at (2y, 2x), ((a + b) + (c + d)) 0.25 - exact for "
    "even sides; for an odd side the last row / column is dropped (OpenCV's INTER_AREA weights fractions there); kcontrast 0.75",
    "each level: Lsmooth = blur(Lt, sigma 1, 5 x 5), Lx / Ly the unnormalised Scharr of Lsmooth with BORDER_REFLECT_101, "
    "Lflow = 1 / (1 + (Lx^2 + Ly^2) / k^2) (OpenCV multiplies by 1 / k^2)",
    "the diffusion step 0.5 tau (((xpos - xneg) + ypos) - yneg) with replicated neighbours on the borders AND in the corners (OpenCV leaves "
    "the corners to the row and column forms), Lt += Lstep",
    "the response: Lsmooth = blur(Lt, sigma 1) afresh for every level, level 0 included; the scaled Scharr kernels of size 3 + 2 (sigma_size "
    "- 1): w = 10 / 3, norm = 1 / (2 sigma_size (w + 2)), smoothing taps (norm, w norm, norm) at -s, 0, +s, derivative taps (-1, +1), "
    "BORDER_REFLECT_101; Lx, Ly are NOT multiplied by sigma_size; Ldet = (Lxx Lyy - Lxy Lxy) sigma_size^4",
    "candidates: Ldet > threshold and strictly above its 8 neighbours, inside border = 2 sigma_size + 1 (where Ldet and its neighbours "
    "reach no reflected pixel; OpenCV's border is larger and derived from the descriptor's reach)",
    "suppression: the radius esigma derivative_factor of the candidate's level, squared distance <= squared radius, levels k - 1, k, k + 1",
    "refinement: Dx, Dy = 0.5 (difference), Dxx = (a + b) - 2 c, Dxy = 0.25 (pp + mm) - 0.25 (mp + pm), the 2 x 2 system solved by Cramer's rule "
    "in double (a zero determinant rejects), accepted when both |offsets| <= 1; pt = (x + dx) 2^octave + 0.5 (2^octave - 1), "
    "size = 2 esigma derivative_factor, response = Ldet, octave, class_id = the level's index",
    "retainBest(max_points) on the response before the orientation, everything >= the n-th largest kept",
    "orientation: s = cvRound(0.5 size / 2^octave), the 109 samples i^2 + j^2 < 36 at (cvRound(xf + i s), cvRound(yf + j s)), samples outside "
    "the level skipped (OpenCV has no such sample), gauss25[id[i + 6]][id[j + 6]], 42 windows at 0.15 rad steps of width pi / 3, a sample "
    "strictly inside its window, the first largest sumX^2 + sumY^2 wins, angle = fastAtan2(sumY, sumX) in degrees; no sample: 0",
    "M-LDB: pattern 10, grids 2 x 2 / 3 x 3 / 4 x 4 with steps 10 / 7 / 5 from -10 (the 3 x 3 grid reaches 10), sample (l, k) at "
    "yf + ((l co) scale + (k si) scale), xf + ((-l si) scale + (k co) scale) rounded by cvRound, samples outside the level skipped, channels Lt, "
    "rrx = -rx si + ry co, rry = rx co + ry si, the cell's mean over its inside samples (0 for none), bits per grid: channel, then pairs "
    "i < j set when v_i > v_j, bit b in byte b >> 3 at 1 << (b & 7)",
)

DESCRIPTOR_MLDB, DIFF_PM_G2 = 5, 1
SOFFSET, DERIVATIVE_FACTOR, SDERIVATIVES, KCONTRAST_PERCENTILE, KCONTRAST_NBINS, TAU_MAX = 1.6, 1.5, 1.0, 0.7, 300, 0.25
MAX_OCTAVES = MAX_SUBLEVELS = 8
MIN_OCTAVE_W, MIN_OCTAVE_H = 80, 40
DESC_BYTES, DESC_BITS = 61, 486
FIXED_LOG2 = 32
WG_PIXELS = 20000                  # a level of at most this many pixels runs its diffusion in one workgroup (the plan's constant)
DEG2RAD = F32(math.pi / 180)
N_WINDOWS = 42
GAUSS25 = np.array([
    [0.02546481, 0.02350698, 0.01849125, 0.01239505, 0.00708017, 0.00344629, 0.00142946],
    [0.02350698, 0.02169968, 0.01706957, 0.01144208, 0.00653582, 0.00318132, 0.00131956],
    [0.01849125, 0.01706957, 0.01342740, 0.00900066, 0.00514126, 0.00250252, 0.00103800],
    [0.01239505, 0.01144208, 0.00900066, 0.00603332, 0.00344629, 0.00167749, 0.00069579],
    [0.00708017, 0.00653582, 0.00514126, 0.00344629, 0.00196855, 0.00095820, 0.00039744],
    [0.00344629, 0.00318132, 0.00250252, 0.00167749, 0.00095820, 0.00046640, 0.00019346],
    [0.00142946, 0.00131956, 0.00103800, 0.00069579, 0.00039744, 0.00019346, 0.00008024]], np.float64).astype(np.float32)
GRIDS = ((2, 10), (3, 7), (4, 5))  # cells per side, sample step


# ---- parameters and the plan's numbers ------------------------------------------------------------------------------------
def check_params(descriptor_type=DESCRIPTOR_MLDB, descriptor_size=0, descriptor_channels=3, threshold=0.001, nOctaves=4, nOctaveLayers=4,
                 diffusivity=DIFF_PM_G2, max_points=-1):
    """-> the word of the refusal, or None"""
    if descriptor_type != DESCRIPTOR_MLDB:
        return "descriptor_type"
    if descriptor_size != 0:
        return "descriptor_size"
    if descriptor_channels != 3:
        return "descriptor_channels"
    if not (threshold > 0 and math.isfinite(threshold)):
        return "threshold"
    if not 1 <= nOctaves <= MAX_OCTAVES:
        return "nOctaves"
    if not 1 <= nOctaveLayers <= MAX_SUBLEVELS:
        return "nOctaveLayers"
    if diffusivity != DIFF_PM_G2:
        return "diffusivity"
    if not (max_points == -1 or max_points >= 1):
        return "max_points"
    return None


def levels(w, h, nOctaves=4, nOctaveLayers=4):
    """-> list of dict(octave, sublevel, w, h, esigma, etime, sigma_size, border, size, radius) - size / radius float32"""
    out = []
    for i in range(nOctaves):
        lw, lh = w >> i, h >> i
        if i > 0 and (lw < MIN_OCTAVE_W or lh < MIN_OCTAVE_H):
            break
        for j in range(nOctaveLayers):
            esigma = SOFFSET * math.pow(2.0, j / nOctaveLayers + i)
            s = cv_round(esigma * DERIVATIVE_FACTOR / (1 << i))
            out.append(dict(octave=i, sublevel=j, w=lw, h=lh, esigma=esigma, etime=0.5 * (esigma * esigma), sigma_size=s, border=2 * s + 1,
                            size=F32(2.0 * esigma * DERIVATIVE_FACTOR), radius=F32(esigma * DERIVATIVE_FACTOR)))
    return out


def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(math.isqrt(n)) + 1))


def fed_unordered(T):
    n = int(math.ceil(math.sqrt(3.0 * T / TAU_MAX + 0.25) - 0.5 - 1.0e-8) + 0.5)
    scale = 3.0 * T / (TAU_MAX * (n * (n + 1)))
    c, d = 1.0 / (4.0 * n + 2.0), scale * TAU_MAX / 2.0
    out = []
    for k in range(n):
        cs = math.cos(math.pi * (2.0 * k + 1.0) * c)
        out.append(d / (cs * cs))
    return np.array(out, np.float64).astype(np.float32)


def fed_steps(T):
    """the step sizes of one transition in the order they are taken (the kappa-cycle)"""
    tauh = fed_unordered(T)
    n = len(tauh)
    kappa, prime = n // 2, n + 1
    while not _is_prime(prime):
        prime += 1
    out, k = [], 0
    for _ in range(n):
        index = ((k + 1) * kappa) % prime - 1
        while index >= n:
            k += 1
            index = ((k + 1) * kappa) % prime - 1
        out.append(tauh[index])
        k += 1
    return np.array(out, np.float32)


def gauss_taps(sigma):
    n = int(math.ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3)))
    n += 1 - n % 2
    s2 = -0.5 / (sigma * sigma)
    t = [math.exp(s2 * (i - (n - 1) * 0.5) ** 2) for i in range(n)]
    total = 0.0
    for v in t:
        total += v
    inv = 1.0 / total
    return np.array([v * inv for v in t], np.float64).astype(np.float32)


def scharr_taps(s):
    """(norm, w norm) of the scaled Scharr kernel, float32"""
    w = 10.0 / 3.0
    norm = 1.0 / (2.0 * s * (w + 2.0))
    return F32(norm), F32(w * norm)


# ---- the filters -------------------------------------------------------------------------------------------------------
def blur(img, taps):
    """row pass then column pass, acc = acc + tap_k px_k for k ascending, BORDER_REPLICATE"""
    h, w = img.shape
    r = len(taps) // 2
    ix = np.clip(np.arange(-r, w + r), 0, w - 1)
    acc = np.zeros((h, w), np.float32)
    for k in range(len(taps)):
        acc = acc + taps[k] * img[:, ix[k:k + w]]
    iy = np.clip(np.arange(-r, h + r), 0, h - 1)
    out = np.zeros((h, w), np.float32)
    for k in range(len(taps)):
        out = out + taps[k] * acc[iy[k:k + h]]
    return out


def deriv(src, s, a, b, axis):
    """the separable Scharr form at reach s with smoothing taps (a, b, a), BORDER_REFLECT_101: axis 'x' differentiates along x
    (row pass) and smooths along y (column pass); axis 'y' smooths along x and differentiates along y"""
    h, w = src.shape
    xm, xp = reflect101(np.arange(w) - s, w), reflect101(np.arange(w) + s, w)
    ym, yp = reflect101(np.arange(h) - s, h), reflect101(np.arange(h) + s, h)
    if axis == "x":
        d = src[:, xp] - src[:, xm]
        out = a * d[ym]
        out = out + b * d
        return out + a * d[yp]
    sm = a * src[:, xm]
    sm = sm + b * src
    sm = sm + a * src[:, xp]
    return sm[yp] - sm[ym]


def halve(src, w, h):
    a, b, c, d = src[0:2 * h:2, 0:2 * w:2], src[0:2 * h:2, 1:2 * w:2], src[1:2 * h:2, 0:2 * w:2], src[1:2 * h:2, 1:2 * w:2]
    return ((a + b) + (c + d)) * F32(0.25)


def kcontrast(img01):
    """the 70th percentile of the gradient magnitude -> (k float32, hmax, npoints)"""
    sm = blur(img01, gauss_taps(1.0))
    lx, ly = deriv(sm, 1, F32(3), F32(10), "x")[1:-1, 1:-1], deriv(sm, 1, F32(3), F32(10), "y")[1:-1, 1:-1]
    g = np.sqrt(lx * lx + ly * ly).ravel()
    hmax = g.max() if g.size else F32(0)
    if hmax == 0:
        return F32(0.03), F32(0), 0
    nz = g[g != 0]
    bins = np.floor(F32(KCONTRAST_NBINS) * (nz / hmax)).astype(np.int64)
    bins = np.minimum(bins, KCONTRAST_NBINS - 1)
    hist = np.bincount(bins, minlength=KCONTRAST_NBINS)
    nthreshold = int(len(nz) * KCONTRAST_PERCENTILE)
    nelements, k = 0, 0
    while nelements < nthreshold and k < KCONTRAST_NBINS:
        nelements += int(hist[k])
        k += 1
    if nelements < nthreshold:
        return F32(0.03), hmax, len(nz)
    return hmax * (F32(k) / F32(KCONTRAST_NBINS)), hmax, len(nz)


def flow(lt, k):
    sm = blur(lt, gauss_taps(1.0))
    lx, ly = deriv(sm, 1, F32(3), F32(10), "x"), deriv(sm, 1, F32(3), F32(10), "y")
    return F32(1) / (F32(1) + (lx * lx + ly * ly) / (k * k))


def nld_step(L, c, tau):
    h, w = L.shape
    xm, xp = np.maximum(np.arange(w) - 1, 0), np.minimum(np.arange(w) + 1, w - 1)
    ym, yp = np.maximum(np.arange(h) - 1, 0), np.minimum(np.arange(h) + 1, h - 1)
    xpos = (c + c[:, xp]) * (L[:, xp] - L)
    xneg = (c[:, xm] + c) * (L - L[:, xm])
    ypos = (c + c[yp]) * (L[yp] - L)
    yneg = (c[ym] + c) * (L - L[ym])
    return L + (F32(0.5) * F32(tau)) * (((xpos - xneg) + ypos) - yneg)


def scale_space(g, nOctaves=4, nOctaveLayers=4):
    """grey uint8 -> (levels, planes per level: dict(Lt, Lflow (None at level 0), Lx, Ly, Ldet), kcontrast per octave)"""
    h, w = g.shape
    lv = levels(w, h, nOctaves, nOctaveLayers)
    img = g.astype(np.float32) / F32(255)
    k0, _, _ = kcontrast(img)
    ks, planes = [k0], []
    t1 = gauss_taps(1.0)
    for i, L in enumerate(lv):
        if i == 0:
            lt, fl = blur(img, gauss_taps(SOFFSET)), None
        else:
            lt = planes[-1]["Lt"]
            if L["octave"] != lv[i - 1]["octave"]:
                lt = halve(lt, L["w"], L["h"])
                ks.append(ks[-1] * F32(0.75))
            fl = flow(lt, ks[-1])
            for tau in fed_steps(L["etime"] - lv[i - 1]["etime"]):
                lt = nld_step(lt, fl, tau)
        s = L["sigma_size"]
        a, b = scharr_taps(s)
        sm = blur(lt, t1)
        lx, ly = deriv(sm, s, a, b, "x"), deriv(sm, s, a, b, "y")
        lxx, lxy, lyy = deriv(lx, s, a, b, "x"), deriv(lx, s, a, b, "y"), deriv(ly, s, a, b, "y")
        planes.append(dict(Lt=lt, Lflow=fl, Lx=lx, Ly=ly, Ldet=(lxx * lyy - lxy * lxy) * F32(s ** 4)))
    return lv, planes, ks


# ---- candidates, suppression, refinement -------------------------------------------------------------------------------
def candidates(lv, planes, threshold):
    """-> list of (level, r, c, response float32) in level / row / column order"""
    out = []
    for i, (L, P) in enumerate(zip(lv, planes)):
        b, D = L["border"], P["Ldet"]
        h, w = D.shape
        if h <= 2 * b or w <= 2 * b:
            continue
        v = D[b:h - b, b:w - b]
        ok = v > F32(threshold)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    ok &= v > D[b + dy:h - b + dy, b + dx:w - b + dx]
        ys, xs = np.nonzero(ok)
        out += [(i, y + b, x + b, v[y, x]) for y, x in zip(ys.tolist(), xs.tolist())]
    return out


def _full_res(lv, cand):
    lvl = np.array([c[0] for c in cand], np.int64)
    ratio = np.array([F32(1 << lv[l]["octave"]) for l in lvl], np.float32)
    half = np.array([F32(0.5 * ((1 << lv[l]["octave"]) - 1)) for l in lvl], np.float32)
    px = np.array([c[2] for c in cand], np.float32) * ratio + half
    py = np.array([c[1] for c in cand], np.float32) * ratio + half
    rad = np.array([lv[l]["radius"] for l in lvl], np.float32)
    resp = np.array([c[3] for c in cand], np.float32)
    return lvl, px, py, rad, resp


def suppress(lv, cand):
    """-> bool [K] survives, int [K] kind of the first suppressor found (0 none, 1 same level, 2 adjacent level)"""
    n = len(cand)
    if n == 0:
        return np.zeros(0, bool), np.zeros(0, np.int64)
    lvl, px, py, rad, resp = _full_res(lv, cand)
    dx, dy = px[None, :] - px[:, None], py[None, :] - py[:, None]
    near = (dx * dx + dy * dy) <= (rad * rad)[:, None]
    idx = np.arange(n)
    beats = (resp[None, :] > resp[:, None]) | ((resp[None, :] == resp[:, None]) & (idx[None, :] < idx[:, None]))
    adj = np.abs(lvl[None, :] - lvl[:, None]) <= 1
    hit = near & beats & adj & (idx[None, :] != idx[:, None])
    same = (hit & (lvl[None, :] == lvl[:, None])).any(1)
    cross = (hit & (lvl[None, :] != lvl[:, None])).any(1)
    return ~hit.any(1), np.where(same, 1, np.where(cross, 2, 0))


def scan_survivors(lv, cand):
    """what a scan in level / row / column order keeps (the shape of OpenCV's loop): a candidate meets the kept ones of its own
    and the previous level - the first within its radius decides: the stronger of the two stays - and afterwards a kept one is
    dropped when a kept one of the next level within its radius is stronger"""
    if not cand:
        return set()
    lvl, px, py, rad, resp = _full_res(lv, cand)
    kept = []
    for i in range(len(cand)):
        decided = False
        for pos, j in enumerate(kept):
            if lvl[i] - lvl[j] in (0, 1):
                dx, dy = px[j] - px[i], py[j] - py[i]
                if dx * dx + dy * dy <= rad[i] * rad[i]:
                    if resp[i] > resp[j]:
                        kept[pos] = i
                    decided = True
                    break
        if not decided:
            kept.append(i)
    out = set()
    for i in kept:
        drop = False
        for j in kept:
            if lvl[j] == lvl[i] + 1:
                dx, dy = px[j] - px[i], py[j] - py[i]
                if dx * dx + dy * dy <= rad[i] * rad[i] and resp[j] > resp[i]:
                    drop = True
        if not drop:
            out.add(i)
    return out


def refine(lv, planes, c):
    """-> None, or dict(x, y, size, response, octave, class_id, level, r, c, dx, dy, angle=0)"""
    lvl, r, x, resp = c
    L = planes[lvl]["Ldet"]
    Dx = F32(0.5) * (L[r, x + 1] - L[r, x - 1])
    Dy = F32(0.5) * (L[r + 1, x] - L[r - 1, x])
    Dxx = (L[r, x + 1] + L[r, x - 1]) - F32(2) * L[r, x]
    Dyy = (L[r + 1, x] + L[r - 1, x]) - F32(2) * L[r, x]
    Dxy = F32(0.25) * (L[r + 1, x + 1] + L[r - 1, x - 1]) - F32(0.25) * (L[r - 1, x + 1] + L[r + 1, x - 1])
    a00, a01, a11, b0, b1 = float(Dxx), float(Dxy), float(Dyy), -float(Dx), -float(Dy)
    det = a00 * a11 - a01 * a01
    if det == 0:
        return None
    d = 1.0 / det
    dx, dy = F32((b0 * a11 - b1 * a01) * d), F32((b1 * a00 - b0 * a01) * d)
    if not (abs(dx) <= 1 and abs(dy) <= 1):
        return None
    o = lv[lvl]["octave"]
    ratio, half = F32(1 << o), F32(0.5 * ((1 << o) - 1))
    return dict(x=(F32(x) + dx) * ratio + half, y=(F32(r) + dy) * ratio + half, size=lv[lvl]["size"], response=resp, octave=o, class_id=lvl,
                level=lvl, r=r, c=x, dx=dx, dy=dy, angle=F32(0))


# ---- the orientation and the descriptor ------------------------------------------------------------------------------------
def to_fixed(v):
    """float32 -> int64 at 2^32, truncated towards zero"""
    return np.trunc(np.asarray(v, np.float32).astype(np.float64) * float(1 << FIXED_LOG2)).astype(np.int64)


def from_fixed(s):
    return (np.asarray(s, np.int64).astype(np.float64) / float(1 << FIXED_LOG2)).astype(np.float32)


def _round_v(v):
    return np.rint(v).astype(np.int64)


PI3, TWO_PI, FIVE_PI3 = F32(math.pi / 3), F32(2 * math.pi), F32(5 * math.pi / 3)


def orientation(lv, planes, k):
    """-> float32 degrees"""
    L, P = lv[k["level"]], planes[k["level"]]
    ratio = F32(1 << L["octave"])
    xf, yf = k["x"] / ratio, k["y"] / ratio
    s = cv_round(F32(0.5) * k["size"] / ratio)
    i, j = np.mgrid[-6:7, -6:7]
    i, j = i.ravel(), j.ravel()
    keep = i * i + j * j < 36
    i, j = i[keep], j[keep]
    iy, ix = _round_v(yf + (j * s).astype(np.float32)), _round_v(xf + (i * s).astype(np.float32))
    ok = (iy >= 0) & (iy < L["h"]) & (ix >= 0) & (ix < L["w"])
    i, j, iy, ix = i[ok], j[ok], iy[ok], ix[ok]
    gw = GAUSS25[np.abs(i), np.abs(j)]
    rx, ry = gw * P["Lx"][iy, ix], gw * P["Ly"][iy, ix]
    ang = fast_atan2_v(ry, rx) * DEG2RAD
    fx, fy = to_fixed(rx), to_fixed(ry)
    best, angle = F32(0), F32(0)
    for w in range(N_WINDOWS):
        a1 = F32(0.15) * F32(w)
        a2 = a1 + PI3
        if a2 > TWO_PI:
            a2 = a1 - FIVE_PI3
        if a1 < a2:
            m = (a1 < ang) & (ang < a2)
        else:
            m = ((ang > 0) & (ang < a2)) | ((ang > a1) & (ang < TWO_PI))
        sx, sy = from_fixed(fx[m].sum()), from_fixed(fy[m].sum())
        v = sx * sx + sy * sy
        if v > best:
            best, angle = v, fast_atan2_v(sy, sx)[()]
    return F32(angle)


def mldb_values(lv, planes, k, stats=None):
    """-> per grid float32 [cells, 3] (the means of Lt, rrx, rry)"""
    L, P = lv[k["level"]], planes[k["level"]]
    ratio = F32(1 << L["octave"])
    xf, yf = k["x"] / ratio, k["y"] / ratio
    scale = F32(cv_round(F32(0.5) * k["size"] / ratio))
    rad = k["angle"] * DEG2RAD
    co, si = F32(math.cos(float(rad))), F32(math.sin(float(rad)))
    out = []
    for cells, step in GRIDS:
        kk, ll = np.mgrid[0:cells * step, 0:cells * step]          # cell (k // step, l // step), sample (k - 10, l - 10)
        kk, ll = kk.ravel(), ll.ravel()
        cell = (kk // step) * cells + ll // step
        fk, fl = (kk - 10).astype(np.float32), (ll - 10).astype(np.float32)
        sy = yf + ((fl * co) * scale + (fk * si) * scale)
        sx = xf + (((-fl) * si) * scale + (fk * co) * scale)
        y1, x1 = _round_v(sy), _round_v(sx)
        ok = (y1 >= 0) & (y1 < L["h"]) & (x1 >= 0) & (x1 < L["w"])
        if stats is not None:
            stats["outside"] = stats.get("outside", 0) + int((~ok).sum())
        y1, x1, cell = y1[ok], x1[ok], cell[ok]
        ri, rx, ry = P["Lt"][y1, x1], P["Lx"][y1, x1], P["Ly"][y1, x1]
        rry = rx * co + ry * si
        rrx = (-rx) * si + ry * co
        sums, cnt = np.zeros((cells * cells, 3), np.int64), np.bincount(cell, minlength=cells * cells)
        for ch, v in enumerate((ri, rrx, rry)):
            np.add.at(sums[:, ch], cell, to_fixed(v))
        vals = np.zeros((cells * cells, 3), np.float32)
        has = cnt > 0
        vals[has] = from_fixed(sums[has]) / cnt[has].astype(np.float32)[:, None]
        out.append(vals)
    return out


def bit_layout():
    """-> list of (grid, channel, i, j) per bit, 486 long"""
    return [(g, ch, i, j) for g, (cells, _) in enumerate(GRIDS) for ch in range(3) for i in range(cells * cells) for j in range(i + 1, cells * cells)]


def mldb_bits(values):
    desc = np.zeros(DESC_BYTES, np.uint8)
    for b, (g, ch, i, j) in enumerate(bit_layout()):
        if values[g][i, ch] > values[g][j, ch]:
            desc[b >> 3] |= 1 << (b & 7)
    return desc


# ---- the whole detector ---------------------------------------------------------------------------------------------------
def detect(img, descriptor_type=DESCRIPTOR_MLDB, descriptor_size=0, descriptor_channels=3, threshold=0.001, nOctaves=4, nOctaveLayers=4,
           diffusivity=DIFF_PM_G2, max_points=-1):
    """-> dict: xy float32 [N,2], aux float32 [N,3] (size, angle, response), lvl int32 [N,2] (octave, class_id), desc uint8 [N,61],
    and the stages: levels, planes, kcontrast, cand, survives, kind, refined (per candidate, None: dropped or rejected), kept,
    scan_differs, outside (descriptor samples that fell outside their level)"""
    assert check_params(descriptor_type, descriptor_size, descriptor_channels, threshold, nOctaves, nOctaveLayers, diffusivity, max_points) is None
    g = gray(img)
    h, w = g.shape
    lv0 = levels(w, h, nOctaves, nOctaveLayers)
    empty = dict(xy=np.zeros((0, 2), np.float32), aux=np.zeros((0, 3), np.float32), lvl=np.zeros((0, 2), np.int32),
                 desc=np.zeros((0, DESC_BYTES), np.uint8), levels=lv0, planes=[], kcontrast=[], cand=[], survives=np.zeros(0, bool),
                 kind=np.zeros(0, np.int64), refined=[], kept=[], scan_differs=0, outside=0, n_refined=0)
    if h <= 2 * lv0[0]["border"] or w <= 2 * lv0[0]["border"]:
        return empty
    lv, planes, ks = scale_space(g, nOctaves, nOctaveLayers)
    cand = candidates(lv, planes, threshold)
    survives, kind = suppress(lv, cand)
    scan = scan_survivors(lv, cand)
    refined = [refine(lv, planes, c) if s else None for c, s in zip(cand, survives)]
    good = [k for k in refined if k is not None]
    if max_points > 0 and len(good) > max_points:
        cut = sorted((k["response"] for k in good), reverse=True)[max_points - 1]
        good = [k for k in good if k["response"] >= cut]
    stats = {}
    xy, aux, lvl, desc = [], [], [], []
    for k in good:                                                 # (already in level / row / column order)
        k["angle"] = orientation(lv, planes, k)
        k["kept"] = True
        desc.append(mldb_bits(mldb_values(lv, planes, k, stats)))
        xy.append((k["x"], k["y"]))
        aux.append((k["size"], k["angle"], k["response"]))
        lvl.append((k["octave"], k["class_id"]))
    n = len(xy)
    return dict(xy=np.array(xy, np.float32).reshape(n, 2), aux=np.array(aux, np.float32).reshape(n, 3), lvl=np.array(lvl, np.int32).reshape(n, 2),
                desc=np.array(desc, np.uint8).reshape(n, DESC_BYTES), levels=lv, planes=planes, kcontrast=ks, cand=cand, survives=survives,
                kind=kind, refined=refined, kept=good, scan_differs=len(scan ^ set(np.nonzero(survives)[0].tolist())),
                outside=stats.get("outside", 0), n_refined=sum(k is not None for k in refined))
