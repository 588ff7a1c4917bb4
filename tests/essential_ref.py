"""CPU reference (numpy, float64) of `sslam_essential_ransac_host`: OpenCV 4.x's classic (non-USAC)
`findEssentialMat(points1, points2, cameraMatrix, RANSAC, prob, threshold, maxIters = 1000, mask)` restated, sequentially:
the ptsetreg.cpp loop around Nister's five-point solver (EMEstimatorCallback of five-point.cpp).

`linalg` picks how the four small dense problems of the solver are done: "lapack" (`np.linalg.svd` for the null space of
the 5 x 9 epipolar matrix and of the 3 x 3 matrix at a root, `np.linalg.solve` for the 10 x 10 elimination, `np.roots`)
or "port", float64 ports of exactly what the kernel runs (csrc/essential_kernels.hip) - a one-sided Jacobi on the five
rows completed to a basis the way OpenCV's JacobiSVD completes one, Gauss-Jordan with partial pivoting, a Durand-Kerner
iteration in real arithmetic, a cross product - with separate multiplies and adds in the order the kernel has them.  Both
variants share the polynomial bookkeeping (the ten cubic constraints, the determinant in z), which has no choice in it.
The two span the null space by DIFFERENT bases, so the models of one sample come in another order and with other
rounding, not as another set; the roots are the same whatever finds them.  What the two disagree by is the measured floor
of the GPU tolerance (tests/test_essential_ref.py, tests/test_essential_gpu.py).

PARITY UNPINNED: the cv2 wheel and OpenCV's sources are absent from the build image.  Restated from memory of
modules/calib3d/src/five-point.cpp (findEssentialMat, EMEstimatorCallback::{runKernel, computeError}), ptsetreg.cpp
(RANSACPointSetRegistrator::run, getSubset) and modules/core (JacobiSVDImpl_, solvePoly).  What could NOT be confirmed
against a real cv2 here:
  * the null-space basis: OpenCV takes the last four rows of Vt of `SVD::compute(A, FULL_UV)`.  Its own JacobiSVD fills
    the rows a 5 x 9 matrix leaves open with +-1/9 vectors from cv::RNG(0x12345678) (`next() & 256` picks the sign), made
    orthogonal to the rows before them in two Gram-Schmidt passes with an L1 rescale after every projection - that is
    what "port" restates; a cv2 built on LAPACK returns dgesdd's basis instead ("lapack" here);
  * `getCoeffMat`: OpenCV's ten rows are generated code; here they are det E and the nine entries of
    (E E' - tr(E E') / 2) E, columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.  The
    rows span the same ideal; their order and scale reach the result only through the pivoting's rounding;
  * the elimination: OpenCV solves the left 10 x 10 block with `solve` (LU); Gauss-Jordan with partial pivoting here;
  * `solvePoly`: remembered as Durand-Kerner from the start values (1 + i)^k with IN-PLACE updates, at most 300
    iterations, stopping on a largest step of zero or below an epsilon.  The port updates all ten roots at once (so
    that it vectorises) from the same start values, at most 300 iterations, and stops once every step is within
    1e-14 (1 + |re| + |im|) of its root; a leading coefficient of zero or a non-finite value gives no model, where
    solvePoly would lower the degree;
  * the two 1e-10 tests: a root is kept when |imag| < 1e-10; it is skipped when the last entry of the unit null vector
    of the 3 x 3 matrix at the root is below 1e-10 in magnitude.  OpenCV finds that vector by an SVD, the port by the
    largest cross product of two rows;
  * whether E is normalised: it is here, each model divided by its Frobenius norm;
  * the order of the models: the order of the kept roots in the root finder's output.
"""
import numpy as np

from oracle.ransac_ref import CvRNG, DBL_MIN, update_num_iters

MODEL_POINTS = 5
MAX_ITERS = 2000                      # the entry's clamp on max_iters
DEFAULT_ITERS = 1000
N_MAX = 16384
JACOBI_SWEEPS = 30
POLY_ITERS = 300
POLY_TOL = 1e-14
MAX_MODELS = 10

# ---- monomial tables (exponents of x, y, z) ----------------------------------------------------------------------------
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 2, 0), (0, 1, 1), (0, 1, 0), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
CUBIC = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return tuple(p + q for p, q in zip(a, b))


T12 = np.array([[QUAD.index(_add(a, b)) for b in LIN] for a in LIN])          # linear x linear -> quadratic
T23 = np.array([[CUBIC.index(_add(q, a)) for a in LIN] for q in QUAD])        # quadratic x linear -> cubic


# ---- the polynomial bookkeeping both variants share --------------------------------------------------------------------
def coeff_matrix(ee):
    """ee [4, 9]: the null-space basis, E = x ee[0] + y ee[1] + z ee[2] + ee[3].  Returns the 10 x 20 matrix of the ten
    cubic constraints.  Every sum runs in the order the kernel has it: a target's terms are added one after another, k
    outermost, then the first factor's monomial, then the second's (np.add.at adds unbuffered, in index order)."""
    L = np.ascontiguousarray(ee.reshape(4, 3, 3).transpose(1, 2, 0))            # [r, c, monomial x y z 1]
    # E E' (quadratic): [r, c, k, i, j] -> target (r, c, T12[i, j])
    prod = L[:, None, :, :, None] * L[None, :, :, None, :]
    EEt = np.zeros((3, 3, 10))
    r, c, k, i, j = np.indices((3, 3, 3, 4, 4))
    np.add.at(EEt, (r.ravel(), c.ravel(), T12[i, j].ravel()), prod.ravel())
    tr = (EEt[0, 0] + EEt[1, 1]) + EEt[2, 2]
    Lam = EEt.copy()
    for d in range(3):
        Lam[d, d] = EEt[d, d] - 0.5 * tr
    # (E E' - tr / 2) E (cubic): [r, c, k, q, i] -> target (r, c, T23[q, i])
    LamT = Lam                                                                   # [r, k, q]
    prod = LamT[:, None, :, :, None] * L.transpose(1, 0, 2)[None, :, :, None, :]  # Lam[r, k, q] * L[k, c, i]
    C = np.zeros((3, 3, 20))
    r, c, k, q, i = np.indices((3, 3, 3, 10, 4))
    np.add.at(C, (r.ravel(), c.ravel(), T23[q, i].ravel()), prod.ravel())
    # det E = sum_c E[0, c] * minor_c; minor_c = E[1, c1] E[2, c2] - E[1, c2] E[2, c1], (c1, c2) = (c + 1, c + 2) mod 3
    M = np.zeros((3, 10))
    for cc in range(3):
        c1, c2 = (cc + 1) % 3, (cc + 2) % 3
        vals = np.stack([L[1, c1][:, None] * L[2, c2][None, :], -(L[1, c2][:, None] * L[2, c1][None, :])], -1)
        np.add.at(M[cc], np.repeat(T12.ravel(), 2), vals.ravel())
    D = np.zeros(20)
    prod = M[:, :, None] * L[0][:, None, :]                                      # [c, q, i]
    np.add.at(D, np.broadcast_to(T23, (3, 10, 4)).ravel(), prod.ravel())
    return np.vstack([D[None], C.reshape(9, 20)])


def _conv(a, b):
    """polynomial product, coefficients ascending: out[i + j] += a[i] b[j], i outermost"""
    out = np.zeros(len(a) + len(b) - 1)
    i, j = np.indices((len(a), len(b)))
    np.add.at(out, (i + j).ravel(), (a[:, None] * b[None, :]).ravel())
    return out


def z_polynomials(R):
    """R [10, 10]: the right block after the elimination (row r: its leading monomial + R[r] . right monomials = 0).
    Returns B [3, 3] of polynomials in z (ascending coefficients; the columns multiply x, y, 1) from the row pairs
    (x^2z, x^2), (y^2z, y^2), (xyz, xy), and the determinant (11 ascending coefficients)."""
    B = []
    for a, b in ((4, 5), (6, 7), (8, 9)):
        e, f = R[a], R[b]
        row = []
        for o in (0, 3):
            row.append(np.array([e[o + 2], e[o + 1] - f[o + 2], e[o] - f[o + 1], -f[o]]))
        row.append(np.array([e[9], e[8] - f[9], e[7] - f[8], e[6] - f[7], -f[6]]))
        B.append(row)
    (kx, ky, k1), (lx, ly, l1), (mx, my, m1) = B
    cx = _conv(ky, l1) - _conv(k1, ly)
    cy = _conv(k1, lx) - _conv(kx, l1)
    c1 = _conv(kx, ly) - _conv(ky, lx)
    det = (_conv(mx, cx) + _conv(my, cy)) + _conv(m1, c1)
    return B, det


def _horner(p, z):
    v = p[-1]
    for k in range(len(p) - 2, -1, -1):
        v = v * z + p[k]
    return v


# ---- the four dense problems, "port": what the kernel runs -------------------------------------------------------------
def null_space_port(A):
    """A [5, 9].  One-sided Jacobi on the five rows (pairs (i, j), i < j; a pair is left alone when
    |p| <= 10 eps sqrt(a b); at most 30 sweeps; every dot product summed from entry 0 up), the rows scaled to unit length;
    then rows 5..8 the way OpenCV's JacobiSVD fills them (module docstring).  Returns the four filled rows [4, 9]."""
    V = np.zeros((9, 9))
    V[:5] = A
    eps = np.finfo(np.float64).eps * 10
    for _ in range(JACOBI_SWEEPS):
        changed = False
        for i in range(4):
            for j in range(i + 1, 5):
                ai, aj = V[i].copy(), V[j].copy()
                pr = np.stack([ai * ai, aj * aj, ai * aj])
                s3 = pr[:, 0]
                for k in range(1, 9):
                    s3 = s3 + pr[:, k]
                a, b, p = float(s3[0]), float(s3[1]), float(s3[2])
                if abs(p) <= eps * np.sqrt(a * b):
                    continue
                changed = True
                p *= 2
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)
                if beta < 0:
                    s = np.sqrt((gamma - beta) * 0.5 / gamma)
                    c = p / (gamma * s * 2)
                else:
                    c = np.sqrt((gamma + beta) / (gamma * 2))
                    s = p / (gamma * c * 2)
                V[i] = c * ai + s * aj
                V[j] = c * aj - s * ai
        if not changed:
            break
    rng = CvRNG(0x12345678)
    for i in range(9):
        sd = 0.0
        if i < 5:
            sq = V[i] * V[i]
            for k in range(9):
                sd = sd + float(sq[k])
            sd = float(np.sqrt(sd))
        tries = 0
        while tries < 100 and sd <= DBL_MIN:
            tries += 1
            V[i] = [(1.0 / 9) if (rng.next() & 256) != 0 else -(1.0 / 9) for _k in range(9)]
            for _pass in range(2):
                for j in range(i):
                    pr = V[i] * V[j]
                    d = 0.0
                    for k in range(9):
                        d = d + float(pr[k])
                    V[i] = V[i] - d * V[j]
                    ab = np.abs(V[i])
                    asum = 0.0
                    for k in range(9):
                        asum = asum + float(ab[k])
                    asum = 1.0 / asum if asum > eps * 100 else 0.0
                    V[i] = V[i] * asum
            sq = V[i] * V[i]
            sd = 0.0
            for k in range(9):
                sd = sd + float(sq[k])
            sd = float(np.sqrt(sd))
        V[i] = V[i] * (1.0 / sd if sd > DBL_MIN else 0.0)
    return V[5:].copy()


def eliminate_port(M):
    """Gauss-Jordan with partial pivoting (the first of equal pivots) on the 10 x 20 M; the right block, or None"""
    M = np.array(M, np.float64)
    for k in range(10):
        piv = k + int(np.argmax(np.abs(M[k:, k])))
        pv = M[piv, k]
        if pv == 0 or not np.isfinite(pv):
            return None
        if piv != k:
            M[[k, piv]] = M[[piv, k]]
        M[k, k:] = M[k, k:] / pv
        f = M[:, k].copy()
        f[k] = 0.0
        M[:, k:] = M[:, k:] - f[:, None] * M[k, k:][None, :]
    return M[:, 10:].copy()


def roots_port(det):
    """The real roots of the tenth-degree polynomial (ascending coefficients), in the order of the iteration's slots:
    Durand-Kerner, all ten roots updated at once, in real arithmetic (module docstring)."""
    lead = det[10]
    if lead == 0 or not np.isfinite(det).all():
        return []
    a = det[:10] / lead
    zr, zi = np.zeros(10), np.zeros(10)
    pr, pi = 1.0, 0.0
    for k in range(10):
        zr[k], zi[k] = pr, pi
        pr, pi = pr - pi, pr + pi
    idx = np.arange(10)
    with np.errstate(all="ignore"):
        for _ in range(POLY_ITERS):
            vr, vi = zr + a[9], zi.copy()
            for k in range(8, -1, -1):
                vr, vi = (vr * zr - vi * zi) + a[k], vr * zi + vi * zr
            dr, di = np.ones(10), np.zeros(10)
            for j in range(10):
                fr, fi = zr - zr[j], zi - zi[j]
                nr, ni = dr * fr - di * fi, dr * fi + di * fr
                dr, di = np.where(idx == j, dr, nr), np.where(idx == j, di, ni)
            den = dr * dr + di * di
            qr, qi = (vr * dr + vi * di) / den, (vi * dr - vr * di) / den
            zr, zi = zr - qr, zi - qi
            if not (np.isfinite(zr).all() and np.isfinite(zi).all()):
                return []
            if ((np.abs(qr) + np.abs(qi)) <= POLY_TOL * ((1.0 + np.abs(zr)) + np.abs(zi))).all():
                break
    return [float(zr[k]) for k in range(10) if abs(zi[k]) < 1e-10]


def null_vector3_port(Bz):
    """unit null vector of the 3 x 3 Bz: the largest (first of equals) of the three cross products of two rows"""
    best, bn = None, -1.0
    for a, b in ((0, 1), (0, 2), (1, 2)):
        u, w = Bz[a], Bz[b]
        v = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
        nn = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
        if nn > bn:
            best, bn = v, nn
    if not bn > 0 or not np.isfinite(bn):
        return None
    return best / np.sqrt(bn)


# ---- "lapack" ----------------------------------------------------------------------------------------------------------
def _null_space_lapack(A):
    return np.linalg.svd(A, full_matrices=True)[2][5:].copy()


def _eliminate_lapack(M):
    try:
        R = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return None
    return R if np.isfinite(R).all() else None


def _roots_lapack(det):
    if not np.isfinite(det).all() or not np.any(det != 0):
        return []
    r = np.roots(det[::-1])
    return [float(z.real) for z in r if abs(z.imag) < 1e-10]


def _null_vector3_lapack(Bz):
    if not np.isfinite(Bz).all():
        return None
    return np.linalg.svd(Bz)[2][2]


# ---- EMEstimatorCallback -----------------------------------------------------------------------------------------------
def epipolar_rows(x1, x2):
    """x1, x2 [k, 2] normalised points -> [k, 9] rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]"""
    a, b, c, d = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    return np.stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones(len(a))], 1)


def run_kernel(x1, x2, linalg="lapack"):
    """The five-point solver on five normalised matches: a list of up to ten E [3, 3] of unit Frobenius norm."""
    port = linalg == "port"
    A = epipolar_rows(np.asarray(x1, np.float64), np.asarray(x2, np.float64))
    ee = null_space_port(A) if port else _null_space_lapack(A)
    M = coeff_matrix(ee)
    R = eliminate_port(M) if port else _eliminate_lapack(M)
    if R is None:
        return []
    B, det = z_polynomials(R)
    roots = roots_port(det) if port else _roots_lapack(det)
    models = []
    for z in roots:
        Bz = np.array([[_horner(p, z) for p in row] for row in B])
        v = null_vector3_port(Bz) if port else _null_vector3_lapack(Bz)
        if v is None or abs(v[2]) < 1e-10:
            continue
        x, y = v[0] / v[2], v[1] / v[2]
        E = ((x * ee[0] + y * ee[1]) + z * ee[2]) + ee[3]
        sq = E * E
        nn = 0.0
        for k in range(9):
            nn = nn + float(sq[k])
        E = E / np.sqrt(nn)
        if np.isfinite(E).all() and len(models) < MAX_MODELS:
            models.append(E.reshape(3, 3))
    return models


def compute_error(x1, x2, E):
    """EMEstimatorCallback::computeError: the Sampson distance in double, stored as float32"""
    e = np.asarray(E, np.float64).reshape(9)
    a, b, c, d = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    with np.errstate(all="ignore"):
        Ex0 = (e[0] * a + e[1] * b) + e[2]
        Ex1 = (e[3] * a + e[4] * b) + e[5]
        Ex2 = (e[6] * a + e[7] * b) + e[8]
        Et0 = (e[0] * c + e[3] * d) + e[6]
        Et1 = (e[1] * c + e[4] * d) + e[7]
        num = (c * Ex0 + d * Ex1) + Ex2
        den = ((Ex0 * Ex0 + Ex1 * Ex1) + Et0 * Et0) + Et1 * Et1
        return (num * num / den).astype(np.float32)


def normalise(pts, K):
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.column_stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]])


# ---- findEssentialMat --------------------------------------------------------------------------------------------------
def find_essential_mat_ransac(pts1, pts2, K, prob=0.999, thresh=1.0, max_iters=DEFAULT_ITERS, linalg="lapack"):
    """Returns (E or None, mask bool [n] or None, info).  E is [3, 3]; for n == 5 the [3k, 3] stack of every model.
    info: "inliers" (-1 without a model), "iterations", "sample", "model" (the winner's index within its sample; for
    n == 5 the number of models), and for the tests "err" (every match's float32 error under the winner), "t" (the float32
    squared threshold), "best" (the (sample, model) pairs that became the best, in order), "n_models" (per sample the loop
    looked at, its number of models) and "sample_indices" (the winning sample's five matches)."""
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = len(p1)
    if len(p2) != n:
        raise ValueError("pts1 / pts2 length mismatch")
    if n > N_MAX:
        raise ValueError(f"at most {N_MAX} matches")
    K = np.asarray(K, np.float64).reshape(3, 3)
    if not (0 < prob < 1):
        prob = 0.999
    if thresh <= 0:
        thresh = 1.0
    max_iters = DEFAULT_ITERS if int(max_iters) <= 0 else min(int(max_iters), MAX_ITERS)
    th = thresh / ((K[0, 0] + K[1, 1]) / 2)
    t = np.float32(th * th)
    info = {"inliers": -1, "iterations": 0, "sample": -1, "model": 0, "err": None, "t": float(t), "best": [],
            "n_models": [], "sample_indices": None}
    if n < MODEL_POINTS:
        return None, None, info
    x1, x2 = normalise(p1, K), normalise(p2, K)
    if n == MODEL_POINTS:
        models = run_kernel(x1, x2, linalg)
        info["n_models"].append(len(models))
        if not models:
            return None, None, info
        info.update(inliers=5, sample=0, model=len(models))
        return np.vstack(models), np.ones(5, bool), info
    rng = CvRNG()
    niters, max_good, best, it = max_iters, 0, None, 0
    while it < niters:
        idx = []
        for _i in range(MODEL_POINTS):
            v = rng.uniform(0, n)
            while v in idx:
                v = rng.uniform(0, n)
            idx.append(v)
        models = run_kernel(x1[idx], x2[idx], linalg)
        info["n_models"].append(len(models))
        for m, E in enumerate(models):
            good = int(np.count_nonzero(compute_error(x1, x2, E) <= t))
            if good > max(max_good, MODEL_POINTS - 1):
                max_good, best = good, E
                info["sample"], info["model"] = it, m
                info["best"].append((it, m))
                info["sample_indices"] = list(idx)
                niters = update_num_iters(prob, (n - good) / n, MODEL_POINTS, niters)
        it += 1
    info["iterations"] = it
    if best is None:
        return None, None, info
    err = compute_error(x1, x2, best)
    mask = err <= t
    info.update(inliers=int(mask.sum()), err=err)
    return best, mask, info
