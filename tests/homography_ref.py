"""CPU reference (numpy, float64) of `sslam_homography_ransac_host`: OpenCV 4.x's classic (non-USAC)
`findHomography(src, dst, RANSAC, thresh, mask, maxIters = 2000, confidence = 0.995)` restated, sequentially.

`linalg` picks how the three small dense problems are solved: "lapack" (`np.linalg.eigh`, `solve`, `inv`) or "jacobi",
float64 ports of what the kernel runs - the cyclic Jacobi on the symmetric 9 x 9 matrix, Gaussian elimination with partial
pivoting for the 8 x 8 steps, Gauss-Jordan for the 8 x 8 inverse.  Two correct evaluations of the same arithmetic: what they
disagree by is the measured floor of the GPU tolerance (tests/test_homography_gpu.py).

PARITY UNPINNED: the cv2 wheel and OpenCV's sources are absent from the build image.  Restated from memory of
modules/calib3d/src/fundam.cpp (findHomography, HomographyEstimatorCallback::{checkSubset, runKernel, computeError},
HomographyRefineCallback), ptsetreg.cpp (RANSACPointSetRegistrator::run, getSubset) and modules/calib3d/src/compat_ptsetreg.cpp /
modules/core levmarq (LMSolverImpl::run).  What could NOT be confirmed against a real cv2 here:
  * `cv::eigen` on the 9 x 9 LtL: OpenCV runs a Jacobi that picks the largest off-diagonal pivot of a row, here the pairs are
    taken cyclically; both end at the eigenvector of the smallest eigenvalue, whose sign cancels in H / H[8];
  * the whole schedule of `LMSolverImpl::run`: lambda starting at 1, lc = 0.75, Rlo / Rhi, the nu clamp, the damping
    `A + lambda diag(A)` with the diagonal of the CURRENT A (OpenCV may keep the diagonal of the first A), both stopping
    thresholds at DBL_EPSILON (OpenCV's factory default may be FLT_EPSILON), the `|d . v| > DBL_EPSILON else 1` guard of nu;
  * `solve` / `invert` with DECOMP_EIG inside it: replaced by elimination (the systems are positive definite);
  * H scaled by a division by H[8] (OpenCV's convertTo multiplies by the reciprocal);
  * the order in which OpenCV sums the centroids and LtL (sequential there, numpy's here, a tree on the GPU).
"""
import math

import numpy as np

from oracle.ransac_ref import CvRNG, DBL_EPSILON, FLT_EPSILON, update_num_iters

MODEL_POINTS = 4
MAX_ITERS = 2000
SUBSET_ATTEMPTS = 10000
N_MAX = 16384
JACOBI_SWEEPS = 30
ORIENT_TRIPLES = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))


# ---- the small dense solvers the kernel runs, in float64 ---------------------------------------------------------------
def jacobi_eig_smallest(A):
    """Eigenvector of the smallest eigenvalue of the symmetric A by cyclic Jacobi: pairs (p, q), p < q, row by row; a pair
    is left alone when |a_pq| <= 1e-18 trace(A); at most 30 sweeps.  The first of equal diagonal entries wins."""
    A = np.array(A, np.float64)
    n = len(A)
    V = np.eye(n)
    thr = 1e-18 * float(np.trace(A))
    for _ in range(JACOBI_SWEEPS):
        changed = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if not abs(apq) > thr:
                    continue
                changed = True
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for M in (A, V):
                    mp, mq = M[:, p].copy(), M[:, q].copy()
                    M[:, p] = c * mp - s * mq
                    M[:, q] = s * mp + c * mq
                rp, rq = A[p].copy(), A[q].copy()
                A[p] = c * rp - s * rq
                A[q] = s * rp + c * rq
        if not changed:
            break
    return V[:, int(np.argmin(np.diag(A)))].copy()


def gauss_solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting (the first of equal pivots); None when a pivot is zero."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = len(b)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if A[piv, k] == 0 or not np.isfinite(A[piv, k]):
            return None
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] = A[i, k:] - f * A[k, k:]
            b[i] = b[i] - f * b[k]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        acc = b[i]
        for j in range(i + 1, n):
            acc = acc - A[i, j] * x[j]
        x[i] = acc / A[i, i]
    return x


def gauss_inverse_diag(A):
    """The diagonal of A^-1, column by column with `gauss_solve`; None when A is singular."""
    n = len(A)
    out = np.zeros(n)
    for k in range(n):
        e = np.zeros(n)
        e[k] = 1.0
        x = gauss_solve(A, e)
        if x is None:
            return None
        out[k] = x[k]
    return out


# ---- HomographyEstimatorCallback ---------------------------------------------------------------------------------------
def last_point_collinear(pts, idx):
    """haveCollinearPoints: the last point against every earlier pair (the test of the F-matrix filter)"""
    i = len(idx) - 1
    xi, yi = float(pts[idx[i]][0]), float(pts[idx[i]][1])
    for j in range(i):
        dx1, dy1 = float(pts[idx[j]][0]) - xi, float(pts[idx[j]][1]) - yi
        for k in range(j):
            dx2, dy2 = float(pts[idx[k]][0]) - xi, float(pts[idx[k]][1]) - yi
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _det3_ones(p, t):
    """det [[x, y, 1] ...] of the three points p[t], cv::Matx33d's expansion"""
    (a, b), (c, d), (e, f) = ((float(p[k][0]), float(p[k][1])) for k in t)
    return a * (d * 1.0 - f * 1.0) - b * (c * 1.0 - e * 1.0) + 1.0 * (c * f - e * d)


def orientation_negatives(src4, dst4):
    return sum(_det3_ones(src4, t) * _det3_ones(dst4, t) < 0 for t in ORIENT_TRIPLES)


def check_subset(p1, p2, idx):
    if last_point_collinear(p1, idx) or last_point_collinear(p2, idx):
        return False
    if len(idx) == 4:
        neg = orientation_negatives(p1[idx], p2[idx])
        if neg != 0 and neg != 4:
            return False
    return True


def get_subset(p1, p2, rng, stats=None):
    n = len(p1)
    for _ in range(SUBSET_ATTEMPTS):
        idx = []
        for _i in range(MODEL_POINTS):
            v = rng.uniform(0, n)
            while v in idx:
                v = rng.uniform(0, n)
            idx.append(v)
        if check_subset(p1, p2, idx):
            return idx
        if stats is not None:
            collinear = last_point_collinear(p1, idx) or last_point_collinear(p2, idx)
            stats["rejected_collinear" if collinear else "rejected_orientation"] += 1
    return None


def run_kernel(M, m, linalg="lapack"):
    """The normalised DLT on source points M and destination points m ([k, 2]); H [3, 3] with H[2, 2] = 1, or None."""
    M = np.asarray(M, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    count = len(M)
    cM, cm = M.sum(0) / count, m.sum(0) / count
    sM, sm = np.abs(M - cM).sum(0), np.abs(m - cm).sum(0)
    if sM[0] < DBL_EPSILON or sM[1] < DBL_EPSILON or sm[0] < DBL_EPSILON or sm[1] < DBL_EPSILON:
        return None
    sM, sm = count / sM, count / sm
    invHnorm = np.array([[1.0 / sm[0], 0, cm[0]], [0, 1.0 / sm[1], cm[1]], [0, 0, 1]])
    Hnorm2 = np.array([[sM[0], 0, -cM[0] * sM[0]], [0, sM[1], -cM[1] * sM[1]], [0, 0, 1]])
    x, y = (m[:, 0] - cm[0]) * sm[0], (m[:, 1] - cm[1]) * sm[1]
    X, Y = (M[:, 0] - cM[0]) * sM[0], (M[:, 1] - cM[1]) * sM[1]
    one, zero = np.ones(count), np.zeros(count)
    Lx = np.stack([X, Y, one, zero, zero, zero, -x * X, -x * Y, -x], 1)
    Ly = np.stack([zero, zero, zero, X, Y, one, -y * X, -y * Y, -y], 1)
    LtL = Lx.T @ Lx + Ly.T @ Ly
    LtL = np.triu(LtL) + np.triu(LtL, 1).T
    if linalg == "jacobi":
        h0 = jacobi_eig_smallest(LtL)
    else:
        h0 = np.linalg.eigh(LtL)[1][:, 0]
    H = invHnorm @ h0.reshape(3, 3) @ Hnorm2
    with np.errstate(all="ignore"):
        return H / H[2, 2]


def compute_error(p1, p2, H):
    """HomographyEstimatorCallback::computeError: everything in float32"""
    Hf = np.asarray(H, np.float64).reshape(9).astype(np.float32)
    X, Y, x, y = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    one = np.float32(1)
    with np.errstate(all="ignore"):
        ww = one / (Hf[6] * X + Hf[7] * Y + one)
        dx = (Hf[0] * X + Hf[1] * Y + Hf[2]) * ww - x
        dy = (Hf[3] * X + Hf[4] * Y + Hf[5]) * ww - y
        return dx * dx + dy * dy


# ---- HomographyRefineCallback + LMSolver -------------------------------------------------------------------------------
def _lm_eval(h, M, m, want_jac):
    X, Y = M[:, 0], M[:, 1]
    den = h[6] * X + h[7] * Y + 1.0
    with np.errstate(all="ignore"):
        ww = np.where(np.abs(den) < DBL_EPSILON, 0.0, 1.0 / den)
    xi = (h[0] * X + h[1] * Y + h[2]) * ww
    yi = (h[3] * X + h[4] * Y + h[5]) * ww
    r = np.stack([xi - m[:, 0], yi - m[:, 1]], 1).reshape(-1)
    if not want_jac:
        return r, None
    z = np.zeros_like(X)
    Jx = np.stack([X * ww, Y * ww, ww, z, z, z, -X * ww * xi, -Y * ww * xi], 1)
    Jy = np.stack([z, z, z, X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi], 1)
    J = np.stack([Jx, Jy], 1).reshape(-1, 8)
    return r, J


def lm_polish(H, M, m, linalg="lapack", max_iters=10):
    """LMSolver (at most 10 iterations) on the first eight entries of H over the matches (M -> m).  Returns (H, iterations)."""
    M = np.asarray(M, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    x = np.asarray(H, np.float64).reshape(9)[:8].copy()
    r, J = _lm_eval(x, M, m, True)
    S = float(r @ r)
    A, v = J.T @ J, J.T @ r
    lam, lc = 1.0, 0.75
    Rlo, Rhi = 0.25, 0.75
    it = 0
    while True:
        Ap = A + lam * np.diag(np.diag(A))
        d = gauss_solve(Ap, v) if linalg == "jacobi" else _lapack_solve(Ap, v)
        if d is None:
            break
        xd = x - d
        rd, _ = _lm_eval(xd, M, m, False)
        Sd = float(rd @ rd)
        dS = float(d @ (2.0 * v - A @ d))
        R = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1.0)
        if R > Rhi:
            lam *= 0.5
            if lam < lc:
                lam = 0.0
        elif R < Rlo:
            t = float(d @ v)
            nu = (Sd - S) / (t if abs(t) > DBL_EPSILON else 1.0) + 2.0
            nu = min(max(nu, 2.0), 10.0)
            if lam == 0:
                dg = gauss_inverse_diag(A) if linalg == "jacobi" else _lapack_inverse_diag(A)
                maxval = DBL_EPSILON if dg is None else max(DBL_EPSILON, float(np.abs(dg).max()))
                lam = lc = 1.0 / maxval
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x = Sd, xd
            r, J = _lm_eval(x, M, m, True)
            A, v = J.T @ J, J.T @ r
        it += 1
        if not (it < max_iters and np.abs(d).max() >= DBL_EPSILON and np.abs(r).max() >= DBL_EPSILON):
            break
    return np.concatenate([x, [1.0]]).reshape(3, 3), it


def _lapack_solve(A, b):
    try:
        x = np.linalg.solve(A, b)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def _lapack_inverse_diag(A):
    try:
        return np.diag(np.linalg.inv(A)).copy()
    except np.linalg.LinAlgError:
        return None


# ---- findHomography ----------------------------------------------------------------------------------------------------
def find_homography_ransac(pts1, pts2, thresh=3.0, confidence=0.995, max_iters=MAX_ITERS, linalg="lapack"):
    """Returns (H [3,3] or None, mask bool [n] or None, info).  info: "inliers" (-1 without a model), "iterations", "sample",
    and for the tests "loop_H" (the winning sample's model, before the refit), "err" (every match's float32 error under it),
    "t" (the float32 squared threshold), "rejected_collinear" / "rejected_orientation" (draws getSubset threw away), "rejected_first" (those
    thrown away before the first sample was accepted, as (collinear, orientation)) and "best_samples" (the samples that
    became the best, in order)."""
    p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
    n = len(p1)
    if len(p2) != n:
        raise ValueError("pts1 / pts2 length mismatch")
    if n < 4:
        raise ValueError("findHomography needs at least 4 matches")
    if n > N_MAX:
        raise ValueError(f"at most {N_MAX} matches")
    if thresh <= 0:
        thresh = 3
    if not (0 < confidence < 1):
        confidence = 0.995
    max_iters = min(max(int(max_iters), 1), MAX_ITERS)
    t = np.float32(thresh * thresh)
    info = {"inliers": -1, "iterations": 0, "sample": -1, "loop_H": None, "err": None, "t": float(t),
            "rejected_collinear": 0, "rejected_orientation": 0, "rejected_first": (0, 0), "best_samples": [],
            "lm_iterations": 0}
    if n == 4:
        H = run_kernel(p1, p2, linalg)
        if H is None:
            return None, None, info
        info.update(inliers=4, sample=0, loop_H=H)
        return H, np.ones(4, bool), info
    rng = CvRNG()
    niters, max_good, best, it = max_iters, 0, None, 0
    while it < niters:
        idx = get_subset(p1, p2, rng, info)
        if it == 0:
            info["rejected_first"] = (info["rejected_collinear"], info["rejected_orientation"])
        if idx is None:
            break                                   # (iteration 0: no model; later: the loop ends)
        H = run_kernel(p1[idx], p2[idx], linalg)
        if H is not None:
            good = int(np.count_nonzero(compute_error(p1, p2, H) <= t))
            if good > max(max_good, MODEL_POINTS - 1):
                max_good, best = good, H
                info["sample"] = it
                info["best_samples"].append(it)
                niters = update_num_iters(confidence, (n - good) / n, MODEL_POINTS, niters)
        it += 1
    info["iterations"] = it
    if best is None:
        return None, None, info
    err = compute_error(p1, p2, best)
    mask = err <= t
    info.update(inliers=int(mask.sum()), loop_H=best, err=err)
    H = best
    refit = run_kernel(p1[mask], p2[mask], linalg)
    if refit is not None:
        H = refit
    H, info["lm_iterations"] = lm_polish(H, p1[mask], p2[mask], linalg)
    return H, mask, info
