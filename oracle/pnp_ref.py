"""CPU restatement: `cv2.solvePnPRansac(pts3d, pts2d, K, None, flags=cv2.SOLVEPNP_ITERATIVE, ...)`.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py): numpy, sequential, the yardstick of csrc/pnp_kernels.hip.  It follows the
reference's two call sites, slam/core/pnp_utils.py `solve_pnp_ransac` (:307-341, with and without `Tcw_init`) and
`refine_pose_pnp` (:200-221, no guess, 200 iterations).

PARITY UNPINNED: `opencv_python==4.11.0.86` (requirements.txt:4) is absent here.  Restated from OpenCV 4.x's published
classic (non-USAC) path:
  modules/calib3d/src/solvepnp.cpp   solvePnPRansac (float32 inputs; model_points 5 with EPnP as the minimal solver;
                                     npoints == 5: one EPnP on all points, every point an inlier, the guess ignored;
                                     final solvePnP(SOLVEPNP_ITERATIVE) on the winner's inliers converted to float64,
                                     its guess the winner's model unless the caller passed one), PnPRansacCallback
                                     (runKernel: solvePnP(EPNP) into the `rvec` / `tvec` members, which share their
                                     data with solvePnPRansac's own `rvec` / `tvec`; computeError: projectPoints to
                                     float32 pixels, err = float ||ip - proj||^2), solvePnP / solvePnPGeneric (EPNP
                                     runs on undistortPoints' float32 normalized points)
  modules/calib3d/src/epnp.cpp       epnp: init_points (us = normalized * f + c), choose_control_points (centroid +
                                     PCA), compute_barycentric_coordinates, fill_M, compute_L_6x10, compute_rho,
                                     find_betas_approx_1/2/3, gauss_newton (5 steps of qr_solve), compute_R_and_t,
                                     solve_for_sign, estimate_R_and_t (R = U V^T, last row negated iff det < 0),
                                     reprojection_error; the best of the three by reprojection error
  modules/calib3d/src/calibration.cpp cvFindExtrinsicCameraParams2 with useExtrinsicGuess (no initialisation: the
                                     LM starts at the guess), cvProjectPoints2 (dpdr / dpdt), cvRodrigues2
  modules/calib3d/src/compat_ptsetreg.cpp CvLevMarq (6 parameters, lambda = 10^k from k = -3, JtJ diagonal x (1 +
                                     lambda), DECOMP_SVD solve, rejected step: ++k (<= 16) and retry from the previous
                                     parameters, accepted step: k = max(k - 1, -16); stop after 20 iterations or a
                                     relative L2 step below FLT_EPSILON)
  modules/calib3d/src/ptsetreg.cpp   RANSACPointSetRegistrator::run (RNG((uint64)-1), new best iff count >
                                     max(best, model_points - 1), niters = RANSACUpdateNumIters(...) after each new
                                     best), getSubset (duplicates re-drawn, 10000 attempts; the PnP callback's
                                     checkSubset accepts every subset), findInliers (err <= (float)(thresh^2))
  modules/core/src/undistort.dispatch.cpp cvUndistortPointsInternal (no distortion: x = (u - cx) * (1 / fx))

What this restatement confirms from the source and follows:
  * With a caller guess, `rvec` / `tvec` are the buffers the callback writes every sample's EPnP pose into, so the final
    LM starts from the LAST EVALUATED sample's pose, not the winner's and not the caller's guess; the guess itself never
    reaches any computation.  Without a guess, the LM starts from the winner's model.
  * `reprojectionError` is a `float` parameter: the threshold is (float)ransac_px, squared in double, then rounded to
    float.
  * The returned inlier mask is the RANSAC winner's; the refinement does not recompute it.

Deviations and points not confirmed (named, so a later pin against cv2 knows where to look):
  * Eigen- and singular vectors.  OpenCV takes them from its own Jacobi SVD (cvSVD on MtM, PW0tPW0, ABt; SVD::compute
    in Rodrigues).  Here every one comes from ONE cyclic Jacobi eigen-solver on a symmetric matrix (`jacobi_eigen`,
    the exact algorithm the kernel runs): the singular vectors of a symmetric PSD matrix are its eigenvectors (order:
    descending eigenvalue), and U V^T of a 3 x 3 A is A (A^T A)^(-1/2).  Signs do not change any result; within a
    repeated eigenvalue (a five-point MtM has a two-dimensional null space) the basis is the solver's own, so the EPnP
    of a single five-point sample agrees with OpenCV's up to the convergence of its Gauss-Newton, not to rounding.
  * cvSolve(CV_SVD) of the 6 x k beta systems is taken as epnp's own Householder `qr_solve` (the same least-squares
    solution for full column rank); cvInvert(CV_SVD) of the control-point matrix is its exact pseudo-inverse (rows
    u_j / k_j, dropped where k_j <= 2 DBL_EPSILON sum(k)); CvLevMarq's DECOMP_SVD 6 x 6 solve is Gaussian
    elimination with partial pivoting.  All agree for non-degenerate input.
  * cv::norm(a, b, NORM_RELATIVE | NORM_L2) is taken as ||a - b|| / (||b|| + DBL_EPSILON) (not confirmed for the C API
    cvNorm that CvLevMarq calls).
  * npoints == 4 (OpenCV's P3P minimal solver) is not restated.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.ransac_ref import CvRNG, update_num_iters

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
MODEL_POINTS = 5
SUBSET_ATTEMPTS = 10000
JACOBI_MAX_SWEEPS = 50
LM_MAX_ITERS = 20


def _div(a, b):
    """IEEE a / b (the kernel's division: no exception on 0)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


# ---- linear algebra shared with the kernel (same operations in the same order) --------------------------------------
def jacobi_eigen(A):
    """Cyclic Jacobi on a symmetric matrix.  Returns (eigenvalues descending, eigenvectors as ROWS in that order).
    Rotation (p, q) in row order; from the fifth sweep on an off-diagonal element negligible against both diagonal
    elements is set to 0 instead of rotated; stops after a sweep that starts with every off-diagonal element 0."""
    A = np.array(A, np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for sweep in range(JACOBI_MAX_SWEEPS):
        if not np.any(A[~np.eye(n, dtype=bool)] != 0.0):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = float(A[p, q])
                if apq == 0.0:
                    continue
                app, aqq = float(A[p, p]), float(A[q, q])
                g = 100.0 * abs(apq)
                if sweep >= 4 and abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    A[p, q] = A[q, p] = 0.0
                    continue
                h = aqq - app
                if abs(h) + g == abs(h):
                    t = apq / h
                else:
                    theta = 0.5 * h / apq
                    t = 1.0 / (abs(theta) + math.sqrt(1.0 + theta * theta))
                    if theta < 0.0:
                        t = -t
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = t * c
                tau = s / (1.0 + c)
                gp, hq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = gp - s * (hq + gp * tau)
                A[:, q] = hq + s * (gp - hq * tau)
                A[p, :] = A[:, p]
                A[q, :] = A[:, q]
                A[p, p] = app - t * apq
                A[q, q] = aqq + t * apq
                A[p, q] = A[q, p] = 0.0
                gp, hq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = gp - s * (hq + gp * tau)
                V[:, q] = hq + s * (gp - hq * tau)
    d = np.diag(A).copy()
    order, left = [], list(range(n))
    while left:                                      # descending, ties by index
        b = left[0]
        for i in left[1:]:
            if d[i] > d[b]:
                b = i
        order.append(b)
        left.remove(b)
    return d[order], V[:, order].T.copy()


def polar3(A):
    """U V^T of the SVD of a 3 x 3 A, as A (A^T A)^(-1/2) (rank 3 assumed)."""
    A = np.asarray(A, np.float64)
    AtA = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            AtA[i, j] = A[0, i] * A[0, j] + A[1, i] * A[1, j] + A[2, i] * A[2, j]
    w, Vt = jacobi_eigen(AtA)
    S = np.zeros((3, 3))                             # V diag(1/sqrt(w)) V^T
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc += Vt[k, i] * _div(1.0, math.sqrt(abs(w[k]))) * Vt[k, j]
            S[i, j] = acc
    R = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = A[i, 0] * S[0, j] + A[i, 1] * S[1, j] + A[i, 2] * S[2, j]
    return R


def qr_solve(A, b):
    """epnp::qr_solve (Householder); A [nr, nc], b [nr].  A zero column leaves X at its previous value (None here -> 0)."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    nr, nc = A.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    for k in range(nc):
        eta = abs(A[k, k])
        for i in range(k + 1, nr):
            eta = max(eta, abs(A[i, k]))
        if eta == 0:
            return None
        inv_eta = 1.0 / eta
        sum2 = 0.0
        for i in range(k, nr):
            A[i, k] *= inv_eta
            sum2 += A[i, k] * A[i, k]
        sigma = math.sqrt(sum2)
        if A[k, k] < 0:
            sigma = -sigma
        A[k, k] += sigma
        A1[k] = sigma * A[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i, k] * A[i, j]
            tau = s / A1[k]
            for i in range(k, nr):
                A[i, j] -= tau * A[i, k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i, j] * b[i]
        tau /= A1[j]
        for i in range(j, nr):
            b[i] -= tau * A[i, j]
    X = np.zeros(nc)
    X[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i, j] * X[j]
        X[i] = (b[i] - s) / A2[i]
    return X


def solve_gauss(A, b):
    """Gaussian elimination with partial pivoting (the LM's 6 x 6 solve)."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    n = len(b)
    for k in range(n):
        p = k
        for i in range(k + 1, n):
            if abs(A[i, k]) > abs(A[p, k]):
                p = i
        if p != k:
            A[[k, p]] = A[[p, k]]
            b[k], b[p] = b[p], b[k]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            for j in range(k, n):
                A[i, j] -= f * A[k, j]
            b[i] -= f * b[k]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        s = b[i]
        for j in range(i + 1, n):
            s -= A[i, j] * x[j]
        x[i] = s / A[i, i]
    return x


# ---- Rodrigues ------------------------------------------------------------------------------------------------------
def rodrigues_r2R(r, jac=False):
    rx, ry, rz = (float(v) for v in r)
    theta = math.sqrt(rx * rx + ry * ry + rz * rz)
    if theta < DBL_EPSILON:
        return (np.eye(3), np.zeros((3, 9))) if jac else np.eye(3)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    itheta = 1.0 / theta
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0, -rz, ry, rz, 0, -rx, -ry, rx, 0]
    I = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    R = np.array([(c * I[k] + c1 * rrt[k]) + s * r_x[k] for k in range(9)]).reshape(3, 3)
    if not jac:
        return R
    drrt = [rx + rx, ry, rz, ry, 0, 0, rz, 0, 0,
            0, rx, 0, rx, ry + ry, rz, 0, rz, 0,
            0, 0, rx, 0, 0, ry, rx, ry, rz + rz]
    d_r_x_ = [0, 0, 0, 0, 0, -1, 0, 1, 0,
              0, 0, 1, 0, 0, 0, -1, 0, 0,
              0, -1, 0, 1, 0, 0, 0, 0, 0]
    J = np.zeros((3, 9))
    for i in range(3):
        ri = (rx, ry, rz)[i]
        a0, a1, a2 = -s * ri, (s - 2 * c1 * itheta) * ri, c1 * itheta
        a3, a4 = (c - s * itheta) * ri, s * itheta
        for k in range(9):
            J[i, k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * r_x[k] + a4 * d_r_x_[k]
    return R, J


def rodrigues_R2r(R):
    R = polar3(R)
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt((r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * 0.25)
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) * 0.5
    c = 1.0 if c > 1.0 else (-1.0 if c < -1.0 else c)
    theta = math.acos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3)
        t = (R[0, 0] + 1) * 0.5
        r[0] = math.sqrt(max(t, 0.0))
        t = (R[1, 1] + 1) * 0.5
        r[1] = math.sqrt(max(t, 0.0)) * (-1.0 if R[0, 1] < 0 else 1.0)
        t = (R[2, 2] + 1) * 0.5
        r[2] = math.sqrt(max(t, 0.0)) * (-1.0 if R[0, 2] < 0 else 1.0)
        if abs(r[0]) < abs(r[1]) and abs(r[0]) < abs(r[2]) and (R[1, 2] > 0) != (r[1] * r[2] > 0):
            r[2] = -r[2]
        theta = _div(theta, math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]))
        return r * theta
    vth = 1.0 / (2.0 * s)
    vth *= theta
    return r * vth


# ---- projection -----------------------------------------------------------------------------------------------------
def _cam(X, R, t):
    x = R[0, 0] * X[:, 0] + R[0, 1] * X[:, 1] + R[0, 2] * X[:, 2] + t[0]
    y = R[1, 0] * X[:, 0] + R[1, 1] * X[:, 1] + R[1, 2] * X[:, 2] + t[1]
    z = R[2, 0] * X[:, 0] + R[2, 1] * X[:, 1] + R[2, 2] * X[:, 2] + t[2]
    with np.errstate(all="ignore"):
        iz = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
    return x * iz, y * iz, iz


def reproj_err(pts3d32, pts2d32, rvec, tvec, K):
    """PnPRansacCallback::computeError: float32 pixels from projectPoints, float ||ip - proj||^2."""
    R = rodrigues_r2R(rvec)
    X = pts3d32.astype(np.float64)
    x, y, _ = _cam(X, R, tvec)
    with np.errstate(all="ignore"):
        u = (x * K[0, 0] + K[0, 2]).astype(np.float32)
        v = (y * K[1, 1] + K[1, 2]).astype(np.float32)
        dx = pts2d32[:, 0] - u
        dy = pts2d32[:, 1] - v
        return dx * dx + dy * dy                       # float32 throughout


# ---- EPnP -----------------------------------------------------------------------------------------------------------
def epnp(pw32, ip32, K, trace=None):
    """solvePnP(SOLVEPNP_EPNP): (R [3,3], t [3]).  pw32 [m,3], ip32 [m,2] float32.
    `trace` (a dict, tests only; no result depends on it) receives the branches taken: `beta` (which of the three
    approximations won), per approximation `flip` (solve_for_sign negated the points) and `det_neg` (the row flip of
    estimate_R_and_t), `dropped_axes` (control axes left out of the pseudo-inverse), `ls_singular` / `gn_singular`
    (qr_solve calls that met a zero column, in the beta least squares / in Gauss-Newton)."""
    tr = {"beta": -1, "flip": [], "det_neg": [], "dropped_axes": 0, "ls_singular": 0, "gn_singular": 0}
    fu, fv, uc, vc = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    m = len(pw32)
    pws = pw32.astype(np.float64)
    xn = ((ip32[:, 0].astype(np.float64) - uc) * (1.0 / fu)).astype(np.float32)
    yn = ((ip32[:, 1].astype(np.float64) - vc) * (1.0 / fv)).astype(np.float32)
    us = np.stack([xn.astype(np.float64) * fu + uc, yn.astype(np.float64) * fv + vc], 1)
    # choose_control_points
    cws = np.zeros((4, 3))
    for i in range(m):
        for j in range(3):
            cws[0, j] += pws[i, j]
    cws[0] /= m
    PW0 = pws - cws[0]
    P = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            acc = 0.0
            for i in range(m):
                acc += PW0[i, a] * PW0[i, b]
            P[a, b] = acc
    dc, uct = jacobi_eigen(P)
    ks = [math.sqrt(abs(dc[i]) / m) for i in range(3)]
    for i in range(1, 4):
        cws[i] = cws[0] + ks[i - 1] * uct[i - 1]
    # compute_barycentric_coordinates: CC = [k_j u_j], its pseudo-inverse has rows u_j / k_j
    thr = 2 * DBL_EPSILON * (ks[0] + ks[1] + ks[2])
    ci = np.zeros((3, 3))
    for j in range(3):
        if ks[j] > thr:
            ci[j] = uct[j] / ks[j]
        else:
            tr["dropped_axes"] += 1
    alphas = np.zeros((m, 4))
    for i in range(m):
        d = pws[i] - cws[0]
        for j in range(3):
            alphas[i, 1 + j] = ci[j, 0] * d[0] + ci[j, 1] * d[1] + ci[j, 2] * d[2]
        alphas[i, 0] = 1.0 - alphas[i, 1] - alphas[i, 2] - alphas[i, 3]
    M = np.zeros((2 * m, 12))
    for i in range(m):
        for j in range(4):
            M[2 * i, 3 * j] = alphas[i, j] * fu
            M[2 * i, 3 * j + 2] = alphas[i, j] * (uc - us[i, 0])
            M[2 * i + 1, 3 * j + 1] = alphas[i, j] * fv
            M[2 * i + 1, 3 * j + 2] = alphas[i, j] * (vc - us[i, 1])
    MtM = np.zeros((12, 12))
    for a in range(12):
        for b in range(12):
            acc = 0.0
            for r in range(2 * m):
                acc += M[r, a] * M[r, b]
            MtM[a, b] = acc
    _, ut = jacobi_eigen(MtM)
    v = [ut[11], ut[10], ut[9], ut[8]]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.array([[v[i][3 * a:3 * a + 3] - v[i][3 * b:3 * b + 3] for (a, b) in pairs] for i in range(4)])

    def dot(x, y):
        return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    L = np.zeros((6, 10))
    for i in range(6):
        L[i] = [dot(dv[0, i], dv[0, i]), 2.0 * dot(dv[0, i], dv[1, i]), dot(dv[1, i], dv[1, i]),
                2.0 * dot(dv[0, i], dv[2, i]), 2.0 * dot(dv[1, i], dv[2, i]), dot(dv[2, i], dv[2, i]),
                2.0 * dot(dv[0, i], dv[3, i]), 2.0 * dot(dv[1, i], dv[3, i]), 2.0 * dot(dv[2, i], dv[3, i]),
                dot(dv[3, i], dv[3, i])]
    rho = np.array([dot(cws[a] - cws[b], cws[a] - cws[b]) for (a, b) in pairs])

    def gauss_newton(betas):
        x = np.zeros(4)
        for _ in range(5):
            A = np.zeros((6, 4))
            bb = np.zeros(6)
            b0, b1, b2, b3 = betas
            for i in range(6):
                l = L[i]
                A[i] = [2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3,
                        l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3,
                        l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3,
                        l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3]
                bb[i] = rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2
                                  + l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3)
            X = qr_solve(A, bb)
            if X is not None:
                x = X
            else:
                tr["gn_singular"] += 1
            betas = [betas[i] + x[i] for i in range(4)]
        return betas

    def ls(cols):
        X = qr_solve(L[:, cols], rho)
        if X is None:
            tr["ls_singular"] += 1
        return np.zeros(len(cols)) if X is None else X

    with np.errstate(all="ignore"):
        b4 = ls([0, 1, 3, 6])
        if b4[0] < 0:
            b0 = math.sqrt(-b4[0])
            B1 = [b0, _div(-b4[1], b0), _div(-b4[2], b0), _div(-b4[3], b0)]
        else:
            b0 = math.sqrt(b4[0])
            B1 = [b0, _div(b4[1], b0), _div(b4[2], b0), _div(b4[3], b0)]
        b3 = ls([0, 1, 2])
        if b3[0] < 0:
            B2 = [math.sqrt(-b3[0]), math.sqrt(-b3[2]) if b3[2] < 0 else 0.0]
        else:
            B2 = [math.sqrt(b3[0]), math.sqrt(b3[2]) if b3[2] > 0 else 0.0]
        if b3[1] < 0:
            B2[0] = -B2[0]
        B2 += [0.0, 0.0]
        b5 = ls([0, 1, 2, 3, 4])
        if b5[0] < 0:
            B3 = [math.sqrt(-b5[0]), math.sqrt(-b5[2]) if b5[2] < 0 else 0.0]
        else:
            B3 = [math.sqrt(b5[0]), math.sqrt(b5[2]) if b5[2] > 0 else 0.0]
        if b5[1] < 0:
            B3[0] = -B3[0]
        B3 += [_div(b5[3], B3[0]), 0.0]

        best = None
        for which, betas in enumerate((B1, B2, B3)):
            betas = gauss_newton(betas)
            ccs = np.zeros((4, 3))
            for i in range(4):
                vv = v[i]
                for j in range(4):
                    for k in range(3):
                        ccs[j, k] += betas[i] * vv[3 * j + k]
            pcs = np.zeros((m, 3))
            for i in range(m):
                a = alphas[i]
                for j in range(3):
                    pcs[i, j] = a[0] * ccs[0, j] + a[1] * ccs[1, j] + a[2] * ccs[2, j] + a[3] * ccs[3, j]
            tr["flip"].append(bool(pcs[0, 2] < 0.0))
            if pcs[0, 2] < 0.0:
                ccs, pcs = -ccs, -pcs
            pc0, pw0 = np.zeros(3), np.zeros(3)
            for i in range(m):
                for j in range(3):
                    pc0[j] += pcs[i, j]
                    pw0[j] += pws[i, j]
            pc0 /= m
            pw0 /= m
            abt = np.zeros((3, 3))
            for i in range(m):
                for j in range(3):
                    for k in range(3):
                        abt[j, k] += (pcs[i, j] - pc0[j]) * (pws[i, k] - pw0[k])
            R = polar3(abt)
            det = (R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0] + R[0, 2] * R[1, 0] * R[2, 1]
                   - R[0, 2] * R[1, 1] * R[2, 0] - R[0, 1] * R[1, 0] * R[2, 2] - R[0, 0] * R[1, 2] * R[2, 1])
            tr["det_neg"].append(bool(det < 0))
            if det < 0:
                R[2] = -R[2]
            t = np.array([pc0[j] - dot(R[j], pw0) for j in range(3)])
            sum2 = 0.0
            for i in range(m):
                pw = pws[i]
                Xc = dot(R[0], pw) + t[0]
                Yc = dot(R[1], pw) + t[1]
                inv_Zc = _div(1.0, dot(R[2], pw) + t[2])
                ue = uc + fu * Xc * inv_Zc
                ve = vc + fv * Yc * inv_Zc
                sum2 += math.sqrt((us[i, 0] - ue) * (us[i, 0] - ue) + (us[i, 1] - ve) * (us[i, 1] - ve))
            err = sum2 / m
            if best is None or err < best[0]:
                best = (err, R, t)
                tr["beta"] = which
    if trace is not None:
        trace.update(tr)
    return best[1], best[2]


def epnp_model(pw32, ip32, K, trace=None):
    """runKernel: the EPnP pose as the callback's (rvec, tvec).  `trace`: epnp's, plus `nan_model`."""
    R, t = epnp(pw32, ip32, K, trace)
    finite = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)))
    if trace is not None:
        trace["nan_model"] = not finite
    if not finite:
        return np.full(3, np.nan), np.full(3, np.nan)
    return rodrigues_R2r(R), t


# ---- LM (cvFindExtrinsicCameraParams2 with a guess) -----------------------------------------------------------------
def _project_jac(X, m, param, K):
    """err = proj - m (double), J [2n, 6] = (dpdr | dpdt)."""
    R, dRdr = rodrigues_r2R(param[:3], jac=True)
    t = param[3:]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = _cam(X, R, t)
    n = len(X)
    err = np.empty(2 * n)
    err[0::2] = x * fx + cx - m[:, 0]
    err[1::2] = y * fy + cy - m[:, 1]
    J = np.zeros((2 * n, 6))
    J[0::2, 3] = fx * z
    J[1::2, 4] = fy * z
    J[0::2, 5] = fx * (-x * z)
    J[1::2, 5] = fy * (-y * z)
    Xs, Ys, Zs = X[:, 0], X[:, 1], X[:, 2]
    for j in range(3):
        dx0 = Xs * dRdr[j, 0] + Ys * dRdr[j, 1] + Zs * dRdr[j, 2]
        dy0 = Xs * dRdr[j, 3] + Ys * dRdr[j, 4] + Zs * dRdr[j, 5]
        dz0 = Xs * dRdr[j, 6] + Ys * dRdr[j, 7] + Zs * dRdr[j, 8]
        J[0::2, j] = fx * (z * (dx0 - x * dz0))
        J[1::2, j] = fy * (z * (dy0 - y * dz0))
    return err, J


def _project_err(X, m, param, K):
    R = rodrigues_r2R(param[:3])
    x, y, _ = _cam(X, R, param[3:])
    err = np.empty(2 * len(X))
    err[0::2] = x * K[0, 0] + K[0, 2] - m[:, 0]
    err[1::2] = y * K[1, 1] + K[1, 2] - m[:, 1]
    return err


def refine_lm(X, m, rvec, tvec, K, max_iter=LM_MAX_ITERS, trace=None):
    """CvLevMarq driven as cvFindExtrinsicCameraParams2 drives it.  Returns (rvec, tvec, iterations).
    `trace` (a dict, tests only) receives `rejected` (steps retried with a larger lambda), `k_max`, `exit` ("cap": the
    iteration limit, "small_step": the relative step), `min_margin` (the smallest |err_norm - prev| / prev over the
    accept / reject decisions; nan compares as 0) and `stop_margin` (the smallest |step - FLT_EPSILON| / FLT_EPSILON
    over the stop tests that the step decided)."""
    tr = {"rejected": 0, "k_max": -3, "exit": None, "min_margin": math.inf, "stop_margin": math.inf}

    def _margin(a, b):
        with np.errstate(all="ignore"):
            v = abs(a - b) / b if b != 0 else math.inf
        return 0.0 if v != v else float(v)
    param = np.concatenate([np.asarray(rvec, np.float64), np.asarray(tvec, np.float64)])
    k = -3
    iters = 0
    err, J = _project_jac(X, m, param, K)
    prev_err_norm = None
    while True:
        JtJ, JtErr = J.T @ J, J.T @ err
        prev = param.copy()
        if prev_err_norm is None:
            prev_err_norm = float(np.sqrt(err @ err))

        def step():
            A = JtJ.copy()
            lam = math.exp(k * math.log(10.0))
            for i in range(6):
                A[i, i] *= 1.0 + lam
            return prev - solve_gauss(A, JtErr)
        param = step()
        while True:
            err_norm = float(np.sqrt(np.sum(_project_err(X, m, param, K) ** 2)))
            tr["min_margin"] = min(tr["min_margin"], _margin(err_norm, prev_err_norm))
            if err_norm > prev_err_norm:
                k += 1
                tr["k_max"] = max(tr["k_max"], k)
                if k <= 16:
                    tr["rejected"] += 1
                    param = step()
                    continue
            break
        k = max(k - 1, -16)
        iters += 1
        dn = float(np.sqrt(np.sum((param - prev) ** 2)))
        pn = float(np.sqrt(np.sum(prev ** 2)))
        if iters < max_iter:
            tr["stop_margin"] = min(tr["stop_margin"], _margin(dn / (pn + DBL_EPSILON), FLT_EPSILON))
        if iters >= max_iter or dn / (pn + DBL_EPSILON) < FLT_EPSILON:
            tr["exit"] = "cap" if iters >= max_iter else "small_step"
            break
        prev_err_norm = err_norm
        err, J = _project_jac(X, m, param, K)
    if trace is not None:
        trace.update(tr)
    return param[:3].copy(), param[3:].copy(), iters


# ---- solvePnPRansac -------------------------------------------------------------------------------------------------
def solve_pnp_ransac(pts3d, pts2d, K, ransac_px=8.0, use_guess=False, iters=100, conf=0.99, trace=None):
    """Returns (ok, rvec, tvec, mask bool[n], info dict).  info: inliers (-1: no model), samples, winner, lm_iters.
    `trace` (a dict, tests only) receives `samples` (one epnp_model trace per sample, with its subset `idx`, its
    `model` and its inlier count `good`), `budgets` (the budget after each new best), `winner` / `last` (the models
    the refinement may start from) and `lm` (refine_lm's trace)."""
    tr = {"samples": [], "budgets": [], "winner": None, "last": None, "lm": {}}
    if trace is not None:
        trace.update(tr)
        tr = trace
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    K = np.asarray(K, np.float64).reshape(3, 3)
    n = len(p3)
    info = {"inliers": -1, "samples": 0, "sample": -1, "lm_iters": 0}
    if n < MODEL_POINTS:
        if n == 4:
            raise NotImplementedError("npoints == 4: OpenCV's P3P minimal solver is not restated")
        return False, None, None, np.zeros(n, bool), info
    if n == MODEL_POINTS:
        st = {"idx": list(range(n))}
        rvec, tvec = epnp_model(p3, p2, K, st)
        tr["samples"].append(st)
        info.update(inliers=n)
        return True, rvec, tvec, np.ones(n, bool), info
    thresh = float(np.float32(ransac_px))
    t = np.float32(thresh * thresh)
    rng = CvRNG()
    niters = max(int(iters), 1)
    max_good, best, best_mask = 0, None, None
    last = None
    it = 0
    while it < niters:
        idx = []
        for _ in range(MODEL_POINTS):
            v = rng.uniform(0, n)
            while v in idx:
                v = rng.uniform(0, n)
            idx.append(v)
        st = {"idx": idx}
        model = epnp_model(p3[idx], p2[idx], K, st)
        tr["samples"].append(st)
        last = model
        e = reproj_err(p3, p2, model[0], model[1], K)
        mask = e <= t
        good = int(np.count_nonzero(mask))
        st["model"], st["good"] = model, good
        if good > max(max_good, MODEL_POINTS - 1):
            max_good, best, best_mask = good, model, mask
            info["sample"] = it
            niters = update_num_iters(conf, (n - good) / n, MODEL_POINTS, niters)
            tr["budgets"].append(niters)
        it += 1
    info["samples"] = it
    if best is None:
        return False, None, None, np.zeros(n, bool), info
    info["inliers"] = max_good
    start = last if use_guess else best
    tr["winner"], tr["last"] = best, last
    X = p3[best_mask].astype(np.float64)
    m = p2[best_mask].astype(np.float64)
    rvec, tvec, lm_iters = refine_lm(X, m, start[0], start[1], K, trace=tr["lm"])
    info["lm_iters"] = lm_iters
    return True, rvec, tvec, best_mask, info


def pose_matrix(rvec, tvec):
    T = np.eye(4)
    T[:3, :3] = rodrigues_r2R(rvec)
    T[:3, 3] = tvec
    return T
