"""CPU reference (numpy, float64) of `sslam_recover_pose_host` and `sslam_two_view_metrics_host`.

`recover_pose` restates OpenCV 4.x `recoverPose(E, points1, points2, cameraMatrix, R, t, distanceThresh, mask)` and the
`decomposeEssentialMat` under it (modules/calib3d/src/five-point.cpp) line for line; `two_view_metrics` restates the
reference's `triangulation_metrics` (slam/core/two_view_bootstrap.py:127-156) and `_triangulate_points_cv` (:314-326).
Both triangulate with `triangulate_ref.triangulate_points`, the restated `cv2.triangulatePoints`.

`svd` picks the SVD of BOTH the 3 x 3 essential matrix and the 4 x 4 DLT matrices: "lapack" (`np.linalg.svd`) or "jacobi",
a float64 port of the one-sided (Hestenes) Jacobi the GPU kernels run (OpenCV's JacobiSVD is the same method) - two
correct evaluations of the same arithmetic, whose disagreement is the measured floor of the GPU tolerance
(tests/test_relative_pose_gpu.py).  The two may order E's (equal) leading singular vectors and sign them differently:
that permutes the four candidates, never the winner's (R, t, mask, good).

PARITY UNPINNED: the cv2 wheel is absent from the build image.  What is restated from the OpenCV source and could not be
confirmed against a real `cv2` here:
  * the mask VALUE: without an input mask the comparisons leave 255 / 0 (cv::Mat comparison results); with one, cv2 does
    `bitwise_and(mask, mask1, mask1)`, so a 0/1 input mask stays 0/1 and a 255 one stays 255;
  * the float32 ROUNDING in `undistortPoints`: for float32 input OpenCV 4.x computes (x - cx) * (1 / fx) in double and
    stores a float32, which `triangulatePoints` widens again (with no distortion and R = I the steps between are exact);
  * the `>=` CHAIN that picks the winner: candidate 1 when its count is >= every other, else 2, else 3, else 4 - so a tie
    goes to the earlier candidate;
  * a singular value of exactly zero: OpenCV's JacobiSVD completes the basis with a seeded random vector orthogonalised
    against the others; in 3-D that is +-(u0 x u1), which is what is taken here (the sign cancels: det U is fixed next).
"""
import numpy as np

import triangulate_ref as T

W = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
P0 = np.hstack([np.eye(3), np.zeros((3, 1))])


def svd3_jacobi(E):
    """One-sided Jacobi on the columns of E, pairs (0,1) (0,2) (1,2), at most 30 sweeps, a pair left alone when
    |p| <= 10 eps sqrt(a b); singular values sorted descending in OpenCV's selection order.  Returns (U, w, Vt)."""
    A = np.array(E, np.float64)
    V = np.eye(3)
    eps = np.finfo(np.float64).eps * 10
    for _ in range(T.JACOBI_SWEEPS):
        changed = False
        for i in range(2):
            for j in range(i + 1, 3):
                ai, aj = A[:, i], A[:, j]
                a = ai[0] * ai[0] + ai[1] * ai[1] + ai[2] * ai[2]
                b = aj[0] * aj[0] + aj[1] * aj[1] + aj[2] * aj[2]
                p = ai[0] * aj[0] + ai[1] * aj[1] + ai[2] * aj[2]
                if abs(p) <= eps * np.sqrt(a * b):
                    continue
                changed = True
                p *= 2
                beta = a - b
                gamma = np.hypot(p, beta)
                if beta < 0:
                    s = np.sqrt((gamma - beta) * 0.5 / gamma)
                    c = p / (gamma * s * 2)
                else:
                    c = np.sqrt((gamma + beta) / (gamma * 2))
                    s = p / (gamma * c * 2)
                for M in (A, V):
                    mi, mj = M[:, i].copy(), M[:, j].copy()
                    M[:, i] = c * mi + s * mj
                    M[:, j] = c * mj - s * mi
        if not changed:
            break
    w = np.sqrt((A * A).sum(0))
    for i in range(2):
        j = i
        for k in range(i + 1, 3):
            if w[j] < w[k]:
                j = k
        if i != j:
            w[[i, j]] = w[[j, i]]; A[:, [i, j]] = A[:, [j, i]]; V[:, [i, j]] = V[:, [j, i]]
    with np.errstate(all="ignore"):
        U = A / w
    if not w[2] > np.finfo(np.float64).tiny:
        U[:, 2] = np.cross(U[:, 0], U[:, 1])
    return U, w, V.T


def decompose_essential(E, svd="lapack", flip=None):
    """(R1, R2, t [3]).  `flip` in (0, 1, 2) negates that singular-vector pair (column of U, row of Vt) first: another valid
    SVD of the same E, for the test that such a choice does not reach the result."""
    E = np.asarray(E, np.float64).reshape(3, 3)
    if svd == "jacobi":
        U, _, Vt = svd3_jacobi(E)
    else:
        U, _, Vt = np.linalg.svd(E)
    U, Vt = U.copy(), Vt.copy()
    if flip is not None:
        U[:, flip] = -U[:, flip]; Vt[flip] = -Vt[flip]
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].copy()


def candidate_vote(P, x1, x2, thresh, svd="lapack"):
    """One candidate's four comparisons.  Returns (good bool [n], margins): the quantities each comparison looks at -
    Q2 Q3 of the UNIT-norm homogeneous point, the first-view depth and the second-view depth."""
    Q = T.triangulate_points(P0, P, x1, x2, svd).T                       # 4 x n
    s = Q[2] * Q[3]
    good = s > 0
    with np.errstate(all="ignore"):
        Q = Q / Q[3]
        good &= Q[2] < thresh
        z1 = Q[2].copy()
        z2 = (P @ Q)[2]
        good &= z2 > 0
        good &= z2 < thresh
    return good, dict(s=s, z1=z1, z2=z2)


def recover_pose(E, pts1, pts2, K, distance_thresh=50.0, mask=None, svd="lapack", flip=None):
    """Returns (good, R [3,3], t [3,1], mask uint8 [n,1], detail); detail = {"winner", "counts" [4], "R1", "R2", "t",
    "margins": per candidate the dict of `candidate_vote`}."""
    pts1 = np.asarray(pts1, np.float32).reshape(-1, 2).astype(np.float64)
    pts2 = np.asarray(pts2, np.float32).reshape(-1, 2).astype(np.float64)
    K = np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x1 = np.column_stack([(pts1[:, 0] - cx) / fx, (pts1[:, 1] - cy) / fy])
    x2 = np.column_stack([(pts2[:, 0] - cx) / fx, (pts2[:, 1] - cy) / fy])
    R1, R2, t = decompose_essential(E, svd, flip)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    masks, margins = [], []
    for R, tt in cands:
        good, m = candidate_vote(np.hstack([R, tt.reshape(3, 1)]), x1, x2, distance_thresh, svd)
        mk = np.where(good, 255, 0).astype(np.uint8)
        if mask is not None:
            mk = np.bitwise_and(np.asarray(mask, np.uint8).ravel(), mk)
        masks.append(mk); margins.append(m)
    g1, g2, g3, g4 = (int(np.count_nonzero(m)) for m in masks)
    if g1 >= g2 and g1 >= g3 and g1 >= g4:
        win = 0
    elif g2 >= g1 and g2 >= g3 and g2 >= g4:
        win = 1
    elif g3 >= g1 and g3 >= g2 and g3 >= g4:
        win = 2
    else:
        win = 3
    R, tt = cands[win]
    detail = dict(winner=win, counts=[g1, g2, g3, g4], R1=R1, R2=R2, t=t, margins=margins)
    return [g1, g2, g3, g4][win], R.copy(), tt.reshape(3, 1).copy(), masks[win].reshape(-1, 1), detail


def undistort_points(pts, K):
    """cv2.undistortPoints(pts.reshape(-1, 1, 2), K, None).reshape(-1, 2) for float32 pts: float32 out.  THE FLOAT32
    ROUNDING COULD NOT BE CONFIRMED AGAINST A cv2 WHEEL (absent from the build image): it is OpenCV 4.x's source - the
    arithmetic in double, (x - cx) * (1 / fx), the result stored in the input's type."""
    pts = np.asarray(pts, np.float32).reshape(-1, 2).astype(np.float64)
    K = np.asarray(K, np.float64)
    ifx, ify = 1.0 / K[0, 0], 1.0 / K[1, 1]
    return np.column_stack([(pts[:, 0] - K[0, 2]) * ifx, (pts[:, 1] - K[1, 2]) * ify]).astype(np.float32)


def triangulate_points_cv(K, R, t, pts_ref, pts_cur, svd="lapack"):
    """`_triangulate_points_cv` (:314-326): X [N,3] in the first camera's frame"""
    p1n, p2n = undistort_points(pts_ref, K), undistort_points(pts_cur, K)
    P2 = np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)])
    Xh = T.triangulate_points(P0, P2, p1n.astype(np.float64), p2n.astype(np.float64), svd).T
    return (Xh[:3] / (Xh[3] + 1e-12)).T


def two_view_metrics(K, R, t, pts1, pts2, sel=None, svd="lapack"):
    """Returns (posdepth, parallax_deg, N, detail) - `triangulation_metrics` (:127-156) on pts[sel != 0];
    detail = {"X" [N,3], "z" [N,2], "in_front", "angle" [N] radians}."""
    pts1 = np.asarray(pts1, np.float32).reshape(-1, 2)
    pts2 = np.asarray(pts2, np.float32).reshape(-1, 2)
    if sel is not None:
        keep = np.asarray(sel).ravel() != 0
        pts1, pts2 = pts1[keep], pts2[keep]
    R = np.asarray(R, np.float64); t = np.asarray(t, np.float64)
    X = triangulate_points_cv(K, R, t, pts1, pts2, svd) if len(pts1) else np.empty((0, 3))
    z1 = X[:, 2]
    z2 = (R @ X.T + t.reshape(3, 1)).T[:, 2]
    front = (z1 > 0) & (z2 > 0)
    detail = dict(X=X, z=np.column_stack([z1, z2]), in_front=int(front.sum()), angle=np.empty(0))
    if len(pts1) < 2:
        detail["in_front"] = 0
        return 0.0, 0.0, 0, detail
    posdepth = float(np.mean(front))
    C2 = (-R.T @ t.reshape(3)).reshape(1, 3)
    v1, v2 = X, X - C2
    cosang = np.sum(v1 * v2, axis=1) / (np.linalg.norm(v1, axis=1) * np.linalg.norm(v2, axis=1) + 1e-12)
    ang = np.arccos(np.clip(cosang, -1.0, 1.0))
    detail["angle"] = ang
    return posdepth, float(np.degrees(np.median(ang))), len(X), detail
