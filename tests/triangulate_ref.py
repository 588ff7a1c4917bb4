"""CPU reference (numpy, float64) of the numeric body of `triangulate_between_kfs_2view`
(reference slam/core/triangulation_utils.py:143-271), restated line for line: projections (:148-149),
`cv2.triangulatePoints` (:152), the homogeneous test (:153-159), `_angle_parallax_deg_batch` (:54-77), the camera-frame
depths and reprojection errors (:195-209) and the gate loop with its `continue`s (:211-249).

`cv2.triangulatePoints` is restated from OpenCV 4.x modules/calib3d/src/triangulate.cpp: per point the 4 x 4 matrix with
rows x P[2] - P[0], y P[2] - P[1] for each view, and the right singular vector of its smallest singular value - here from
`np.linalg.svd` (LAPACK), or, with svd="jacobi", from a float64 port of the one-sided (Hestenes) Jacobi SVD the GPU kernel
runs (OpenCV's JacobiSVD is the same method): two correct evaluations of the same arithmetic, whose disagreement is the
measured floor of the GPU tolerance (tests/test_triangulate_gpu.py).

PARITY UNPINNED: the cv2 wheel is absent from the build image, so agreement with a real `cv2.triangulatePoints` could not
be confirmed here (oracle/pnp_ref.py says the same of its restatement).

The reference has no reason for a match whose w is not usable (it never enters its loop); it is "invalid_w" here.
"""
import numpy as np

REASONS = ("kept", "invalid_w", "low_parallax", "bad_depth", "behind_cam", "high_reproj")
KEPT, INVALID_W, LOW_PARALLAX, BAD_DEPTH, BEHIND_CAM, HIGH_REPROJ = range(6)
JACOBI_SWEEPS = 30


def dlt_matrices(P1, P2, pts1, pts2):
    """[n,4,4]: rows x1 P1[2] - P1[0], y1 P1[2] - P1[1], x2 P2[2] - P2[0], y2 P2[2] - P2[1]"""
    p1 = np.asarray(pts1, np.float64).reshape(-1, 2)
    p2 = np.asarray(pts2, np.float64).reshape(-1, 2)
    A = np.empty((len(p1), 4, 4))
    A[:, 0] = p1[:, 0:1] * P1[2] - P1[0]
    A[:, 1] = p1[:, 1:2] * P1[2] - P1[1]
    A[:, 2] = p2[:, 0:1] * P2[2] - P2[0]
    A[:, 3] = p2[:, 1:2] * P2[2] - P2[1]
    return A


def null_vectors_jacobi(A):
    """One-sided Jacobi on the columns of every A[i] ([n,4,4]), rotation order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most
    30 sweeps, a pair left alone when |p| <= 10 eps sqrt(a b): the column of V belonging to the column of smallest norm."""
    A = np.array(A, np.float64)                      # columns are A[:, :, j]
    n = len(A)
    V = np.tile(np.eye(4), (n, 1, 1))
    eps = np.finfo(np.float64).eps * 10
    for _ in range(JACOBI_SWEEPS):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                ai, aj = A[:, :, i], A[:, :, j]
                a = (ai * ai).sum(1); b = (aj * aj).sum(1); p = (ai * aj).sum(1)
                act = ~(np.abs(p) <= eps * np.sqrt(a * b))
                if not act.any():
                    continue
                changed = True
                with np.errstate(all="ignore"):
                    p2 = p * 2
                    beta = a - b
                    gamma = np.hypot(p2, beta)
                    neg = beta < 0
                    delta = (gamma - beta) * 0.5
                    s_neg = np.sqrt(delta / gamma); c_neg = p2 / (gamma * s_neg * 2)
                    c_pos = np.sqrt((gamma + beta) / (gamma * 2)); s_pos = p2 / (gamma * c_pos * 2)
                c = np.where(act, np.where(neg, c_neg, c_pos), 1.0)[:, None]
                s = np.where(act, np.where(neg, s_neg, s_pos), 0.0)[:, None]
                for M in (A, V):
                    mi, mj = M[:, :, i].copy(), M[:, :, j].copy()
                    M[:, :, i] = np.where(act[:, None], c * mi + s * mj, mi)
                    M[:, :, j] = np.where(act[:, None], c * mj - s * mi, mj)
        if not changed:
            break
    k = np.argmin((A * A).sum(1), axis=1)            # first of equals
    return V[np.arange(n), :, k]


def triangulate_points(P1, P2, pts1, pts2, svd="lapack"):
    """cv2.triangulatePoints(P1, P2, pts1.T, pts2.T).T: homogeneous [n,4] (unit norm, sign arbitrary)"""
    A = dlt_matrices(P1, P2, pts1, pts2)
    if len(A) == 0:
        return np.empty((0, 4))
    if svd == "jacobi":
        return null_vectors_jacobi(A)
    return np.linalg.svd(A)[2][:, 3, :]


def parallax_deg(K_inv, R1, R2, uv1, uv2):
    """World-frame parallax in degrees (:54-77): each pixel's ray K^-1 (u, v, 1) turned into the world frame by R^T, divided
    by (norm + 1e-12); the angle between the two, cosine clipped to [-1, 1]."""
    def world_rays(R, uv):
        cam = np.column_stack([uv, np.ones(len(uv))]) @ K_inv.T
        wld = cam @ R                                   # rows (R^T cam)^T
        return wld / (np.linalg.norm(wld, axis=1, keepdims=True) + 1e-12)
    cosang = np.clip((world_rays(R1, uv1) * world_rays(R2, uv2)).sum(1), -1.0, 1.0)
    return np.degrees(np.arccos(cosang))


def _view(K, T, X, uv):
    """Depth in the view and reprojection error against uv (+inf where the point is not in front: z <= 1e-6), :195-209"""
    Xc = X @ T[:3, :3].T + T[:3, 3]
    z = Xc[:, 2]
    front = z > 1e-6
    e = np.full(len(X), np.inf)
    if front.any():
        proj = (Xc[front] / z[front, None]) @ K.T
        e[front] = np.linalg.norm(proj[:, :2] - uv[front], axis=1)
    return z, front, e


def triangulate_2view(pts1, pts2, K, T1, T2, min_depth=0.0, max_depth=1e6, use_parallax_gate=True, parallax_min_deg=2.0,
                      reproj_px_max=1.0, svd="lapack"):
    """pts1, pts2: float32 [n,2] as `pts_from_matches` returns them.  Returns (X [kept,3], kept_idx [kept], reason [n] int32,
    diag {"parallax_deg", "z1", "z2", "e1", "e2", "w": [n]}; NaN where the reference has no value)."""
    pts1 = np.asarray(pts1, np.float32).reshape(-1, 2)
    pts2 = np.asarray(pts2, np.float32).reshape(-1, 2)
    K = np.asarray(K, np.float64); T1 = np.asarray(T1, np.float64); T2 = np.asarray(T2, np.float64)
    n = len(pts1)
    reason = np.full(n, INVALID_W, np.int32)
    diag = {k: np.full(n, np.nan) for k in ("parallax_deg", "z1", "z2", "e1", "e2", "w")}
    none = (np.empty((0, 3)), np.empty(0, np.int32), reason, diag)
    if n == 0:
        return none
    X4 = triangulate_points(K @ T1[:3, :], K @ T2[:3, :], pts1.astype(np.float64), pts2.astype(np.float64), svd)
    w = X4[:, 3]
    diag["w"] = w.copy()
    valid = np.flatnonzero(np.isfinite(w) & (np.abs(w) > 1e-12))           # :154
    if use_parallax_gate:
        diag["parallax_deg"] = parallax_deg(np.linalg.inv(K), T1[:3, :3], T2[:3, :3], pts1.astype(np.float64),
                                            pts2.astype(np.float64))
    if len(valid) == 0:                                                     # :155-157
        return none
    X = X4[valid, :3] / w[valid, None]
    z1, front1, e1 = _view(K, T1, X, pts1[valid])
    z2, front2, e2 = _view(K, T2, X, pts2[valid])
    for name, val in (("z1", z1), ("z2", z2), ("e1", e1), ("e2", e2)):
        diag[name][valid] = val
    keep = []
    for o, m in enumerate(valid):                                           # the gate loop, one verdict per match (:211-249)
        if use_parallax_gate and float(diag["parallax_deg"][m]) < parallax_min_deg:
            reason[m] = LOW_PARALLAX
        elif not (min_depth <= float(z1[o]) <= max_depth and min_depth <= float(z2[o]) <= max_depth):
            reason[m] = BAD_DEPTH
        elif (not front1[o]) or (not front2[o]):
            reason[m] = BEHIND_CAM
        elif max(float(e1[o]), float(e2[o])) > reproj_px_max:
            reason[m] = HIGH_REPROJ
        else:
            reason[m] = KEPT
            keep.append(o)
    return X[keep].reshape(-1, 3), valid[keep].astype(np.int32), reason, diag
