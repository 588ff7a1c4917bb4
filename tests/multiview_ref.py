"""CPU reference (numpy, float64) of N-view track triangulation as include/sslam_hip.h defines it
(`sslam_triangulate_tracks_host`), restated step by step:

    per view   P = K Tcw[:3]
    per track  V < 2: too_few_views.  Rows u P[2] - P[0], v P[2] - P[1] of its observations stack to A [2V, 4]; Xh = the unit
               right singular vector of A's smallest singular value; w not finite or |w| <= 1e-12: invalid_w.
               X = Xh[:3] / w, z_k = (Tcw_k X)[2].  Some z_k outside [min_depth, max_depth]: bad_depth.  Some z_k <= 1e-6:
               behind_cam.  The MEAN over the views of ||K (Tcw_k X) / z_k - (u_k, v_k)|| above max_rep_err: high_reproj.
               Otherwise kept.

The singular vector comes from `np.linalg.svd` of A itself (svd="lapack"), or (svd="qr_jacobi") from a float64 port of what
the GPU kernel runs: A folded row by row into its 4 x 4 triangular factor R by Givens rotations, then the one-sided Jacobi
of tests/triangulate_ref.py on R, the column of V under R's column of smallest norm.  Two correct evaluations of the same
arithmetic; their disagreement is the measured floor of the GPU tolerance (tests/test_multiview_gpu.py).

PARITY UNPINNED: the module whose contract this is (`slam.core.multi_view_utils` of the reference) is not in the reference's
tree; the definition is taken from the reference's tests of it and from its drivers' CLI help.
"""
import numpy as np

import triangulate_ref as _two_view

REASONS = ("kept", "too_few_views", "invalid_w", "bad_depth", "behind_cam", "high_reproj")
KEPT, TOO_FEW_VIEWS, INVALID_W, BAD_DEPTH, BEHIND_CAM, HIGH_REPROJ = range(6)


def dlt_rows(P, view, uv):
    """[M,2,4]: per observation the rows u P[2] - P[0], v P[2] - P[1] of its view"""
    Pv = P[view]
    uv = np.asarray(uv, np.float64)
    return np.stack([uv[:, 0:1] * Pv[:, 2] - Pv[:, 0], uv[:, 1:2] * Pv[:, 2] - Pv[:, 1]], axis=1)


def givens_triangular_factors(rows, off):
    """R [n,4,4] (row-major, upper) of every track's A, its rows folded in order: per row, for k = 0..3, the rotation
    (c, s) = (R[k,k], row[k]) / hypot(R[k,k], row[k]) zeroes row[k] (skipped when row[k] is 0).  All tracks advance one
    row at a time."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    A = rows.reshape(-1, 4)                                  # row 2 o + {0, 1} belongs to observation o
    lo, hi = 2 * off[:-1], 2 * off[1:]
    R = np.zeros((n, 4, 4))
    for step in range(int((hi - lo).max()) if n else 0):
        t = np.flatnonzero(lo + step < hi)
        row = A[lo[t] + step].copy()
        for k in range(4):
            act = row[:, k] != 0.0
            if not act.any():
                continue
            ta, ra = t[act], row[act]
            with np.errstate(all="ignore"):
                r = np.hypot(R[ta, k, k], ra[:, k])
                c, s = (R[ta, k, k] / r)[:, None], (ra[:, k] / r)[:, None]
            Rk = R[ta, k, k:].copy()
            R[ta, k, k:] = c * Rk + s * ra[:, k:]
            ra[:, k:] = c * ra[:, k:] - s * Rk
            row[act] = ra
    return R


def null_vectors(P, off, view, uv, svd):
    """[n,4] unit null vectors (NaN rows for tracks with fewer than two observations)"""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    Xh = np.full((n, 4), np.nan)
    V = np.diff(off)
    use = np.flatnonzero(V >= 2)
    if len(use) == 0:
        return Xh
    rows = dlt_rows(P, view, uv)
    if svd == "qr_jacobi":
        R = givens_triangular_factors(rows, off)
        Xh[use] = _two_view.null_vectors_jacobi(R[use])
    elif svd == "lapack":
        for i in use:
            Xh[i] = np.linalg.svd(rows[off[i]:off[i + 1]].reshape(-1, 4))[2][-1]
    else:
        raise ValueError(svd)
    return Xh


def triangulate_tracks(K, Tcw, track_off, obs_view, obs_uv, min_depth=0.40, max_depth=100.0, max_rep_err=2.0, svd="lapack"):
    """Returns (X [kept,3], kept_idx [kept] int32, reason [n] int32, diag {"mean_err", "z_min", "z_max", "w": [n]}; NaN
    where the definition has no value)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    Tcw = np.asarray(Tcw, np.float64).reshape(-1, 4, 4)
    off = np.asarray(track_off, np.int64)
    view = np.asarray(obs_view, np.int64)
    uv = np.asarray(obs_uv, np.float32).reshape(-1, 2).astype(np.float64)
    n = len(off) - 1
    reason = np.full(n, TOO_FEW_VIEWS, np.int32)
    diag = {k: np.full(n, np.nan) for k in ("mean_err", "z_min", "z_max", "w")}
    P = K @ Tcw[:, :3, :]
    Xh = null_vectors(P, off, view, uv, svd)
    Xall = np.full((n, 3), np.nan)
    for i in range(n):
        o0, o1 = off[i], off[i + 1]
        if o1 - o0 < 2:
            continue
        w = Xh[i, 3]
        diag["w"][i] = w
        if not (np.isfinite(w) and abs(w) > 1e-12):
            reason[i] = INVALID_W
            continue
        X = Xh[i, :3] / w
        Xall[i] = X
        T = Tcw[view[o0:o1]]
        Xc = T[:, :3, :3] @ X + T[:, :3, 3]
        z = Xc[:, 2]
        front = z > 1e-6
        e = np.full(len(z), np.inf)
        xn, yn = Xc[front, 0] / z[front], Xc[front, 1] / z[front]
        du = K[0, 0] * xn + K[0, 1] * yn + K[0, 2] - uv[o0:o1][front, 0]
        dv = K[1, 0] * xn + K[1, 1] * yn + K[1, 2] - uv[o0:o1][front, 1]
        e[front] = np.sqrt(du * du + dv * dv)
        mean = float(e.sum() / len(z))
        diag["mean_err"][i], diag["z_min"][i], diag["z_max"][i] = mean, z.min(), z.max()
        if not ((min_depth <= z) & (z <= max_depth)).all():
            reason[i] = BAD_DEPTH
        elif not front.all():
            reason[i] = BEHIND_CAM
        elif mean > max_rep_err:
            reason[i] = HIGH_REPROJ
        else:
            reason[i] = KEPT
    kept = np.flatnonzero(reason == KEPT).astype(np.int32)
    return Xall[kept].reshape(-1, 3), kept, reason, diag


def multi_view_triangulation(K, poses_w_c, pts2d, min_depth, max_depth, max_rep_err, svd="lapack"):
    """one track from camera-to-world poses, as the reference's tests call it: X [3] or None"""
    uv = np.asarray(pts2d, np.float32).reshape(-1, 2)
    Tcw = np.stack([np.linalg.inv(np.asarray(T, np.float64)) for T in poses_w_c]) if len(uv) else np.empty((0, 4, 4))
    X, kept, _, _ = triangulate_tracks(K, Tcw, [0, len(uv)], np.arange(len(uv)), uv, min_depth, max_depth, max_rep_err, svd)
    return X[0] if len(kept) else None
