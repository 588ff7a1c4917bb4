"""Synthetic keyframe pairs for the triangulation tests, on tests/two_view.py's geometry: KITTI `K`, its second view
(0.05 rad about y, `T_VIEW`), and a NON-IDENTITY first pose, so world and first-camera frame differ.

Every match is planted with the reason the gates of `triangulate_between_kfs_2view` must give it, decided here from the TRUE
geometry alone (the point, the two camera centres, the true depths) - never from the pixels or an SVD:

    kept          a point in front of both views, inside the depth window, true parallax above the gate
    low_parallax  a far point whose true parallax lies below the gate (every match of the near-pure-rotation pair)
    bad_depth     a near point (z < min_depth) with ample parallax; with the gate off also the far points beyond max_depth
    behind_cam    a point behind one or both cameras, in a scene whose min_depth is negative (with min_depth >= 0 the depth
                  window rejects such a point first, as in the reference)
    high_reproj   an outlier: a point with more than 4.5 degrees of parallax (over 50 px of disparity) whose second pixel is
                  moved 6 - 12 px ACROSS its epipolar line: that can only widen the angle between the rays, and against that
                  disparity it moves the triangulated depths by a fraction only
    invalid_w     rays that are parallel by construction: a translation-only pair (R2 == R1) and the SAME float32 pixel in
                  both views.  The first three columns of the two views' DLT rows are then bitwise equal, the null vector
                  is the point at infinity and the computed |w| is rounding noise (measured 1e-17 .. 1e-15 with LAPACK
                  and with the Jacobi port, against the 1e-12 test).  So yes: a zero w CAN be constructed from finite inputs.

Points are drawn by rejection until the true quantity clears its gate by a margin (0.05 degrees, 0.2 m), so no match sits on
a threshold.  The pixels handed to the code under test are float32 (what `pts_from_matches` returns); `p1_exact` /
`p2_exact` keep the float64 projections for the reference's own recovery test.
"""
import numpy as np

import two_view

K = two_view.K
ANG = 0.05
R_VIEW = np.array([[np.cos(ANG), 0, np.sin(ANG)], [0, 1, 0], [-np.sin(ANG), 0, np.cos(ANG)]])
KEPT, INVALID_W, LOW_PARALLAX, BAD_DEPTH, BEHIND_CAM, HIGH_REPROJ = range(6)
REASONS = ("kept", "invalid_w", "low_parallax", "bad_depth", "behind_cam", "high_reproj")

PARAMS = dict(min_depth=5.0, max_depth=100.0, use_parallax_gate=True, parallax_min_deg=1.0, reproj_px_max=1.0)


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def first_pose():
    T = np.eye(4)
    T[:3, :3] = _rot([0.2, 1.0, -0.1], 0.4)
    T[:3, 3] = [1.5, -0.7, 3.0]
    return T


def second_pose(T1, R=R_VIEW, t=two_view.T_VIEW):
    rel = np.eye(4)
    rel[:3, :3] = R
    rel[:3, 3] = t
    return rel @ T1


def _cam(T, Xw):
    return Xw @ T[:3, :3].T + T[:3, 3]


def _project(T, Xw):
    x = _cam(T, Xw) @ K.T
    return x[:, :2] / x[:, 2:]


def true_parallax_deg(T1, T2, Xw):
    """Angle between the two pixel rays through the true point: the ray of a pixel points AWAY from the camera, so for a point
    behind a camera it is the opposite of (X - C)."""
    out = []
    for T in (T1, T2):
        C = -T[:3, :3].T @ T[:3, 3]
        d = (Xw - C) * np.sign(_cam(T, Xw)[:, 2:3])
        out.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    return np.degrees(np.arccos(np.clip((out[0] * out[1]).sum(1), -1, 1)))


def planted_reason(T1, T2, Xw, outlier, P):
    par = true_parallax_deg(T1, T2, Xw)
    z1, z2 = _cam(T1, Xw)[:, 2], _cam(T2, Xw)[:, 2]
    r = np.full(len(Xw), KEPT, np.int32)
    r[outlier] = HIGH_REPROJ
    r[(z1 <= 1e-6) | (z2 <= 1e-6)] = BEHIND_CAM
    r[~((P["min_depth"] <= z1) & (z1 <= P["max_depth"]) & (P["min_depth"] <= z2) & (z2 <= P["max_depth"]))] = BAD_DEPTH
    if P["use_parallax_gate"]:
        r[par < P["parallax_min_deg"]] = LOW_PARALLAX
    return r


BOXES = {   # first-camera-frame boxes (x, y, z ranges) per kind
    "good": ((-15, 15), (-4, 4), (8, 60)),
    "far": ((-15, 15), (-4, 4), (60, 400)),
    "low": ((-15, 15), (-4, 4), (8, 60)),
    "wide": ((-15, 15), (-4, 4), (8, 30)),
    "near": ((-1.5, 1.5), (-0.5, 0.5), (1.5, 3.6)),
    "behind_one": ((-0.4, 0.4), (-0.2, 0.2), (-0.9, -0.2)),
    "behind_both": ((-4, 4), (-1, 1), (-12, -3)),
}


def _draw(rng, kind, n, T1, T2, P):
    """n world points of a kind, each clearing every gate it is judged by with a margin"""
    out = np.empty((0, 3))
    T1i = np.linalg.inv(T1)
    while len(out) < n:
        (x0, x1), (y0, y1), (z0, z1) = BOXES[kind]
        m = 4 * n + 16
        Xc = np.stack([rng.uniform(x0, x1, m), rng.uniform(y0, y1, m), rng.uniform(z0, z1, m)], 1)
        Xw = Xc @ T1i[:3, :3].T + T1i[:3, 3]
        par = true_parallax_deg(T1, T2, Xw)
        za, zb = _cam(T1, Xw)[:, 2], _cam(T2, Xw)[:, 2]
        gate = P["parallax_min_deg"] if P["use_parallax_gate"] else -1.0
        ok = np.abs(par - gate) > 0.05
        for z in (za, zb):
            ok &= (np.abs(z - P["min_depth"]) > 0.2) & (np.abs(z - P["max_depth"]) > 0.2) & (np.abs(z) > 0.05)
        if kind in ("good", "wide"):
            ok &= (par > (gate if kind == "good" else gate + 3.5)) & (za > P["min_depth"]) & (zb > P["min_depth"]) & (za < P["max_depth"]) & (zb < P["max_depth"])
        elif kind == "far":
            ok &= par < gate if P["use_parallax_gate"] else (za > P["max_depth"])
        elif kind == "low":
            ok &= par < gate
        elif kind == "near":
            ok &= (par > gate) & (za < P["min_depth"]) & (zb < P["min_depth"]) & (za > 0) & (zb > 0)
        elif kind == "behind_one":
            ok &= (par > gate) & (za < 0) & (zb > 0)
        elif kind == "behind_both":
            ok &= (par > gate) & (za < 0) & (zb < 0)
        out = np.concatenate([out, Xw[ok]])
    return out[:n]


def make_scene(name, counts, seed, params=None, T2=None, same_pixel=0):
    """counts: {kind: n} with kinds of BOXES plus "outlier".  `same_pixel`: that many extra matches with the same float32 pixel
    in both views (only meaningful with R2 == R1: the planted invalid_w)."""
    P = dict(PARAMS, **(params or {}))
    rng = np.random.default_rng(seed)
    T1 = first_pose()
    T2 = second_pose(T1) if T2 is None else T2
    parts, outl = [], []
    for kind, n in counts.items():
        parts.append(_draw(rng, "wide" if kind == "outlier" else kind, n, T1, T2, P))
        outl.append(np.full(n, kind == "outlier"))
    Xw = np.concatenate(parts) if parts else np.empty((0, 3))
    outlier = np.concatenate(outl) if outl else np.empty(0, bool)
    order = rng.permutation(len(Xw))
    Xw, outlier = Xw[order], outlier[order]
    p1, p2 = _project(T1, Xw), _project(T2, Xw)
    reason = planted_reason(T1, T2, Xw, outlier, P)
    if outlier.any():
        # across the epipolar line of p1 in view 2: l = F (p1, 1), F = K^-T [t]x R K^-1 of the relative pose
        rel = T2 @ np.linalg.inv(T1)
        t = rel[:3, 3]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Ki = np.linalg.inv(K)
        F = Ki.T @ tx @ rel[:3, :3] @ Ki
        l = np.column_stack([p1, np.ones(len(p1))]) @ F.T
        nrm = l[:, :2] / np.linalg.norm(l[:, :2], axis=1, keepdims=True)
        shift = rng.uniform(6, 12, len(p1)) * rng.choice([-1.0, 1.0], len(p1))
        p2 = np.where(outlier[:, None], p2 + nrm * shift[:, None], p2)
    exact = ~outlier
    if same_pixel:
        q = np.column_stack([rng.uniform(50, 1190, same_pixel), rng.uniform(20, 350, same_pixel)]).astype(np.float32).astype(np.float64)
        at = rng.choice(len(p1) + 1, same_pixel)
        p1 = np.insert(p1, at, q, axis=0); p2 = np.insert(p2, at, q, axis=0)
        Xw = np.insert(Xw, at, np.nan, axis=0)
        reason = np.insert(reason, at, INVALID_W); exact = np.insert(exact, at, False)
    return dict(name=name, K=K, T1=T1, T2=T2, params=P, pts1=p1.astype(np.float32), pts2=p2.astype(np.float32),
                p1_exact=p1, p2_exact=p2, X_true=Xw, exact=exact, reason=reason, baseline=True)


def _rotation_only_pair():
    T1 = first_pose()
    return second_pose(T1, t=1e-4 * two_view.T_VIEW)


def _translation_only_pair():
    T1 = first_pose()
    return second_pose(T1, R=np.eye(3), t=np.array([0.9, -0.1, 0.4]))


def all_scenes():
    """name -> scene.  Sizes: 0, 1, not a multiple of 64, one workgroup turn of each launch (256, 1024) and several, 4096."""
    S = [
        make_scene("clean_1024", dict(good=700, far=324), 11),
        make_scene("outliers30_1000", dict(good=500, far=200, outlier=300), 12),
        make_scene("near_rotation_300", dict(low=200, far=100), 13, T2=_rotation_only_pair()),
        make_scene("behind_700", dict(good=300, behind_one=150, behind_both=150, far=100), 14, params=dict(min_depth=-100.0)),
        make_scene("depth_window_517", dict(good=300, near=150, far=67), 15),
        make_scene("gate_off_900", dict(good=500, far=250, near=150), 16, params=dict(use_parallax_gate=False)),
        make_scene("empty_0", dict(), 17),
        make_scene("single_1", dict(good=1), 18),
        make_scene("odd_100", dict(good=60, far=20, near=10, outlier=10), 19),
        make_scene("turn_256", dict(good=200, outlier=56), 20),
        make_scene("turns_1025", dict(good=600, far=225, outlier=200), 21),
        make_scene("turns_2500", dict(good=1500, far=400, near=300, outlier=300), 22),
        make_scene("full_4096", dict(good=2400, far=800, near=296, outlier=600), 23),
        make_scene("parallel_rays_220", dict(good=150, far=50), 24, T2=_translation_only_pair(), same_pixel=20),
    ]
    S[2]["baseline"] = False                 # (no baseline: the points are not recoverable, only their verdict is)
    return {s["name"]: s for s in S}
