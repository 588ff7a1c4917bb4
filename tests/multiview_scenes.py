"""Synthetic multi-view scenes for tests/test_multiview_ref.py, test_multiview_gpu.py and test_multi_view_utils_gpu.py.

`rig()` is 33 views: centres along x over 2 m with a little y / z wander, small rotations, view 1 with view 0's rotation
(a translation-only pair) and view 16 pushed 3 m forward (so a point can lie behind ONE camera).  Every track is planted
with the reason the definition must give it, decided here from the TRUE geometry alone - never from an SVD:

    kept           a point 4 - 6 m ahead, 0.4 px noise, 2 / 3 / 5 / 33 views at least 8 views (0.5 m) apart
    too_few_views  one observation
    invalid_w      rays that are parallel by construction: views 0 and 1 (same rotation, different centres) and the SAME
                   float32 pixel in both.  The first three columns of the two views' DLT rows are bitwise equal, the null
                   vector is the point at infinity and the computed |w| is rounding noise.  (A pair that differs by a pure
                   ROTATION sharing one ray cannot give this verdict: its rays meet in the common centre, the null vector
                   is that centre with w = 1 / sqrt(|C|^2 + 1), and the verdict is bad_depth at z = 0.)
    bad_depth      a noise-free point 150 - 200 m ahead, beyond max_depth; and, in the scene whose min_depth is 0, a point
                   behind view 16 (z = -1 there): by the definition's order the window [0, max_depth] rejects it first
    behind_cam     the same point behind view 16 in the scene whose min_depth is -100: reachable only with min_depth <= 1e-6
    high_reproj    a kept-style point of 2 / 3 / 5 views, one observation moved 40 px across the baseline
"""
import numpy as np

K = np.array([[800.0, 0.0, 320.0], [0.0, 800.0, 240.0], [0.0, 0.0, 1.0]])
F = 33
FORWARD_VIEW = 16
KEPT, TOO_FEW_VIEWS, INVALID_W, BAD_DEPTH, BEHIND_CAM, HIGH_REPROJ = range(6)
PARAMS = dict(min_depth=0.40, max_depth=100.0, max_rep_err=2.0)
VIEW_COUNTS = (2, 3, 5, 33, 1)


def _rot_x(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def rig():
    """(poses_w_c [F,4,4] camera-to-world, Tcw [F,4,4])"""
    poses = np.tile(np.eye(4), (F, 1, 1))
    for k in range(F):
        kr = 0 if k == 1 else k
        poses[k, :3, :3] = _rot_y(0.03 * np.sin(0.9 * kr)) @ _rot_x(0.02 * np.cos(1.3 * kr))
        poses[k, :3, 3] = (2.0 * k / (F - 1), 0.1 * np.sin(k), 0.05 * np.cos(1.7 * k) + (3.0 if k == FORWARD_VIEW else 0.0))
    return poses, np.stack([np.linalg.inv(T) for T in poses])


POSES, TCW = rig()


def project(X, views):
    Xc = np.einsum("vij,j->vi", TCW[views, :3, :3], X) + TCW[views, :3, 3]
    return (Xc[:, :2] / Xc[:, 2:3]) @ K[:2, :2].T + K[:2, 2], Xc[:, 2]


def _spread_views(rng, V, must=None):
    """V distinct views in random order, the lowest and highest at least 8 apart, never the translation-only pair alone"""
    if V >= F:
        return rng.permutation(F)
    while True:
        v = rng.choice(F, V, replace=False)
        if must is not None:
            v[0] = must
        if len(set(v.tolist())) == V and v.max() - v.min() >= 8:
            return v


def make_scene(name, n, seed, params=None, behind=False, pair_only=None):
    """n tracks.  `behind`: every 9th track is the point behind view 16.  `pair_only` = (a, b): every track is a 2-view
    track of those views (for the comparison with the two-view entry)."""
    P = dict(PARAMS, **(params or {}))
    rng = np.random.default_rng(seed)
    off, view, uv, reason, X_true = [0], [], [], [], []
    for i in range(n):
        V = VIEW_COUNTS[i % len(VIEW_COUNTS)]
        kind = "good"
        if pair_only is not None:
            V = 2
            kind = "far" if i % 7 == 3 else "outlier" if i % 7 == 5 else "good"
        elif n == 1:
            V = 3
        elif V == 1:
            kind = "one_view"
        elif i % 37 == 5:
            kind = "parallel"
        elif behind and i % 9 == 2:
            kind = "behind"
        elif i % 11 == 3:
            kind = "far"
        elif i % 11 == 7 and V <= 5:
            kind = "outlier"
        X = np.array([rng.uniform(0.0, 2.0), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 6.0)])
        if kind == "one_view":
            v = rng.choice(F, 1)
            p, _ = project(X, v)
            p = p + rng.normal(0, 0.4, p.shape)
            r = TOO_FEW_VIEWS
        elif kind == "parallel":
            v = np.array([0, 1])
            p = np.tile(np.float32([rng.uniform(50, 590), rng.uniform(50, 430)]), (2, 1))
            X = np.full(3, np.nan)
            r = INVALID_W
        elif kind == "behind":
            X = np.array([1.0 + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 2.0])       # 2 m ahead of the row, 1 m behind view 16
            v = _spread_views(rng, 3, must=FORWARD_VIEW)
            p, z = project(X, v)
            assert (z < 0).sum() == 1
            r = BEHIND_CAM if P["min_depth"] < -50 else BAD_DEPTH
        else:
            if kind == "far":
                X[2] = rng.uniform(150.0, 200.0)
            v = np.array(pair_only) if pair_only is not None else _spread_views(rng, V)
            p, z = project(X, v)
            assert (z > 0.5).all()
            if kind != "far":
                p = p + rng.normal(0, 0.4, p.shape)
            if kind == "outlier":
                p[rng.integers(len(v)), 1] += 40.0
            r = {"good": KEPT, "far": BAD_DEPTH, "outlier": HIGH_REPROJ}[kind]
        off.append(off[-1] + len(v)); view.extend(v.tolist()); uv.append(np.asarray(p, np.float64)); reason.append(r); X_true.append(X)
    return dict(name=name, K=K, Tcw=TCW, params=P, off=np.array(off, np.int32), view=np.array(view, np.int32),
                uv=(np.concatenate(uv) if uv else np.empty((0, 2))).astype(np.float32).reshape(-1, 2),
                reason=np.array(reason, np.int32), X_true=np.array(X_true).reshape(-1, 3), pair_only=pair_only)


def all_scenes():
    """name -> scene.  Sizes: 0, 1, one workgroup of the track launch less one / exactly / plus one (255, 256, 257) and more
    than one turn of the 1024-wide tail (1025); views per track 1, 2, 3, 5 and 33 mixed inside every call."""
    S = [
        make_scene("empty_0", 0, 40),
        make_scene("single_1", 1, 41),
        make_scene("mixed_255", 255, 42),
        make_scene("mixed_256", 256, 43),
        make_scene("mixed_257", 257, 44),
        make_scene("mixed_1025", 1025, 45),
        make_scene("behind_min0_257", 257, 46, params=dict(min_depth=0.0), behind=True),
        make_scene("behind_minneg_130", 130, 47, params=dict(min_depth=-100.0), behind=True),
        make_scene("pairs_300", 300, 48, pair_only=(0, 12)),
    ]
    return {s["name"]: s for s in S}


# ---- the scenes of the reference's own tests of the lost module, rebuilt from their parameters --------------------------
def translated_pose(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


def observe(Kc, poses_w_c, X, rng=None, noise_px=0.0):
    """[V,2] float32 pixels of world point X in camera-to-world poses, Gaussian pixel noise from `rng`"""
    out = []
    for T in poses_w_c:
        pc = (np.linalg.inv(T) @ np.append(X, 1.0))[:3]
        p = (Kc @ pc)[:2] / pc[2]
        if rng is not None:
            p = p + rng.normal(0.0, noise_px, 2)
        out.append(p)
    return np.float32(out)


def five_view_scene(seed, n_views=5, n_pts=40, noise_px=0.4):
    """(K, poses_w_c, pts_w [n_pts,3], pts2d: per view [n_pts,2] float32): views translated 0 - 1 m along x, points in
    [-1,1]^2 x [4,6], K 800 / 320 / 240"""
    rng = np.random.default_rng(seed)
    poses = [translated_pose(t) for t in np.linspace(0.0, 1.0, n_views)]
    pts_w = np.column_stack([rng.uniform(-1, 1, n_pts), rng.uniform(-1, 1, n_pts), rng.uniform(4, 6, n_pts)])
    pts2d = []
    for T in poses:
        Tcw = np.linalg.inv(T)
        Xc = pts_w @ Tcw[:3, :3].T + Tcw[:3, 3]
        p = (Xc[:, :2] / Xc[:, 2:3]) @ K[:2, :2].T + K[:2, 2]
        pts2d.append((p + rng.normal(0.0, noise_px, p.shape)).astype(np.float32))
    return K, poses, pts_w, pts2d
