"""Synthetic two-view pairs with a PLANTED relative pose for the recoverPose / two-view-metrics tests: KITTI intrinsics
(tests/two_view.py's `K`), x2 = R x1 + t with |t| = 1 (an essential matrix knows no scale, so depths are in baselines and
`distance_thresh` = 50 means 50 baselines).

Every match is planted with what the vote of the TRUE candidate must say of it, decided from the true geometry alone:

    good      in front of both cameras, both depths inside (2, 40)
    far       in front of both, both depths inside (60, 120): beyond distance_thresh
    behind    behind both cameras (depths below -3): its pixels are valid, its triangulated depth negative
    mismatch  the second pixel is a random pixel of the image: no geometry, whatever the vote says

Good / far / behind points are drawn by rejection until their true parallax exceeds 0.1 degree (a point near the epipole of a
forward motion has none, and its depth would be rounding noise).  Mismatches are drawn in oversupply and only those are kept
that clear every comparison of every candidate with ten times the margin the GPU tests ask for, under LAPACK's SVD and the
Jacobi port alike - a mismatch has no planted verdict, so the only thing a test can ask of it is that its verdict is not a
coin toss.  E is built from the planted (R, t), or - `ransac` - from the project's own F-matrix RANSAC restatement
(oracle/ransac_ref.py) on the pixels, E = K^T F K; `negate` hands over -E, the same essential matrix.

`sel` (for the metrics) selects the matches that are not mismatches, with bytes 1 and 255 alternating, and one of them
cleared where needed so that the selected count has the parity the scene asks for.
"""
import numpy as np

import relative_pose_ref as R
import two_view
from oracle import ransac_ref

K = two_view.K
THRESH = 50.0
GOOD, FAR, BEHIND, MISMATCH = range(4)
KINDS = ("good", "far", "behind", "mismatch")

# what the GPU tests ask every match to clear (tests/test_relative_pose_gpu.py); scenes are built with ten times as much
MARGIN_S = 1e-9           # |Q2 Q3| of the unit-norm homogeneous point
MARGIN_Z0 = 1e-6          # a depth against 0
MARGIN_REL = 1e-6         # a depth against distance_thresh, relative
MARGIN_METRIC_Z = 1e-9    # z1, z2 of the metrics against 0


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


MOTIONS = {
    "forward": (_rot([0.2, 1.0, -0.1], 0.03), _unit([0.05, -0.02, -1.0])),
    "sideways": (_rot([0.0, 1.0, 0.0], 0.02), _unit([1.0, 0.05, 0.02])),
    "rotation": (_rot([0.1, 1.0, 0.2], 0.25), _unit([0.6, -0.1, 0.3])),
    "rotation_back": (_rot([0.1, 1.0, 0.2], 0.25), _unit([-0.6, 0.1, -0.3])),
    "backward": (_rot([0.2, 1.0, -0.1], 0.03), _unit([-0.05, 0.02, 1.0])),
}
RANGES = {GOOD: (2.0, 40.0), FAR: (60.0, 120.0), BEHIND: (-120.0, -3.0)}


def essential(Rm, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ Rm


def _project(X):
    x = X @ K.T
    return x[:, :2] / x[:, 2:]


def _draw(rng, kind, n, Rm, t):
    lo, hi = RANGES[kind]
    out = np.empty((0, 3))
    while len(out) < n:
        m = 4 * n + 16
        z = rng.uniform(lo, hi, m)
        X1 = np.stack([rng.uniform(-0.7, 0.7, m) * z, rng.uniform(-0.22, 0.22, m) * z, z], 1)
        X2 = X1 @ Rm.T + t
        C2 = -Rm.T @ t
        v2 = X1 - C2
        cos = (X1 * v2).sum(1) / (np.linalg.norm(X1, axis=1) * np.linalg.norm(v2, axis=1))
        ok = (X2[:, 2] > lo) & (X2[:, 2] < hi) & (np.degrees(np.arccos(np.clip(cos, -1, 1))) > 0.1)
        out = np.concatenate([out, X1[ok]])
    return out[:n]


def margins_clear(detail_margins, factor=1.0):
    """bool [n]: the match clears every comparison of every candidate (a non-finite value fails every comparison on
    both sides and clears them all)"""
    ok = None
    for m in detail_margins:
        c = np.abs(m["s"]) > factor * MARGIN_S
        for z in (m["z1"], m["z2"]):
            fin = np.isfinite(z)
            with np.errstate(invalid="ignore"):
                c &= ~fin | ((np.abs(z) > factor * MARGIN_Z0) & (np.abs(z - THRESH) > factor * MARGIN_REL * THRESH))
        ok = c if ok is None else ok & c
    return ok


def make_scene(name, n, motion, seed, mismatch=0.0, far=0.0, behind=0.0, mask01=False, ransac=False, noise=0.0,
               negate=False, parity=None):
    rng = np.random.default_rng(seed)
    Rm, t = MOTIONS[motion]
    n_mis = int(round(mismatch * n)); n_far = int(round(far * n)); n_beh = int(round(behind * n))
    n_good = n - n_mis - n_far - n_beh
    extra = 3 * n_mis + (8 if n_mis else 0)
    kinds = np.concatenate([np.full(n_good, GOOD), np.full(n_far, FAR), np.full(n_beh, BEHIND), np.full(n_mis + extra, MISMATCH)])
    X = np.concatenate([_draw(rng, k, c, Rm, t) for k, c in ((GOOD, n_good), (FAR, n_far), (BEHIND, n_beh))] +
                       [_draw(rng, GOOD, n_mis + extra, Rm, t)]) if n else np.empty((0, 3))
    p1 = _project(X)
    p2 = _project(X @ Rm.T + t)
    mis = kinds == MISMATCH
    p2[mis] = np.column_stack([rng.uniform(2, 1238, mis.sum()), rng.uniform(2, 373, mis.sum())])
    if noise:
        p1 = p1 + rng.normal(0, noise, p1.shape); p2 = p2 + rng.normal(0, noise, p2.shape)
    order = rng.permutation(len(X))
    X, kinds, p1, p2 = X[order], kinds[order], p1[order].astype(np.float32), p2[order].astype(np.float32)
    E = essential(Rm, t)
    if ransac:
        F, _, _ = ransac_ref.find_fundamental_ransac(p1, p2, 1.0, 0.99)
        assert F is not None
        E = K.T @ np.asarray(F, np.float64) @ K
    if negate:
        E = -E
    if n_mis:       # keep the mismatches whose verdicts are clear, under both SVDs; trim to n_mis of them
        clear = np.ones(len(X), bool)
        for svd in ("lapack", "jacobi"):
            clear &= margins_clear(R.recover_pose(E, p1, p2, K, THRESH, svd=svd)[4]["margins"], factor=10.0)
        keep = np.flatnonzero(kinds != MISMATCH)
        mis_ok = np.flatnonzero((kinds == MISMATCH) & clear)[:n_mis]
        assert len(mis_ok) == n_mis, (name, len(mis_ok), n_mis)
        idx = np.sort(np.concatenate([keep, mis_ok]))
        X, kinds, p1, p2 = X[idx], kinds[idx], p1[idx], p2[idx]
    assert len(p1) == n
    mask = (rng.uniform(size=n) < 0.8).astype(np.uint8) if mask01 else None
    sel = np.zeros(n, np.uint8)
    chosen = np.flatnonzero(kinds != MISMATCH)
    sel[chosen[0::2]] = 1; sel[chosen[1::2]] = 255
    if parity is not None and len(chosen) % 2 != parity and len(chosen):
        sel[chosen[len(chosen) // 2]] = 0
    return dict(name=name, n=n, motion=motion, K=K, R=Rm, t=t, E=E, pts1=np.ascontiguousarray(p1), pts2=np.ascontiguousarray(p2),
                kind=kinds, X_true=X, mask=mask, sel=sel, thresh=THRESH, noise_free=not (ransac or noise or n_mis),
                planted_E=not ransac)


def all_scenes():
    """name -> scene.  Match counts 0, 1, 2, either side of a wave (64) and of a workgroup (256), 600, and 4096 / 4097:
    several turns of the one-workgroup launches (1024 a turn) with and without a remainder."""
    S = [
        make_scene("empty_0", 0, "forward", 101),
        make_scene("single_1", 1, "sideways", 102),
        make_scene("pair_2", 2, "forward", 103, parity=0),
        make_scene("forward_63", 63, "forward", 104, far=0.2, behind=0.1, parity=1),
        make_scene("sideways_64", 64, "sideways", 105, far=0.2, parity=0, negate=True),
        make_scene("rotation_65", 65, "rotation", 106, far=0.15, behind=0.1, parity=1),
        make_scene("sideways_255", 255, "sideways", 107, mismatch=0.2, far=0.1, mask01=True, parity=0),
        make_scene("forward_256", 256, "forward", 108, mismatch=0.4, behind=0.05, parity=1, negate=True),
        make_scene("rotation_257", 257, "rotation", 109, mismatch=0.1, far=0.1, ransac=True, parity=0),
        make_scene("forward_600", 600, "forward", 110, mismatch=0.3, far=0.05, mask01=True, ransac=True, noise=0.3, parity=1),
        make_scene("sideways_4096", 4096, "sideways", 111, mismatch=0.25, far=0.1, parity=0),
        make_scene("rotation_4097", 4097, "rotation", 112, mismatch=0.05, far=0.1, behind=0.05, parity=1, negate=True),
        make_scene("rotation_back_300", 300, "rotation_back", 113, far=0.1, behind=0.2),
        make_scene("backward_300", 300, "backward", 114, far=0.3, behind=0.1, mask01=True),
    ]
    return {s["name"]: s for s in S}
