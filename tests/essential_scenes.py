"""Planted two-view pairs for the essential-matrix RANSAC tests: KITTI intrinsics (tests/two_view.py's `K`), 3-D points seen
from two poses related by a planted (R, t); a share of the matches gets a second pixel placed far from its epipolar line
(a mismatch, beyond ten times the threshold under the true E by construction), the rest bounded pixel noise well inside the
threshold.

A GPU test can ask for IDENTICAL samples, model indices, iteration counts and masks only of inputs that are not coin
tosses, so a scene is accepted only when, on the CPU restatement alone (tests/essential_ref.py),
  * its "lapack" and its "port" variant agree on the winning sample, the iteration count, the inlier count and the mask,
    and on E up to sign within 1e-6 (the two order a sample's models differently: two models of one sample that tie in
    their count would make them return different ones - a plane admits two essential matrices, so that does happen);
  * no match's error under the winning model lies within 1e-3 relative of the squared threshold;
a draw that fails either is drawn again with another seed (never waived); `attempts` records how often, and SEEDS below holds
the attempt that passed for every scene, so that building the scenes does not search again.  Every scene also carries
`reaches`: the branch it was built for, asserted on the restatement's own trace by `assert_reaches`.

Two branches the restatement does not show reachable, so no scene claims them: a sample without any model (no scene's
trace holds one: a tenth-degree polynomial from five generic matches keeps real roots), and the no-model exit
(info[0] = -1) for n >= 5 - copies of one match were tried, and every E that fits the one match then has all copies as
inliers, so a model is found.  That exit is left to the n < 5 path, which the Python wrapper answers.
"""
import numpy as np

import essential_ref as ER
import two_view

K = two_view.K
W, Hh = 1240.0, 375.0
THRESH = 1.0
PROB = 0.999
NOISE = 0.03                       # inlier noise, uniform in [-NOISE, NOISE] px
MARGIN_REL = 1e-3
E_AGREE = 1e-6
CHUNK_BOUNDS = (8, 128)            # the kernel's chunk bounds (csrc/essential_kernels.hip)


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


MOTIONS = {                        # name -> (R, t, planar)
    "general": (_rot([0.1, 1.0, 0.05], 0.05), np.array([0.3, -0.05, 1.1]), False),
    "forward": (_rot([0.2, 1.0, 0.1], 0.01), np.array([0.02, -0.01, 1.0]), False),      # a KITTI lost frame
    "sideways": (_rot([0.1, 1.0, -0.2], 0.03), np.array([1.0, 0.03, 0.02]), False),
    "plane": (_rot([0.1, 1.0, 0.05], 0.05), np.array([0.3, -0.05, 1.1]), True),
}


def true_essential(motion):
    R, t, _ = MOTIONS[motion]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return E / np.linalg.norm(E)


def e_err(E, Eref):
    """E against Eref up to sign (both of unit Frobenius norm), relative to max |Eref|"""
    E, Eref = np.asarray(E, np.float64), np.asarray(Eref, np.float64)
    return float(min(np.abs(E - Eref).max(), np.abs(E + Eref).max()) / np.abs(Eref).max())


def set_err(Es, Erefs):
    """two [3k, 3] stacks as SETS of models up to sign: the largest distance of a model to its nearest in the other stack"""
    A, B = np.asarray(Es).reshape(-1, 3, 3), np.asarray(Erefs).reshape(-1, 3, 3)
    if len(A) != len(B):
        return float("inf")
    d = np.array([[e_err(a, b) for b in B] for a in A])
    return float(max(d.min(1).max(), d.min(0).max()))


def exact_five(motion, seed):
    """five exact, normalised correspondences of the motion (float64, no pixel rounding)"""
    R, t, planar = MOTIONS[motion]
    rng = np.random.default_rng(seed)
    X = _points(rng, 5, planar)
    Y = X @ R.T + t
    return X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]


def _points(rng, n, planar):
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-4, 4, n), rng.uniform(8, 60, n)], 1)
    if planar:
        X[:, 2] = 25.0 + 0.4 * X[:, 0] - 1.5 * X[:, 1]
    return X


def _draw(n, seed, inlier_frac, motion):
    R, t, planar = MOTIONS[motion]
    rng = np.random.default_rng(seed)
    X = _points(rng, n, planar)
    x1 = (K @ X.T).T
    x2 = (K @ (X @ R.T + t).T).T
    p1 = x1[:, :2] / x1[:, 2:] + rng.uniform(-NOISE, NOISE, (n, 2))
    p2 = x2[:, :2] / x2[:, 2:] + rng.uniform(-NOISE, NOISE, (n, 2))
    n_in = n if inlier_frac >= 1 else int(round(inlier_frac * n))
    bad = rng.permutation(n)[n_in:]
    truth = np.ones(n, bool)
    truth[bad] = False
    Et = true_essential(motion)
    far = np.float32((10 * THRESH / K[0, 0]) ** 2)
    for i in bad:                                         # a mismatch: beyond ten times the threshold under the true E
        for tries in range(10000):
            q = np.array([rng.uniform(0, W), rng.uniform(0, Hh)])
            if tries >= 20:                               # (next to the epipole nothing is far: the first pixel moves too)
                p1[i] = [rng.uniform(0, W), rng.uniform(0, Hh)]
            e = ER.compute_error(ER.normalise(p1[i:i + 1], K), ER.normalise(q[None], K), Et)[0]
            if e > far:
                break
        p2[i] = q
    p1, p2 = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    return p1, p2, truth


def _agree(rl, rp, n):
    il, ip = rl[2], rp[2]
    same = all(il[k] == ip[k] for k in ("sample", "iterations", "inliers")) and (rl[0] is None) == (rp[0] is None)
    if same and rl[0] is not None:
        same = bool(np.array_equal(rl[1], rp[1]))
        same = same and (set_err(rp[0], rl[0]) if n == 5 else e_err(rp[0], rl[0])) <= E_AGREE
    return same


def _clear(info):
    if info["err"] is None:
        return True
    return bool((np.abs(info["err"].astype(np.float64) - info["t"]) > MARGIN_REL * info["t"]).all())


def not_a_coin_toss(s):
    """(ok, lapack result, port result): the two conditions of the module docstring"""
    a = (s["pts1"], s["pts2"], K, PROB, s["thresh"], s["max_iters"])
    rl = ER.find_essential_mat_ransac(*a, linalg="lapack")
    rp = ER.find_essential_mat_ransac(*a, linalg="port")
    return _agree(rl, rp, s["n"]) and _clear(rl[2]) and _clear(rp[2]), rl, rp


# name -> the attempt (seed + 7919 * attempt) that passed when the scenes were last searched
SEEDS = {"six_6": 3}


def make_scene(name, n, seed, inlier_frac=0.8, motion="general", reaches="model", thresh=THRESH, max_iters=1000):
    first = SEEDS.get(name, 0)
    for attempt in range(first, first + 20):
        p1, p2, truth = _draw(n, seed + 7919 * attempt, inlier_frac, motion)
        s = dict(name=name, n=n, pts1=p1, pts2=p2, thresh=thresh, max_iters=max_iters, motion=motion, truth=truth,
                 reaches=reaches, attempts=attempt + 1)
        ok, rl, rp = not_a_coin_toss(s)
        if ok:
            s.update(ref=rl, ref_port=rp)
            return s
    raise AssertionError(f"{name}: no draw out of 20 is free of coin tosses")


def assert_reaches(s):
    """the branch the scene was built for, on the restatement's own trace"""
    r = s["reaches"]
    for E, mask, info in (s["ref"], s["ref_port"]):
        it = info["iterations"]
        if r == "direct":
            assert s["n"] == 5 and E is not None and E.shape[0] == 3 * info["model"] >= 3 and mask.all() and it == 0
        elif r == "ends_in_first_chunk":
            assert 0 < it <= CHUNK_BOUNDS[0] and E is not None
        elif r == "ends_in_second_chunk":
            assert CHUNK_BOUNDS[0] < it <= CHUNK_BOUNDS[1] and E is not None
        elif r == "ends_in_third_chunk":
            assert CHUNK_BOUNDS[1] < it < s["max_iters"] and E is not None
        elif r == "exhausts_max_iters":
            assert it == s["max_iters"] > CHUNK_BOUNDS[1] and E is not None
        elif r == "later_model_beats_earlier":            # two models of ONE sample became the best, one after the other
            b = info["best"]
            assert any(b[k][0] == b[k + 1][0] and b[k][1] < b[k + 1][1] for k in range(len(b) - 1)) and E is not None
        else:
            assert r == "model" and E is not None and s["n"] > 5 and info["inliers"] >= 5 and it >= 1


_CACHE = {}


def all_scenes():
    """name -> scene, built once per process.  Match counts 5 (every model), 6 and 7 (the first real loops), either side of a
    wave (64), of the scoring workgroup (256) and of the tail's (1024), the entry's bound 16384 at a share at which the budget
    collapses within the first chunk; then one scene per branch of the loop."""
    if _CACHE:
        return _CACHE
    S = [
        make_scene("five_5", 5, 301, 1.0, "general", reaches="direct"),
        make_scene("six_6", 6, 302, 1.0, "forward"),
        make_scene("seven_7", 7, 303, 1.0, "sideways"),
        make_scene("general_63", 63, 304, 0.8, "general"),
        make_scene("forward_64", 64, 305, 0.8, "forward"),
        make_scene("sideways_65", 65, 306, 0.8, "sideways"),
        make_scene("plane_255", 255, 307, 0.8, "plane"),
        make_scene("general_256", 256, 308, 0.8, "general"),
        make_scene("forward_257", 257, 309, 0.8, "forward"),
        make_scene("sideways_1023", 1023, 310, 0.8, "sideways"),
        make_scene("plane_1024", 1024, 311, 0.8, "plane"),
        make_scene("general_1025", 1025, 312, 0.8, "general"),
        make_scene("forward_16384", 16384, 313, 0.97, "forward", reaches="ends_in_first_chunk"),
        make_scene("clean_600", 600, 314, 0.96, "general", reaches="ends_in_first_chunk"),
        make_scene("second_600", 600, 315, 0.7, "forward", reaches="ends_in_second_chunk"),
        make_scene("third_600", 600, 316, 0.5, "general", reaches="ends_in_third_chunk"),
        make_scene("sparse_300", 300, 317, 0.3, "forward", reaches="exhausts_max_iters", max_iters=150),
        make_scene("two_roots_400", 400, 318, 0.7, "general", reaches="later_model_beats_earlier"),
    ]
    _CACHE.update({s["name"]: s for s in S})
    return _CACHE
