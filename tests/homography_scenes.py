"""Planted planar two-view pairs for the homography RANSAC tests: KITTI intrinsics (tests/two_view.py's `K`), points on a
plane n . X = d seen from two poses, so that the pixels are related by H = K (R + t n^T / d) K^-1; a fraction of the
matches gets a random second pixel (a mismatch), the rest Gaussian pixel noise.

A GPU test can ask for IDENTICAL samples, iteration counts and masks only of inputs that are not coin tosses, so a scene is
accepted only when, on the CPU restatement alone (tests/homography_ref.py),
  * its LAPACK and its Jacobi variant agree on the winning sample, the iteration count, the inlier count and the mask, and
  * no match's error under the winning sample's model lies within 1e-3 relative of the squared threshold;
a draw that fails either is drawn again with another seed (never waived), and `attempts` records how often.  Every scene also
carries `reaches`: the branch it was built for, asserted on the restatement by `assert_reaches`.
"""
import numpy as np

import homography_ref as HR
import two_view

K = two_view.K
W, Hh = 1240.0, 375.0
THRESH = 1.5
MARGIN_REL = 1e-3
CHUNK_BOUNDS = (8, 128)            # the kernel's chunk bounds (csrc/homography_kernels.hip)


def _rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def plane_homography(R, t, nrm, d):
    H = K @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K)
    return H / H[2, 2]


PLANTED = plane_homography(_rot([0.1, 1.0, 0.05], 0.04), np.array([0.6, -0.05, 0.2]), np.array([0.1, 0.2, -1.0]) / np.linalg.norm([0.1, 0.2, -1.0]), -12.0)


def apply_h(H, p):
    q = np.column_stack([p, np.ones(len(p))]) @ H.T
    return q[:, :2] / q[:, 2:]


def _draw(n, seed, inlier_frac, noise, kind):
    rng = np.random.default_rng(seed)
    p1 = np.column_stack([rng.uniform(20, W - 20, n), rng.uniform(20, Hh - 20, n)])
    if kind == "line":                                   # every source point on one line: getSubset never accepts a draw
        p1[:, 1] = 0.25 * p1[:, 0] + 30.0
        p1 = np.round(p1 * 4) / 4
        p1[:, 1] = 0.25 * p1[:, 0] + 30.0                # (exact in float32: multiples of 1 / 16)
    p2 = apply_h(PLANTED, p1) + rng.normal(0, noise, (n, 2))
    n_in = n if inlier_frac >= 1 else int(round(inlier_frac * n))
    bad = rng.permutation(n)[n_in:]
    if kind == "mirror":                                 # the others follow a REFLECTED map: a draw that mixes the two fails the orientation test
        q = p1[bad].copy(); q[:, 0] = W - q[:, 0]
        p2[bad] = apply_h(PLANTED, q) + rng.normal(0, noise, (len(bad), 2))
    else:
        p2[bad] = np.column_stack([rng.uniform(0, W, len(bad)), rng.uniform(0, Hh, len(bad))])
    if kind == "degenerate4":                            # four source points with one x: runKernel returns no model
        p1[:, 0] = 100.0
    return np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)


def not_a_coin_toss(p1, p2, thresh, max_iters=2000):
    """(ok, lapack result, jacobi result): the two conditions of the module docstring"""
    rl = HR.find_homography_ransac(p1, p2, thresh, max_iters=max_iters, linalg="lapack")
    rj = HR.find_homography_ransac(p1, p2, thresh, max_iters=max_iters, linalg="jacobi")
    il, ij = rl[2], rj[2]
    same = all(il[k] == ij[k] for k in ("sample", "iterations", "inliers")) and (rl[1] is None) == (rj[1] is None)
    if same and rl[1] is not None:
        same = bool(np.array_equal(rl[1], rj[1]))
    clear = True
    for i in (il, ij):
        if i["err"] is not None:
            clear &= bool((np.abs(i["err"].astype(np.float64) - i["t"]) > MARGIN_REL * i["t"]).all())
    return same and clear, rl, rj


def make_scene(name, n, seed, inlier_frac=0.8, noise=0.2, kind="plane", reaches="", thresh=THRESH, max_iters=2000):
    for attempt in range(20):
        p1, p2 = _draw(n, seed + 7919 * attempt, inlier_frac, noise, kind)
        ok, rl, rj = not_a_coin_toss(p1, p2, thresh, max_iters)
        if ok:
            return dict(name=name, n=n, pts1=p1, pts2=p2, thresh=thresh, max_iters=max_iters, ref=rl, ref_jacobi=rj,
                        reaches=reaches, attempts=attempt + 1)
    raise AssertionError(f"{name}: no draw out of 20 is free of coin tosses")


def assert_reaches(s):
    """the branch the scene was built for, on the restatement alone"""
    H, mask, info = s["ref"]
    r = s["reaches"]
    if r == "direct":
        assert s["n"] == 4 and H is not None and mask.all() and info["iterations"] == 0
    elif r == "direct_none":
        assert s["n"] == 4 and H is None and info["inliers"] == -1
    elif r == "past_second_chunk":
        assert info["iterations"] > CHUNK_BOUNDS[1] and H is not None and 0.3 < info["inliers"] / s["n"] < 0.4
    elif r == "collapses_in_first_chunk":
        assert 0 < info["iterations"] < CHUNK_BOUNDS[0] and H is not None
    elif r == "orientation_rejects_first_draws":
        assert info["rejected_first"][1] >= 2 and H is not None
    elif r == "no_model":
        assert H is None and mask is None and info["iterations"] == 0 and info["rejected_collinear"] == HR.SUBSET_ATTEMPTS
    else:
        assert r == "model" and H is not None and s["n"] > 4 and info["inliers"] >= 4 and info["iterations"] >= 1


_CACHE = {}


def all_scenes():
    """name -> scene, built once per process.  Match counts 4 and 5, either side of a wave (64), of the scoring workgroup
    (256) and of one turn of the tail's workgroup (1024), the entry's bound 16384; then one scene per branch of the loop."""
    if _CACHE:
        return _CACHE
    S = [
        make_scene("four_4", 4, 201, 1.0, 0.0, reaches="direct"),
        make_scene("four_degenerate_4", 4, 202, 1.0, 0.0, kind="degenerate4", reaches="direct_none"),
        make_scene("five_5", 5, 203, 1.0, 0.05, reaches="model"),
        make_scene("plane_63", 63, 204, 0.7, reaches="model"),
        make_scene("plane_64", 64, 205, 0.8, reaches="model"),
        make_scene("plane_65", 65, 206, 0.6, reaches="model"),
        make_scene("plane_255", 255, 207, 0.7, reaches="model"),
        make_scene("plane_1023", 1023, 208, 0.6, reaches="model"),
        make_scene("plane_1024", 1024, 209, 0.8, reaches="model"),
        make_scene("plane_1025", 1025, 210, 0.7, reaches="model"),
        make_scene("plane_16384", 16384, 211, 0.8, reaches="model"),
        make_scene("sparse_600", 600, 212, 0.35, reaches="past_second_chunk"),
        make_scene("clean_600", 600, 213, 0.96, reaches="collapses_in_first_chunk"),
        make_scene("mirror_400", 400, 214, 0.6, kind="mirror", reaches="orientation_rejects_first_draws"),
        make_scene("line_50", 50, 215, 1.0, 0.0, kind="line", reaches="no_model"),
    ]
    _CACHE.update({s["name"]: s for s in S})
    return _CACHE
