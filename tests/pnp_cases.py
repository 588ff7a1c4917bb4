"""Cases for csrc/pnp_kernels.hip built around the places where the kernel decides: every sample's EPnP (A), the sample
loop at the chunk bounds of ransac_chunk_bounds(max_iters, 64) = [0, 8) [8, 64) [64, max_iters) (B), the strides of the
score / LM / tail / head loops and the LM's LDS limit (C), the LM's exits (D) and the closed threshold (E).

Every case is a plain dict of arrays; the restatement (oracle/pnp_ref.py, about 13 ms per sample) runs once per case and is
shared through functools.lru_cache - the arrays it returns are read-only.  tests/test_pnp_cases.py asserts, on the
restatement alone, that each case reaches the branch it is named for; tests/test_pnp_edges_gpu.py compares the kernel."""
import functools
import math

import numpy as np

import pnp_scenes as S
from oracle import pnp_ref as O

CONF, PX = S.CONF, S.RANSAC_PX
ANGLE_BAR = math.pi - 1e-3               # rodrigues_R2r is ill-conditioned past this rotation angle


@functools.lru_cache(maxsize=None)
def subsets(n, count):
    """The first `count` five-point subsets of the cv::RNG stream for n correspondences."""
    rng = O.CvRNG()
    out = []
    for _ in range(count):
        idx = []
        for _ in range(5):
            v = rng.uniform(0, n)
            while v in idx:
                v = rng.uniform(0, n)
            idx.append(v)
        out.append(tuple(idx))
    return tuple(out)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- A: every sample's EPnP ------------------------------------------------------------------------------------------------
def _scene_subsets(sc, count=64):
    p3, p2 = sc["pts3d"], sc["pts2d"]
    return [(p3[list(s)].copy(), p2[list(s)].copy()) for s in subsets(len(p3), count)]


def _fam_rand():
    return _scene_subsets(S.make_scene(301, 60, 0.3, "rand")), S.K_RAND


def _fam_kitti():
    return _scene_subsets(S.make_scene(302, 60, 0.3, "kitti")), S.KITTI_K


def _fam_clean():
    return _scene_subsets(S.make_scene(303, 60, 0.0, "rand", noise_px=0.0)), S.K_RAND


def _fam_duplicate():
    """One point twice (getSubset never draws this; the n == 5 branch takes what it is given)."""
    out = []
    for k, (p3, p2) in enumerate(_scene_subsets(S.make_scene(304, 60, 0.0, "rand"), 8)):
        i, j = k % 5, (k + 1 + k // 5) % 5
        p3[j], p2[j] = p3[i], p2[i]
        out.append((p3, p2))
    return out, S.K_RAND


def _fam_coplanar():
    """One world coordinate constant: exactly coplanar in float32, the projections as the scene has them."""
    out = []
    for k, (p3, p2) in enumerate(_scene_subsets(S.make_scene(305, 60, 0.0, "rand"), 9)):
        p3[:, k % 3] = np.float32(0.75 * (k // 3) - 0.5)
        out.append((p3, p2))
    return out, S.K_RAND


def _fam_collinear():
    """Five points on a line: along a world axis (two coordinates constant), then along a general direction."""
    out = []
    for k, (p3, p2) in enumerate(_scene_subsets(S.make_scene(306, 60, 0.0, "rand"), 8)):
        if k < 6:
            for ax in range(3):
                if ax != k % 3:
                    p3[:, ax] = p3[0, ax]
        else:
            d = np.array([0.5, -0.25, 1.0], np.float32)
            p3[:] = p3[0] + np.arange(5, dtype=np.float32)[:, None] * d        # (exact in float32: small dyadic steps)
        out.append((p3, p2))
    return out, S.K_RAND


def _fam_identical():
    out = []
    for k, (p3, p2) in enumerate(_scene_subsets(S.make_scene(307, 60, 0.0, "rand"), 2)):
        p3[:] = p3[0]
        if k == 1:
            p2[:] = p2[0]
        out.append((p3, p2))
    return out, S.K_RAND


FAMILIES = {"rand60": _fam_rand, "kitti60": _fam_kitti, "clean60": _fam_clean, "duplicate": _fam_duplicate,
            "coplanar": _fam_coplanar, "collinear": _fam_collinear, "identical": _fam_identical}
NAN_FAMILIES = ("coplanar", "collinear", "identical")


@functools.lru_cache(maxsize=None)
def family(name):
    """(subsets: tuple of (p3 [5,3] f32, p2 [5,2] f32), K)"""
    subs, K = FAMILIES[name]()
    return tuple(_frozen(p3, p2) for p3, p2 in subs), K


@functools.lru_cache(maxsize=None)
def family_restated(name):
    """Per subset of the family: (rvec, tvec, trace) of O.epnp_model."""
    subs, K = family(name)
    out = []
    for p3, p2 in subs:
        tr = {}
        r, t = O.epnp_model(p3, p2, K, tr)
        out.append(_frozen(r, t) + (tr,))
    return tuple(out)


def beyond_angle_bar(rvec):
    return bool(np.all(np.isfinite(rvec)) and np.linalg.norm(rvec) > ANGLE_BAR)


# ---- scenes with a chosen inlier set -----------------------------------------------------------------------------------------
def plant(n, h, good, seed):
    """`good` indices that hold sample h of the stream for n, such that no earlier sample lies wholly inside; None if the
    greedy fill does not get there."""
    subs = subsets(n, h + 1)
    inl = set(subs[h])
    earlier = [set(s) for s in subs[:h]]
    if any(e <= inl for e in earlier) or good < 5:
        return None
    rng = np.random.default_rng(seed)
    for c in rng.permutation([i for i in range(n) if i not in inl]):
        if len(inl) == good:
            break
        if not any(e <= inl | {int(c)} for e in earlier):
            inl.add(int(c))
    return sorted(inl) if len(inl) == good else None


def inlier_scene(seed, n, inliers, cam="rand", noise_px=0.0):
    """A scene of pnp_scenes with exactly the points `inliers` on their projections; the others anywhere in the image."""
    sc = S.make_scene(seed, n, 0.0, cam, noise_px=noise_px)
    W, H = (S.RAND_W, S.RAND_H) if cam == "rand" else (S.KITTI_W, S.KITTI_H)
    rng = np.random.default_rng(7000 + seed)
    p2 = sc["pts2d"].copy()
    out = np.ones(n, bool)
    out[list(inliers)] = False
    p2[out] = np.stack([rng.uniform(0, W, out.sum()), rng.uniform(0, H, out.sum())], 1).astype(np.float32)
    return dict(pts3d=sc["pts3d"], pts2d=p2, K=sc["K"], inlier=~out)


def _case(sc, iters, px=PX, **expect):
    c = dict(pts3d=sc["pts3d"], pts2d=sc["pts2d"], K=sc["K"], iters=iters, px=px, expect=expect)
    _frozen(c["pts3d"], c["pts2d"])
    return c


# ---- B: the sample loop at its chunk bounds ------------------------------------------------------------------------------------
PLANT_H = (0, 7, 8, 63, 64)             # the first sample, and both sides of the chunk bounds 8 and 64
PLANT_SEED = {0: 400, 7: 407, 8: 408, 63: 463, 64: 464}
MAX_ITERS = (0, 1, 7, 8, 9, 63, 64, 65)
# update_num_iters(0.999, (n - good) / n, 5, 300) for (n, good)
BUDGETS = {7: (11, 10), 8: (10, 9), 9: (9, 8), 63: (11, 7), 64: (30, 19), 65: (19, 12)}
BUDGET_SEED = {7: 507, 8: 508, 9: 509, 63: 563, 64: 564, 65: 565}


def _planted(h, iters):
    """n = 40, 12 inliers around sample h.  The full budget for the samples on the third chunk's bound, 100 for the others
    (the loop's behaviour after the winner does not depend on where the winner lies)."""
    sc = inlier_scene(PLANT_SEED[h], 40, plant(40, h, 12, PLANT_SEED[h]))
    return _case(sc, iters, sample=h, samples=max(iters, 1), inliers=12)


def _budget(b):
    n, good = BUDGETS[b]
    for h in range(6, -1, -1):                       # the latest winner before sample 7 that can be planted
        inl = plant(n, h, good, BUDGET_SEED[b])
        if inl is not None:
            return _case(inlier_scene(BUDGET_SEED[b], n, inl), S.ITERS, sample=h, samples=b, inliers=good)
    raise AssertionError(f"no winner before sample 7 can be planted for n = {n}, good = {good}")


def _four_inliers():
    sc = inlier_scene(601, 40, [3, 11, 22, 35])
    return _case(sc, 24, ok=False, samples=24)


def _five_inlier_winner():
    return _case(S.make_scene(FIVE_SEED, 60, 0.5, "rand"), 12, inliers=5)


def _six_points():
    return _case(inlier_scene(603, 6, [0, 1, 2, 3, 4, 5]), 20, inliers=6)


FIVE_SEED = 680
LOOP_CASES = {}
for _h in PLANT_H:
    LOOP_CASES[f"planted_h{_h}_full"] = functools.partial(_planted, _h, S.ITERS if _h >= 63 else 100)
    LOOP_CASES[f"planted_h{_h}_last"] = functools.partial(_planted, _h, _h + 1)
for _m in MAX_ITERS:
    LOOP_CASES[f"max_iters_{_m}"] = functools.partial(_planted, 0, _m)
for _b in BUDGETS:
    LOOP_CASES[f"budget_{_b}"] = functools.partial(_budget, _b)
LOOP_CASES["four_inliers"] = _four_inliers
LOOP_CASES["five_inlier_winner"] = _five_inlier_winner
LOOP_CASES["six_points"] = _six_points

# ---- C: sizes ----------------------------------------------------------------------------------------------------------------------
# host entry: the score loop strides by 64, the LM's sums by 256, the tail's mask by 1024; the LM reads LDS up to 3072 points
SIZES = (6, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3072, 3073)
SIZE_SEED = {n: 700 + i for i, n in enumerate(SIZES)}
SIZE_SEED[65] = 803                      # n = stride + 1: a seed whose point n - 1 the restated mask holds
LONE_LANE_SIZES = (65, 257, 1025, 3073)


def _size(n):
    """KITTI camera, 30 % outliers.  (n = 6: two outliers, no pose; 100 iterations of the full budget.)"""
    return _case(S.make_scene(SIZE_SEED[n], n, 0.3, "kitti"), S.ITERS if n > 6 else 100)


SIZE_CASES = {f"n{n}": functools.partial(_size, n) for n in SIZES}

# device entry: the head compacts by 1024
DEV_POINTS = (1023, 1024, 1025, 2049)
DEV_PATTERNS = ("all", "every_other", "past_1024", "four", "five")
# "past_1024" needs at least 6 slots there: 2049, and 1030 (exactly 6 in the head's second turn)
DEV_CASES = tuple((q, p) for q in DEV_POINTS for p in DEV_PATTERNS if p != "past_1024" or q >= 1030) + ((1030, "past_1024"),)


def association(n_points, pattern, seed=0):
    """kp_of_point [n_points] (-1: not associated), map points [n_points,3] float64, keypoints [*,2] float32 of a KITTI
    scene with 30 % outliers whose correspondences sit at the associated slots, the keypoints shuffled."""
    if pattern == "all":
        slots = np.arange(n_points)
    elif pattern == "every_other":
        slots = np.arange(1, n_points, 2)
    elif pattern == "past_1024":
        slots = np.arange(1024, n_points)
    else:
        k = {"four": 4, "five": 5}[pattern]
        slots = np.sort(np.array([0, n_points - 1, 511, n_points - 2, n_points // 2 + 1][:k]))
    m = len(slots)
    sc = S.make_scene(750 + seed, m, 0.3 if m >= 20 else 0.0, "kitti")     # (4, 5 or 6 correspondences: all inliers)
    rng = np.random.default_rng(751 + seed)
    kp = np.concatenate([sc["pts2d"], rng.uniform(0, 370, (17, 2)).astype(np.float32)])
    perm = rng.permutation(len(kp))
    kp_sh = np.empty_like(kp)
    kp_sh[perm] = kp
    kop = np.full(n_points, -1, np.int32)
    kop[slots] = perm[:m]
    xyz = rng.uniform(-5, 5, (n_points, 3))
    xyz[slots] = sc["pts3d"].astype(np.float64)
    return kop, xyz, kp_sh, sc


# ---- D: the LM ---------------------------------------------------------------------------------------------------------------------
DEGENERATE_H, DEGENERATE_SEED = 11, 816


def _degenerate_last():
    """The last sample the loop evaluates (h = iters - 1) is coplanar in the world: with a guess the LM starts at NaN."""
    sc = S.make_scene(DEGENERATE_SEED, 60, 0.5, "rand")
    p3 = sc["pts3d"].copy()
    p3[list(subsets(60, DEGENERATE_H + 1)[DEGENERATE_H]), 2] = np.float32(1.5)
    return _case(dict(pts3d=p3, pts2d=sc["pts2d"], K=sc["K"]), DEGENERATE_H + 1)


# Scenes (n = 100, 30 % outliers) whose every LM decision - accept / reject and stop - has a traced relative margin of at
# least LM_MARGIN, so that `lm_iters` is pinned: the kernel sums JtJ, JtErr and ||err||^2 in another order than numpy, an
# error of at most n 2^-53 < 1e-12 relative for n <= 6000.  Found by a search over 48 noisy and 200 noise-free seeds.
LM_MARGIN = 1e-9
LM_PINNED = {                            # name: (seed, camera, noise_px, guess, exit)
    "lm_cap_906": (906, "kitti", S.NOISE_PX, False, "cap"),
    "lm_cap_911": (911, "rand", S.NOISE_PX, False, "cap"),
    "lm_cap_guess_901": (901, "rand", S.NOISE_PX, True, "cap"),
    "lm_cap_guess_902": (902, "kitti", S.NOISE_PX, True, "cap"),
    "lm_step_2001": (2001, "rand", 0.0, False, "small_step"),
    "lm_step_2004": (2004, "kitti", 0.0, False, "small_step"),
    "lm_step_guess_2011": (2011, "rand", 0.0, True, "small_step"),
    "lm_step_guess_2040": (2040, "kitti", 0.0, True, "small_step"),
}
# noise-free, with a guess: lambda's exponent k climbs to its cap of 16 (10 of the 200 noise-free seeds do); its decisions
# at the convergence floor are rounding, so `lm_iters` is not pinned here
LM_K_CAP = {"lm_k_cap_2006": (2006, "kitti", 0.0, True, None)}


def _lm(seed, cam, noise_px):
    return _case(S.make_scene(seed, 100, 0.3, cam, noise_px=noise_px), S.ITERS)


LM_CASES = {"degenerate_last": _degenerate_last}
for _name, (_seed, _cam, _noise, _g, _exit) in {**LM_PINNED, **LM_K_CAP}.items():
    LM_CASES[_name] = functools.partial(_lm, _seed, _cam, _noise)

# ---- E: the threshold is closed ------------------------------------------------------------------------------------------------------
# Scene 1001 (n = 60, 30 % outliers): the winner's float32 error of point 23 is the square of a float32 pixel threshold,
# and the run at that threshold keeps the winner (sample 15).  Found at the second of at most 200 seeds.
THRESHOLD_SEED, THRESHOLD_POINT = 1001, 23


def _threshold_scene():
    return S.make_scene(THRESHOLD_SEED, 60, 0.3, "rand")


@functools.lru_cache(maxsize=None)
def threshold_px():
    """px32 with float32(float(px32) ** 2) == the error of THRESHOLD_POINT under the winner at PX, and the float32 below."""
    e = restated("threshold_base").err[THRESHOLD_POINT]
    px32 = np.float32(np.sqrt(e))
    return px32, np.nextafter(px32, np.float32(0))


THRESHOLD_CASES = {"threshold_base": lambda: _case(_threshold_scene(), S.ITERS),
                   "threshold_at": lambda: _case(_threshold_scene(), S.ITERS, px=float(threshold_px()[0])),
                   "threshold_below": lambda: _case(_threshold_scene(), S.ITERS, px=float(threshold_px()[1]))}

ALL_CASES = {**LOOP_CASES, **SIZE_CASES, **LM_CASES, **THRESHOLD_CASES}


@functools.lru_cache(maxsize=None)
def case(name):
    return ALL_CASES[name]()


class Restated:
    """What the restatement gives for a case: ok, rvec, tvec, mask, info, trace - and the winner's float32 errors."""

    def __init__(self, c, ok, r, t, mask, info, trace):
        self.ok, self.rvec, self.tvec, self.mask, self.info, self.trace = ok, r, t, mask, info, trace
        self.err = None
        if ok and info["sample"] >= 0:
            w = trace["winner"]
            self.err = O.reproj_err(c["pts3d"], c["pts2d"], w[0], w[1], c["K"])
            self.err.setflags(write=False)
        mask.setflags(write=False)


@functools.lru_cache(maxsize=None)
def restated(name, use_guess=False):
    """O.solve_pnp_ransac of the case.  With a guess only the refinement's start differs (the last sample instead of the
    winner, tests/test_oracle_pnp.py), so the sample loop of the no-guess run is reused."""
    c = case(name)
    if not use_guess:
        tr = {}
        ok, r, t, mask, info = O.solve_pnp_ransac(c["pts3d"], c["pts2d"], c["K"], c["px"], False, c["iters"], CONF, trace=tr)
        return Restated(c, ok, r, t, mask, info, tr)
    base = restated(name, False)
    if not base.ok:
        return base
    tr = dict(base.trace, lm={})
    last = tr["last"]
    X, m = c["pts3d"][base.mask].astype(np.float64), c["pts2d"][base.mask].astype(np.float64)
    r, t, lm_iters = O.refine_lm(X, m, last[0], last[1], c["K"], trace=tr["lm"])
    return Restated(c, True, r, t, base.mask.copy(), dict(base.info, lm_iters=lm_iters), tr)
