"""The device LM (csrc/ba_lm.hip) at the sizes and exits where it switches, against the single-Jacobian oracle
(oracle/ba_ref.solve_dense_lm, scipy.sparse form): MAX_PO = 12 (reduced system in LDS / in device memory), a large
global problem, every exit of the loop the oracle can be driven to on both solver paths, rejected steps on the big
path, structure edges (a point seen only from constant poses, a point nobody observes, constant points and Huber
outliers on the big path, a residual exactly on the Huber threshold) and the 256-thread blocks of the reductions.

Comparison as in test_ba_lm_gpu: identical `iterations`, `successful_steps`, `termination`; `initial_cost` at rtol 1e-12;
`final_cost` and parameters at the tolerances that file uses for the same scene generator and solver path (LDS: its
C3-size test, device memory: its global-BA test).  Every scene built for an exit first asserts the oracle's exit.

Exits: "function tolerance" (a noisy scene run to convergence), "parameter tolerance" (the noisy scene, landmarks
constant, re-solved from its own solution until the first step is below 1e-8 of the parameters' norm) and "gradient
tolerance" are reached.  The gradient bound of Ceres is absolute (1e-10), and with pixel-scale residuals one ulp of a
600 px coordinate times a Jacobian entry of ~700 is already 1e-10: the oracle and the kernel could disagree by rounding alone.  The converged scene for that exit is
therefore expressed in normalised image coordinates (fx = fy = 1, cx = cy = 0) with every observation set to the
oracle's own projection, where the gradient is ~1e-16 whatever the summation order.

Left out - "trust region collapsed": the radius falls from 1e4 below 1e-32 only after 15 consecutive rejected steps
(divisors 2, 4, 8, ...).  A rejected step shortens the next one, and a step below 1e-8 of the parameters' norm ends the
loop with "parameter tolerance" first; where the candidate's residuals are non-finite (a point stepping through a camera
plane) the shorter step that follows is finite again.  The oracle was not driven to that exit, so `done = 4` is not
compared.

Left out - the LANDMARKS of a large problem run to convergence, and 128 free poses.  The device path walks the oracle's
trajectory there too (64 free poses: 22 iterations, 22 steps, "function tolerance" on both sides; 128 free poses, 10
iterations: same counts, final cost equal to 3.8e-11), but the parameters miss the fixed bars of test_ba_lm_gpu (at 128
poses after 10 iterations, t by 2.7 x).  The reason is the scene, not the summation order alone: a landmark seen twice
under a small baseline is free along its ray, and by the time the function-tolerance exit stops, such landmarks have
run thousands of metres.  The oracle's own two forms show it: at 64 free poses converged, dense against sparse=True
(measured once on the CPU, 91 s against 6 s) agree on iterations / steps / exit, differ by 8.6e-10 relative in final
cost, 2.6e-8 in q, 2.5e-4 in t - and by 2.7e4 in X (4.8 % relative).  Ten times that is no bar for X, so the converged
64-pose case below compares the trajectory, the cost, q and t at 10 x those disagreements and not X; the landmarks of a
large problem are compared after 10 iterations (test_large_global_problem, fixed bars), and convergence including the
landmarks at 14 free poses on the device-memory path ("big" exit cases).  256 poses are tested for acceptance only."""
import copy
import time

import numpy as np
import pytest

import ba_scenes
from conftest import load_pkg
from oracle import ba_ref

pytestmark = pytest.mark.gpu

# (final_cost rtol, q (rtol, atol), t (rtol, atol), X (rtol, atol)) - test_ba_lm_gpu.py, per solver path
TOL_LDS = (1e-8, (1e-7, 1e-8), (1e-7, 1e-7), (1e-6, 1e-6))      # test_device_lm_matches_oracle_at_c3_size_and_is_deterministic
TOL_BIG = (1e-8, (1e-7, 1e-8), (1e-7, 1e-7), (1e-4, 1e-3))      # test_global_ba_shape_on_the_device_and_in_the_host_loop_...
MAX_PO = 12                                                      # csrc/ba_lm.hip


@pytest.fixture(scope="module")
def S():
    return load_pkg("ba_solver")


def _window(n_kf, n_points, opt, fix, **scene):
    bau = load_pkg("slam.core.ba_utils")
    wmap, kfs, K = ba_scenes.scaled_scene(n_kf=n_kf, n_points=n_points, **scene)
    prob, _, _ = bau.snapshot_problem(wmap, K, kfs, list(opt), list(fix), 10 ** 6)
    return prob


def _free(prob):
    return int(np.count_nonzero(~np.asarray(prob.pose_const, bool)))


def _oracle(prob, iters, points_const=False, delta=2.0):
    return ba_ref.solve_dense_lm(prob.q, prob.t, prob.pose_const, prob.X, prob.intr, prob.obs_pose, prob.obs_point,
                                 prob.obs_uv, iters, delta, points_const, sparse=True)


def _zero_cost_floor(prob):
    """For the gradient-tolerance scene ONLY, whose cost is zero to rounding (0.0 in the oracle: every observation is its
    own projection): a relative bound on 0 admits nothing but 0, and another correct evaluation order of the projection
    leaves residuals of an ulp.  With d = 2 ulp of the largest coordinate per residual component the cost stays below
    2 n d^2: coordinates below 1 in normalised image units, d = 2.2e-16, n = 2 900 observations -> 2.8e-28 absolute (the
    pixel-scale costs of every other scene are 1e3: 3e-31 of them).  Every other scene is compared with the plain
    relative bounds, floor 0."""
    d = 2 * np.spacing(float(np.abs(prob.obs_uv).max()))
    return 2 * len(prob.obs_pose) * d * d


def _same(summ, got, ref, prob, tol, what="", floor=False):
    q, t, X, info = ref
    print(f"\n[{what}] oracle {info['iterations']} it / {info['successful_steps']} ok / {info['termination']}; "
          f"got {summ.iterations} / {summ.successful_steps} / {summ.termination}; "
          f"cost {summ.final_cost!r} vs {info['final_cost']!r}")
    assert (summ.iterations, summ.successful_steps, summ.termination) == (
        info["iterations"], info["successful_steps"], info["termination"]), what
    np.testing.assert_allclose(summ.initial_cost, info["initial_cost"], rtol=1e-12,
                               atol=_zero_cost_floor(prob) if floor else 0.0, err_msg=what)
    np.testing.assert_allclose(summ.final_cost, info["final_cost"], rtol=tol[0],
                               atol=_zero_cost_floor(prob) if floor else 0.0, err_msg=what)
    np.testing.assert_allclose(got.q, q, rtol=tol[1][0], atol=tol[1][1], err_msg=what)
    np.testing.assert_allclose(got.t, t, rtol=tol[2][0], atol=tol[2][1], err_msg=what)
    np.testing.assert_allclose(got.X, X, rtol=tol[3][0], atol=tol[3][1], err_msg=what)
    # constant blocks are bit-for-bit untouched
    np.testing.assert_array_equal(got.q[prob.pose_const], prob.q[prob.pose_const])
    np.testing.assert_array_equal(got.t[prob.pose_const], prob.t[prob.pose_const])


def _parity(S, prob, iters, ref=None, points_const=False, host=False, what="", floor=False):
    """solve_device (and solve_host) against the oracle; the tolerance set follows the solver path."""
    ref = ref or _oracle(prob, iters, points_const)
    tol = TOL_BIG if _free(prob) > MAX_PO else TOL_LDS
    dev = copy.deepcopy(prob)
    _same(S.solve_device(dev, iters, 2.0, points_const=points_const), dev, ref, prob, tol, what + " device", floor)
    if host:
        h = copy.deepcopy(prob)
        _same(S.solve_host(h, iters, 2.0, points_const=points_const), h, ref, prob, tol, what + " host", floor)
    return ref[3], dev


# ---- MAX_PO ----------------------------------------------------------------------------------------------------------
WINDOWS = {1: ([14], range(9, 14)), 12: (range(3, 15), range(0, 3)), 13: (range(2, 15), range(0, 2))}


@pytest.mark.parametrize("po", [1, 12, 13], ids=lambda p: f"po-{p}")
def test_free_pose_counts_around_the_lds_limit(S, po):
    """12 free poses: the last reduced system factored in LDS; 13: the first in device memory.  There also the host Schur
    loop: all three walk the oracle's trajectory."""
    prob = _window(15, 600, *WINDOWS[po])
    assert _free(prob) == po
    info, _ = _parity(S, prob, 12, host=po >= 12, what=f"po-{po}")
    assert info["final_cost"] < 0.5 * info["initial_cost"]


# ---- a large global problem ------------------------------------------------------------------------------------------
def test_large_global_problem(S):
    """64 free poses, two gauge keyframes, 1500 landmarks, 8 651 observations, 10 iterations as the suite's other global
    case: the sparse oracle takes 1 - 3 s for it on the CPU (a minute would allow far more poses; what bounds the size
    is the comparison, see the module docstring)."""
    prob = _window(66, 1500, range(66), [0, 1])
    assert _free(prob) == 64
    t0 = time.perf_counter()
    ref = _oracle(prob, 10)
    print(f"\n[po-64] sparse oracle {time.perf_counter() - t0:.1f} s, {len(prob.obs_pose)} observations, {ref[3]}")
    assert ref[3]["successful_steps"] >= 8 and ref[3]["final_cost"] < 0.2 * ref[3]["initial_cost"]
    _parity(S, prob, 10, ref=ref, what="po-64")


def test_large_global_problem_to_convergence(S):
    """The same 64 free poses until the oracle stops on the function tolerance (22 iterations).  This scene is genuinely
    ill-conditioned at convergence (module docstring), so the bars are 10 x the disagreement of the oracle's own two
    forms, dense against sparse=True, measured on the CPU:
        final_cost  8.6e-10 relative -> rtol 8.6e-9
        q           2.6e-8 absolute  -> atol 2.6e-7
        t           2.5e-4 absolute  -> atol 2.5e-3
        X           2.7e4 absolute (4.8 % relative): no bar can be derived, not compared."""
    prob = _window(66, 1500, range(66), [0, 1])
    q, t, X, info = _oracle(prob, 60)
    assert info["termination"] == "function tolerance" and info["iterations"] > 12
    dev = copy.deepcopy(prob)
    summ = S.solve_device(dev, 60, 2.0)
    print(f"\n[po-64 converged] oracle {info}; got {summ}; |dq| {np.abs(dev.q - q).max():.3g} |dt| {np.abs(dev.t - t).max():.3g}")
    assert (summ.iterations, summ.successful_steps, summ.termination) == (
        info["iterations"], info["successful_steps"], info["termination"])
    np.testing.assert_allclose(summ.initial_cost, info["initial_cost"], rtol=1e-12)
    np.testing.assert_allclose(summ.final_cost, info["final_cost"], rtol=8.6e-9)
    np.testing.assert_allclose(dev.q, q, rtol=0, atol=2.6e-7)
    np.testing.assert_allclose(dev.t, t, rtol=0, atol=2.5e-3)
    assert np.isfinite(dev.X).all()
    np.testing.assert_array_equal(dev.q[prob.pose_const], prob.q[prob.pose_const])


def test_256_free_poses_are_accepted_and_257_refused(S, native):
    prob = _window(258, 3000, range(258), [0, 1])
    assert _free(prob) == 256 == S.MAX_DEVICE_POSES
    a, b = copy.deepcopy(prob), copy.deepcopy(prob)
    sa, sb = S.solve_device(a, 4, 2.0), S.solve_device(b, 4, 2.0)
    assert sa.iterations == 4 and np.isfinite(sa.final_cost) and sa.final_cost <= sa.initial_cost
    assert sa.successful_steps >= 1 and sa.final_cost < sa.initial_cost
    for arr in (a.q, a.t, a.X):
        assert np.isfinite(arr).all()
    assert sa == sb
    for x, y in ((a.q, b.q), (a.t, b.t), (a.X, b.X)):
        np.testing.assert_array_equal(x, y)                                 # bit-reproducible
    over = _window(258, 3000, range(258), [0])
    assert _free(over) == 257
    with pytest.raises(native.NativeError, match="optimised poses"):
        S.solve_device(over, 4, 2.0)


# ---- every exit ------------------------------------------------------------------------------------------------------
PATHS = {"lds": (range(5, 15), range(0, 5)), "big": (range(1, 15), [0])}
CLEAN = dict(pix_noise=0.0, point_noise=0.0, rot_noise_deg=0.0, trans_noise=0.0)


def _exit_scene(path, exit_):
    opt, fix = PATHS[path]
    if exit_ == "function tolerance":
        return _window(15, 300, opt, fix), 100
    if exit_ == "parameter tolerance":
        # the noisy scene (residuals of pixels, so the plain relative bounds on the cost apply), landmarks constant,
        # re-solved from its own solution until the FIRST step is below 1e-8 |x|: that test comes before the step is
        # evaluated, so the loop ends in iteration 1 with no step taken.  Each re-solve ends after one step with "function
        # tolerance" and shortens the next step to ~0.56 of the last (2.2e-4, 1.2e-4, ... measured on the CPU); the
        # first one under the bound (5.4e-6) is at ~0.7 of it, 9 re-solves in
        prob = _window(15, 300, opt, fix)
        for _ in range(30):
            q, t, _, info = _oracle(prob, 100, points_const=True)
            if info["termination"] == "parameter tolerance":
                break
            prob.q[:] = q; prob.t[:] = t
        return prob, 20
    prob = _window(15, 300, opt, fix, **CLEAN)
    if exit_ == "gradient tolerance":
        # the converged scene in normalised image coordinates, every observation at its own projection (module docstring)
        prob.intr = np.array([1.0, 1.0, 0.0, 0.0])
        r = ba_ref.reproj_residual_jacobian(prob.obs_pose, prob.obs_point, np.zeros_like(prob.obs_uv), prob.q, prob.t, prob.X,
                                            prob.intr)[0]
        prob.obs_uv = np.ascontiguousarray(r)                                # residual = projection - observation
    return prob, 20


@pytest.mark.parametrize("path", ["lds", "big"])
@pytest.mark.parametrize("exit_", ["gradient tolerance", "parameter tolerance", "function tolerance"],
                         ids=lambda e: "exit-" + e.split()[0])
def test_every_exit_against_the_oracle(S, path, exit_):
    prob, iters = _exit_scene(path, exit_)
    assert (_free(prob) > MAX_PO) == (path == "big")
    points_const = exit_ == "parameter tolerance"
    ref = _oracle(prob, iters, points_const)
    assert ref[3]["termination"] == exit_, ref[3]                           # the oracle takes the exit the case is named for
    assert ref[3]["iterations"] < iters
    if exit_ == "function tolerance":
        assert ref[3]["iterations"] > 12                                     # (the suite's other cases stop at 10 - 12 by max_iters)
    if exit_ == "parameter tolerance":
        assert (ref[3]["iterations"], ref[3]["successful_steps"]) == (1, 0) and ref[3]["final_cost"] > 1e3
    _parity(S, prob, iters, ref=ref, points_const=points_const, host=True, what=f"{path} {exit_}",
            floor=exit_ == "gradient tolerance")


def test_rejected_steps_on_the_big_path(S):
    """The device-memory path through the rejection branch: radius shrinks, the linearisation is reused."""
    prob = _window(15, 300, *PATHS["big"])
    ref = _oracle(prob, 31)
    assert _free(prob) > MAX_PO and ref[3]["successful_steps"] <= ref[3]["iterations"] - 3, ref[3]
    _parity(S, prob, 31, ref=ref, what="big rejected")


# ---- structure edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["lds", "big"], ids=lambda p: f"const-only-point-{p}")
def test_point_seen_only_from_constant_poses(S, path):
    prob = _window(15, 300, *PATHS[path])
    const_rows = np.flatnonzero(prob.pose_const)
    victim = int(prob.obs_point[0])
    mine = np.flatnonzero(prob.obs_point == victim)
    prob.obs_pose = prob.obs_pose.copy()
    prob.obs_pose[mine] = const_rows[np.arange(len(mine)) % len(const_rows)]              # re-attach its observations
    assert prob.pose_const[prob.obs_pose[prob.obs_point == victim]].all() and len(mine) >= 2
    info, dev = _parity(S, prob, 8, what=f"{path} const-only point")
    assert not np.array_equal(dev.X[victim], prob.X[victim])                               # it still moves (its own 3 x 3 block)


@pytest.mark.parametrize("path", ["lds", "big"], ids=lambda p: f"unobserved-point-{p}")
def test_point_without_observation_comes_back_bit_identical(S, path):
    prob = _window(15, 300, *PATHS[path])
    lone = np.array([[1.25, -0.5, 17.0], [3.0, 0.25, 40.0]])
    at = 100
    prob.X = np.concatenate([prob.X[:at], lone[:1], prob.X[at:], lone[1:]])                # one inside a block, one last
    prob.obs_point = (prob.obs_point + (prob.obs_point >= at)).astype(np.int32)
    assert not np.isin([at, len(prob.X) - 1], prob.obs_point).any()
    info, dev = _parity(S, prob, 8, what=f"{path} unobserved point")
    np.testing.assert_array_equal(dev.X[at], lone[0])
    np.testing.assert_array_equal(dev.X[-1], lone[1])


def test_points_const_on_the_big_path(S):
    prob = _window(15, 300, *PATHS["big"])
    info, dev = _parity(S, prob, 12, points_const=True, what="big points_const")
    np.testing.assert_array_equal(dev.X, prob.X)
    assert info["final_cost"] < info["initial_cost"]


def test_gross_outliers_on_the_big_path(S):
    prob = _window(15, 300, *PATHS["big"])
    rng = np.random.default_rng(7)
    bad = rng.choice(len(prob.obs_uv), len(prob.obs_uv) // 10, replace=False)              # 10 % gross outliers (50 px)
    prob.obs_uv[bad] += rng.normal(0, 50.0, (len(bad), 2))
    _parity(S, prob, 15, what="big huber")


def test_residual_exactly_on_the_huber_threshold(S):
    """|r|^2 == delta^2 exactly takes the quadratic branch (s > b is false) in the oracle and must in the kernel:
    normalised intrinsics and a noise-free scene make the projection the oracle's own, an integer offset (2, 0) the residual."""
    prob, _ = _exit_scene("lds", "gradient tolerance")
    prob.obs_uv = prob.obs_uv.copy()
    on, above, below = 3, 11, 19
    prob.obs_uv[on] -= [2.0, 0.0]
    prob.obs_uv[above] -= [0.0, 2.5]
    prob.obs_uv[below] -= [1.5, 0.0]
    r = ba_ref.reproj_residual_jacobian(prob.obs_pose, prob.obs_point, prob.obs_uv, prob.q, prob.t, prob.X, prob.intr)[0]
    s = np.sum(r * r, axis=1)
    rho = ba_ref.huber_rho(s, 2.0)[0]
    # the oracle's residual is (2, 0) to the bit (coordinates below 1: p - (p - 2) rounds to 2), so s == delta^2 exactly
    # and `s > b` is false: the quadratic branch.  (Huber is C1 there, so the cost alone could not tell the branches
    # apart: what the case adds is the exact input.)
    assert r[on][0] == 2.0 and r[on][1] == 0.0 and s[on] == 4.0 and rho[on] == 4.0
    assert s[above] > 4.0 > s[below]
    want = 0.5 * float(np.sum(rho))
    dev = copy.deepcopy(prob)
    summ = S.solve_device(dev, 0, 2.0)
    assert summ.iterations == 0
    np.testing.assert_allclose(summ.initial_cost, want, rtol=1e-12)
    np.testing.assert_allclose(summ.final_cost, want, rtol=1e-12)
    np.testing.assert_allclose(want, 0.5 * (4.0 + (2 * 2.0 * 2.5 - 4.0) + 2.25), rtol=1e-9)


# ---- the 256-thread blocks of the two-stage reductions ---------------------------------------------------------------
def _truncate(prob, n_obs=None, n_points=None):
    p = copy.deepcopy(prob)
    if n_points is not None:
        keep = p.obs_point < n_points
        p.obs_pose, p.obs_point, p.obs_uv = p.obs_pose[keep].copy(), p.obs_point[keep].copy(), p.obs_uv[keep].copy()
        p.X = p.X[:n_points].copy()
    if n_obs is not None:
        p.obs_pose, p.obs_point, p.obs_uv = p.obs_pose[:n_obs].copy(), p.obs_point[:n_obs].copy(), p.obs_uv[:n_obs].copy()
        used = int(p.obs_point.max()) + 1                                                  # (points stay observed: drop the rest)
        p.X = p.X[:used].copy()
    return p


@pytest.mark.parametrize("kind,n", [("obs", 255), ("obs", 256), ("obs", 257), ("points", 255), ("points", 256),
                                    ("points", 257), ("points", 513)], ids=lambda v: str(v))
def test_block_edges_of_the_reductions(S, kind, n):
    base = _window(15, 600, range(5, 15), range(0, 5))
    prob = _truncate(base, n_obs=n) if kind == "obs" else _truncate(base, n_points=n)
    assert (len(prob.obs_pose) if kind == "obs" else len(prob.X)) == n
    zero = copy.deepcopy(prob)
    s0 = S.solve_device(zero, 0, 2.0)
    ref0 = _oracle(prob, 0)[3]
    np.testing.assert_allclose(s0.initial_cost, ref0["initial_cost"], rtol=1e-12)
    _parity(S, prob, 10, what=f"{kind}-{n}")
