"""One scratch slab under every geometry entry.  BA, the device LM, the F / H / E / PnP RANSACs, triangulation, recoverPose,
the two-view metrics and the 2D-3D association keep nothing between calls: each lays its pieces out in the context's slab
(csrc/geom_slab.hpp) and must write every byte it later reads.  The per-family tests drive the slab big-then-small within one
family; here ONE context serves every host entry in turn - a large round, a 20 000-observation Jacobian that fills the slab's
front with non-zero doubles, then every entry's smallest legal sizes, each right behind a larger call of ANOTHER family - and
every output must equal, bit for bit, the same call made on a fresh context of its own."""
import ctypes as C

import numpy as np
import pytest

import ba_scenes
import pnp_scenes
import relative_pose_scenes as RPS
import reproject_scenes
import triangulate_scenes as TS
import two_view
from conftest import load_pkg

pytestmark = pytest.mark.gpu


def _flat(out):
    """every array / scalar of a wrapper's result, in order (None stays None, dicts by sorted key)"""
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [x for o in out for x in _flat(o)]
    return [None if out is None else np.asarray(out)]


def _same(got, want, what):
    a, b = _flat(got), _flat(want)
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, i)
        if x is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, x.shape, y.shape)
        # (triangulation's diagnostics document NaN for matches without a point)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, i)


def _calls():
    """name -> (family, fn(ctx) -> result)"""
    E_ = load_pkg("epipolar"); H_ = load_pkg("homography"); EM_ = load_pkg("essential"); PN_ = load_pkg("pnp")
    TR_ = load_pkg("triangulation"); RP_ = load_pkg("relative_pose"); S_ = load_pkg("ba_solver")
    PU_ = load_pkg("slam.core.pnp_utils"); BU_ = load_pkg("slam.core.ba_utils"); native = load_pkg("_native")
    calls = {}

    for n in (8, 15, 300):                    # 8: LMedS; 15: the first RANSAC size
        p1, p2, _ = two_view.make_matches(n, outlier_frac=0.3 if n == 300 else 0.0, seed=n)
        calls[f"F{n}"] = ("F", lambda ctx, p1=p1, p2=p2: E_.find_fundamental_ransac(p1, p2, 1.0, 0.99, ctx=ctx))
    for n in (4, 5, 300):                     # 4: the direct solve
        p1, p2, _ = two_view.make_matches(n, outlier_frac=0.3 if n == 300 else 0.0, seed=10 + n, planar=True)
        calls[f"H{n}"] = ("H", lambda ctx, p1=p1, p2=p2: H_.find_homography_ransac(p1, p2, 1.5, ctx=ctx))
    for n in (5, 6, 300):                     # 5: the direct solve
        p1, p2, _ = two_view.make_matches(n, outlier_frac=0.3 if n == 300 else 0.0, noise=0.03, seed=20 + n)
        calls[f"E{n}"] = ("E", lambda ctx, p1=p1, p2=p2: EM_.find_essential_mat_ransac(p1, p2, two_view.K, ctx=ctx))
    for n in (5, 6, 300):                     # 5: a single EPnP
        sc = pnp_scenes.make_scene(30 + n, n, 0.3 if n == 300 else 0.0)
        for guess in (False, True):
            calls[f"PnP{n}{'g' if guess else ''}"] = ("PnP", lambda ctx, sc=sc, guess=guess: PN_.solve_pnp_ransac(
                sc["pts3d"], sc["pts2d"], sc["K"], use_guess=guess, ctx=ctx))
    for n, counts in ((1, {"good": 1}), (300, {"good": 200, "far": 40, "outlier": 60})):
        sc = TS.make_scene(f"slab{n}", counts, 40 + n)
        calls[f"TRI{n}"] = ("TRI", lambda ctx, sc=sc: TR_.triangulate_2view(
            sc["pts1"], sc["pts2"], sc["K"], sc["T1"], sc["T2"], want_diag=True, ctx=ctx, **sc["params"]))
    for n in (0, 1, 300):
        sc = RPS.make_scene(f"slab{n}", n, "rotation", 50 + n, far=0.1 if n == 300 else 0.0, mask01=True)
        for m in (False, True):
            calls[f"RP{n}{'m' if m else ''}"] = ("RP", lambda ctx, sc=sc, m=m: RP_.recover_pose(
                sc["E"], sc["pts1"], sc["pts2"], sc["K"], sc["thresh"], mask=sc["mask"] if m else None, ctx=ctx, want_info=True))
    for n in (2, 300):
        sc = RPS.make_scene(f"slabtv{n}", n, "sideways", 60 + n)
        calls[f"TV{n}"] = ("TV", lambda ctx, sc=sc: RP_.two_view_metrics(
            sc["K"], sc["R"], sc["t"], sc["pts1"], sc["pts2"], sel=sc["sel"], want_points=True, ctx=ctx, want_info=True))

    rm = reproject_scenes.make_case(*reproject_scenes.CASES[4])          # 50 map points, 40 keypoints
    _, pts, cnt, desc = PU_.snapshot_map_points(rm["wmap"])
    pts, cnt, desc = (np.ascontiguousarray(x) for x in (pts, cnt, desc))
    K9, T16 = np.ascontiguousarray(rm["K"], np.float64).reshape(9), np.ascontiguousarray(rm["Tcw"], np.float64).reshape(16)

    def reproject(ctx):
        Q, N = len(pts), len(rm["kp"])
        out, uv, info = np.full(Q, -7, np.int32), np.full((Q, 2), np.nan, np.float32), (C.c_int32 * 2)()
        p = native.ptr
        native.check(native.lib().sslam_reproject_match_host(
            ctx.handle, Q, p(pts), p(cnt), p(desc), p(K9), p(T16), N, p(rm["kp"]), p(rm["des"]), int(rm["W"]), int(rm["H"]),
            12.0, 0.8, p(out), p(uv), info), "sslam_reproject_match_host")
        return out, uv, np.array(list(info))
    calls["RM"] = ("RM", reproject)

    def residual_jacobian(ctx, pi, xi, uv, q, t, X, intr):
        n = len(pi)
        r, Jq, Jt, JX = (np.full((n,) + s, np.nan) for s in ((2,), (2, 4), (2, 3), (2, 3)))
        p = native.ptr
        native.check(native.lib().sslam_ba_residual_jacobian_host(
            ctx.handle, n, p(pi), p(xi), p(uv), len(q), p(q), p(t), len(X), p(X), p(intr), p(r), p(Jq), p(Jt), p(JX)))
        return r, Jq, Jt, JX

    wmap, kfs, Kc = ba_scenes.reference_test_scene(3, n_points=20, add_noise=True)
    prob, _, _ = BU_.snapshot_problem(wmap, Kc, kfs, [1, 2], [0])
    small = tuple(np.ascontiguousarray(x, d) for x, d in ((prob.obs_pose, np.int32), (prob.obs_point, np.int32), (prob.obs_uv, np.float64),
                                                          (prob.q, np.float64), (prob.t, np.float64), (prob.X, np.float64), (prob.intr, np.float64)))
    calls["BA"] = ("BA", lambda ctx: residual_jacobian(ctx, *small))

    def solve(ctx):
        p = S_.BAProblem(prob.q.copy(), prob.t.copy(), prob.pose_const.copy(), prob.X.copy(), prob.intr.copy(),
                         prob.obs_pose.copy(), prob.obs_point.copy(), prob.obs_uv.copy())
        s = S_.solve_device(p, 10, 2.0, ctx=ctx)
        return p.q, p.t, p.X, np.array([s.iterations, s.successful_steps, s.initial_cost, s.final_cost])
    calls["LM"] = ("LM", solve)

    rng = np.random.default_rng(7)
    n, P, Q = 20000, 15, 5000
    q = rng.standard_normal((P, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    big = (rng.integers(0, P, n).astype(np.int32), rng.integers(0, Q, n).astype(np.int32), rng.uniform(0, 1241, (n, 2)), q,
           rng.standard_normal((P, 3)), rng.standard_normal((Q, 3)) * 3 + np.array([0, 0, 20.0]),
           np.array([718.856, 718.856, 607.1928, 185.2157]))
    calls["BA20000"] = ("BA", lambda ctx: residual_jacobian(ctx, *big))
    return calls


LARGE = ["F300", "H300", "E300", "PnP300g", "PnP300", "TRI300", "RP300m", "RP300", "TV300", "RM", "BA", "LM"]
# (larger call, small call of another family) - the small one reads the slab the larger one left
PAIRS = [("H300", "F8"), ("E300", "F15"), ("F300", "H4"), ("PnP300", "H5"), ("H300", "E5"), ("TRI300", "E6"), ("E300", "PnP5g"),
         ("RP300", "PnP5"), ("TV300", "PnP6g"), ("F300", "PnP6"), ("PnP300g", "TRI1"), ("H300", "RP0"), ("E300", "RP0m"),
         ("TRI300", "RP1"), ("F300", "RP1m"), ("PnP300", "TV2"), ("RP300m", "RM"), ("TV300", "BA"), ("H300", "LM")]


def test_every_entry_on_one_slab_equals_a_fresh_context(native, gpu_ctx):
    calls = _calls()
    order = LARGE + ["BA20000"] + [name for pair in PAIRS for name in pair]
    assert set(order) == set(calls)
    for big, small in PAIRS:
        assert calls[big][0] != calls[small][0], (big, small)
    shared = native.Context(0)
    try:
        got = [(name, calls[name][1](shared)) for name in order]
    finally:
        shared.close()
    want = {}
    for name in calls:                        # one fresh context per call, one after another
        ctx = native.Context(0)
        try:
            want[name] = calls[name][1](ctx)
        finally:
            ctx.close()
    for i, (name, out) in enumerate(got):
        _same(out, want[name], f"call {i} ({name}) on the shared slab")
