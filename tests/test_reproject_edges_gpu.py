"""The 2D-3D association (csrc/reproject_kernels.hip) at its edges, against oracle/reproject_ref.py: the outputs the
overlay drops (`uv_out`, the candidate count, the overflow flag of the device entry), the half-open image border,
`0 < z <= 1e-8`, the radius boundary, RP_MAXC = 128 keypoints per projection, the 64-keypoint ballot blocks, the
4-points-per-workgroup tail, every `obs_cnt` 0..6, contention for one keypoint, and a descriptor distance on the
threshold.  Index arrays must be equal; `sslam_reproject_match_host` / `_dev` are called directly (through `_native`) and
must agree with each other on every case where both can run.

Every scene built to reach a branch first asserts on the oracle, on the CPU, that it does."""
import ctypes as C
import types
import warnings

import numpy as np
import pytest

import reproject_scenes as RS
from conftest import load_pkg
from oracle import reproject_ref as R

pytestmark = pytest.mark.gpu
RP_MAXC = 128                      # csrc/reproject_kernels.hip
F32 = np.float32


@pytest.fixture(scope="module")
def P():
    return load_pkg("slam.core.pnp_utils")


def _mp(position, descs):
    """A map point whose observations carry `descs` (None: an observation stored without descriptor)."""
    return types.SimpleNamespace(position=np.asarray(position, np.float64).copy(),
                                 observations=[(j, j, None if d is None else np.asarray(d, F32)) for j, d in enumerate(descs)])


def _wmap(points):
    return types.SimpleNamespace(points={7 + 3 * i: p for i, p in enumerate(points)})


def _scene(points, K, Tcw, kp, des, W, H, radius=12.0, max_l2=0.8):
    return dict(wmap=_wmap(points), K=np.asarray(K, np.float64), Tcw=np.asarray(Tcw, np.float64),
                kp=np.ascontiguousarray(kp, F32), des=np.ascontiguousarray(des, F32), W=W, H=H, radius=radius, max_l2=max_l2)


def _oracle(sc):
    """(kp_of_point [Q], uv [Q,2], candidate points that carry a descriptor) of the oracle."""
    items = list(sc["wmap"].points.items())
    _, _, kpr, mpr = R.reproject_and_match_2d3d(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                                radius_px=sc["radius"], max_l2=sc["max_l2"])
    row = {k: q for q, (k, _) in enumerate(items)}
    want = np.full(len(items), -1, np.int32)
    for i, m in zip(kpr, mpr):
        want[row[m]] = i
    uv, z = R.project_points(sc["K"], sc["Tcw"], np.asarray([mp.position for _, mp in items], np.float64))
    cand = (z > 0.0) & (uv[:, 0] >= 0.0) & (uv[:, 0] < float(sc["W"])) & (uv[:, 1] >= 0.0) & (uv[:, 1] < float(sc["H"]))
    has = np.array([bool(mp.observations) and mp.observations[-1][2] is not None for _, mp in items])
    return want, uv, cand & has


def _args(P, sc):
    ids, pts, cnt, desc = P.snapshot_map_points(sc["wmap"])
    return (np.ascontiguousarray(pts), np.ascontiguousarray(cnt), np.ascontiguousarray(desc),
            np.ascontiguousarray(sc["K"], np.float64).reshape(9), np.ascontiguousarray(sc["Tcw"], np.float64).reshape(16))


def _host(P, native, ctx, sc):
    pts, cnt, desc, K9, T16 = _args(P, sc)
    Q, N = len(pts), len(sc["kp"])
    out, uv, info = np.full(Q, -7, np.int32), np.full((Q, 2), np.nan, F32), (C.c_int32 * 2)()
    p = native.ptr
    native.check(native.lib().sslam_reproject_match_host(
        ctx.handle, Q, p(pts), p(cnt), p(desc), p(K9), p(T16), N, p(sc["kp"]), p(sc["des"]), int(sc["W"]), int(sc["H"]),
        float(sc["radius"]), float(sc["max_l2"]), p(out), p(uv), info), "sslam_reproject_match_host")
    return out, uv, int(info[0]), int(info[1])


def _dev(P, native, ctx, sc):
    """The device entry on uploaded copies; returns (kp_of_point, uv, info[4])."""
    pts, cnt, desc, K9, T16 = _args(P, sc)
    Q, N = len(pts), len(sc["kp"])
    d = [ctx.upload(a) for a in (pts, cnt, desc, sc["kp"], sc["des"])]
    o = [ctx.upload(np.full(Q, -7, np.int32)), ctx.upload(np.full((Q, 2), np.nan, F32)), ctx.upload(np.full(4, -7, np.int32))]
    p = native.ptr
    try:
        native.check(native.lib().sslam_reproject_match_dev(
            ctx.handle, Q, p(d[0]), p(d[1]), p(d[2]), p(K9), p(T16), N, p(d[3]), p(d[4]), int(sc["W"]), int(sc["H"]),
            float(sc["radius"]), float(sc["max_l2"]), p(o[0]), p(o[1]), p(o[2])), "sslam_reproject_match_dev")
        ctx.sync()
        out, uv, info = np.empty(Q, np.int32), np.empty((Q, 2), F32), np.empty(4, np.int32)
        ctx.d2h(out, o[0]); ctx.d2h(uv, o[1]); ctx.d2h(info, o[2])
    finally:
        ctx.sync()
        for q in d + o:
            ctx.free(q)
    return out, uv, info


def _check(P, native, ctx, sc):
    """Both entries against the oracle and against each other; returns the oracle's (kp_of_point, uv, candidates)."""
    want, uv_r, cand_r = _oracle(sc)
    out_h, uv_h, n_h, cand_h = _host(P, native, ctx, sc)
    out_d, uv_d, info_d = _dev(P, native, ctx, sc)
    np.testing.assert_array_equal(out_h, want)
    np.testing.assert_array_equal(out_d, out_h)
    assert n_h == info_d[0] == int((want >= 0).sum())
    assert info_d[1] == 0
    assert cand_h == info_d[2] == int(cand_r.sum())
    # bit equality of the float32 pixels (views as integers: -0.0 / NaN would not slip through)
    np.testing.assert_array_equal(uv_h.view(np.int32), uv_r.view(np.int32))
    np.testing.assert_array_equal(uv_d.view(np.int32), uv_r.view(np.int32))
    return want, uv_r, cand_r


def _unit_rows(rng, n):
    return RS.unit(rng.standard_normal((n, 128)))


# ---- uv_out and the candidate count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 2], ids=["uv-case0", "uv-case2"])
def test_uv_and_candidate_count_on_seeded_cases(P, native, gpu_ctx, c):
    sc = RS.make_case(*RS.CASES[c])
    want, uv, cand = _check(P, native, gpu_ctx, sc)
    assert (want >= 0).sum() > 20 and (uv[:, 0] == -1).any() and 0 < cand.sum() < len(cand)


def test_uv_behind_the_camera_and_at_tiny_depth(P, native, gpu_ctx):
    """Identity pose, so the camera depth IS the stored z: z < 0, z == 0, 0 < z <= 1e-8 give (-1, -1) and no candidate;
    the first double above 1e-8 projects."""
    rng = np.random.default_rng(5)
    zs = [-3.0, -1e-9, 0.0, 5e-324, 5e-9, 1e-8, float(np.nextafter(1e-8, 1.0)), 2e-8, 1.0, 30.0]
    base = _unit_rows(rng, len(zs))
    # x, y scale with z so the points that do project land inside the image (K of the seeded scenes)
    pts = [_mp([0.1 * z * (i - 4), 0.02 * z * i, z], [base[i]]) for i, z in enumerate(zs)]
    kp = np.stack([rng.uniform(0, RS.W, 40), rng.uniform(0, RS.H, 40)], 1)
    sc = _scene(pts, RS.K, np.eye(4), kp, _unit_rows(rng, 40), RS.W, RS.H)
    want, uv, cand = _oracle(sc)
    assert [bool(c) for c in cand] == [z > 1e-8 for z in zs]                 # the branch: the 1e-8 guard, not z > 0
    assert (uv[:6] == -1).all() and (uv[6:] != -1).all()
    _check(P, native, gpu_ctx, sc)


# ---- the half-open image border --------------------------------------------------------------------------------------
def test_image_border_is_half_open(P, native, gpu_ctx):
    """K = I, identity pose, z = 1: the float32 projection is exactly the stored x, y.  [0, img_w) x [0, img_h)."""
    W, H = 1241, 376
    below = lambda x: float(np.nextafter(F32(x), F32(-np.inf)))
    us = [(0.0, True), (below(0.0), False), (float(W), False), (below(W), True)]
    vs = [(0.0, True), (below(0.0), False), (float(H), False), (below(H), True)]
    probes = [(u, 40.0 + 50 * i, ok) for i, (u, ok) in enumerate(us)] + [(100.0 + 200 * i, v, ok) for i, (v, ok) in enumerate(vs)]
    probes += [(0.0, 0.0, True), (below(W), below(H), True), (float(W), below(H), False), (below(W), float(H), False)]
    rng = np.random.default_rng(6)
    base = _unit_rows(rng, len(probes))
    pts = [_mp([u, v, 1.0], [base[i]]) for i, (u, v, _) in enumerate(probes)]
    kp = np.array([[np.clip(u, 0, W - 1), np.clip(v, 0, H - 1)] for u, v, _ in probes], F32)   # one keypoint per probe, within 1 px
    sc = _scene(pts, np.eye(3), np.eye(4), kp, base, W, H, radius=2.0, max_l2=0.1)
    want, uv, cand = _oracle(sc)
    np.testing.assert_array_equal(uv, np.array([[u, v] for u, v, _ in probes], F32))       # exact projections
    assert [bool(c) for c in cand] == [ok for _, _, ok in probes]
    np.testing.assert_array_equal(want >= 0, cand)                                          # every candidate takes its keypoint
    _check(P, native, gpu_ctx, sc)


# ---- the radius boundary ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [12.0, 0.0], ids=["radius-12", "radius-0"])
def test_radius_boundary_is_closed(P, native, gpu_ctx, radius):
    """Axis-aligned offsets of exactly `radius` are in (d2 <= r2, the float64 square is exact), the next float32 out."""
    up = lambda x: float(np.nextafter(F32(x), F32(np.inf)))
    down = lambda x: float(np.nextafter(F32(x), F32(-np.inf)))
    c = [(100.0, 100.0), (300.0, 100.0), (500.0, 100.0), (700.0, 100.0), (900.0, 100.0)]
    kp = [(c[0][0] + radius, c[0][1], True), (up(c[1][0] + radius), c[1][1], False),
          (c[2][0], c[2][1] - radius, True), (c[3][0], down(c[3][1] - radius), False), (c[4][0], c[4][1], True)]
    rng = np.random.default_rng(7)
    base = _unit_rows(rng, len(c))
    pts = [_mp([u, v, 1.0], [base[i]]) for i, (u, v) in enumerate(c)]
    sc = _scene(pts, np.eye(3), np.eye(4), [(x, y) for x, y, _ in kp], base, 1241, 376, radius=radius, max_l2=0.1)
    want, _, cand = _oracle(sc)
    assert cand.all()
    np.testing.assert_array_equal(want, [i if ok else -1 for i, (_, _, ok) in enumerate(kp)])
    _check(P, native, gpu_ctx, sc)


# ---- RP_MAXC ---------------------------------------------------------------------------------------------------------
def _capacity_scene(k):
    """One projection with exactly k keypoints within the radius; the map point's descriptor is that of the LAST of them,
    so the right answer sits in the last slot of the candidate list.  A few other points / keypoints around."""
    rng = np.random.default_rng(8)
    g = np.array([(x, y) for y in range(-12, 13) for x in range(-12, 13) if x * x + y * y <= 144], np.float64)
    assert len(g) > 129
    inside = g[:k] + [600.0, 200.0]
    far = np.stack([rng.uniform(0, 400, 60), rng.uniform(0, 376, 60)], 1)
    kp = np.concatenate([far[:30], inside, far[30:]])                                       # ascending index: 30 .. 30 + k - 1
    des = _unit_rows(rng, len(kp))
    pts = [_mp([far[i][0], far[i][1], 1.0], [des[i]]) for i in range(5)]
    pts.insert(2, _mp([600.0, 200.0, 1.0], [_unit_rows(rng, 1)[0], des[30 + k - 1]]))
    return _scene(pts, np.eye(3), np.eye(4), kp, des, 1241, 376), 30 + k - 1


def _in_range(sc, q):
    """Indices of the keypoints within the radius of map point q's projection, as the oracle's ball query finds them."""
    uv, _ = R.project_points(sc["K"], sc["Tcw"], np.asarray([mp.position for mp in sc["wmap"].points.values()]))
    d2 = np.sum((sc["kp"].astype(np.float64) - uv[q].astype(np.float64)) ** 2, axis=1)
    return np.flatnonzero(d2 <= float(sc["radius"]) ** 2)


@pytest.mark.parametrize("k", [127, 128], ids=["maxc-127", "maxc-128"])
def test_candidate_capacity_is_usable_to_the_last_slot(P, native, gpu_ctx, k):
    sc, last = _capacity_scene(k)
    assert len(_in_range(sc, 2)) == k
    want, _, _ = _oracle(sc)
    assert want[2] == last and (want >= 0).sum() == 6
    _check(P, native, gpu_ctx, sc)
    L = load_pkg("slam.core.landmark_utils")                                                # ... and the overlay's SoA path
    m = P.reproject_and_match_2d3d(L.Map.from_reference(sc["wmap"]), sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                   ctx=gpu_ctx)
    np.testing.assert_array_equal(m.kp_indices, want[want >= 0])


def test_candidate_capacity_overflow_is_reported(P, native, gpu_ctx):
    sc, _ = _capacity_scene(129)
    assert len(_in_range(sc, 2)) == RP_MAXC + 1
    with pytest.raises(native.NativeError, match="keypoints within"):
        _host(P, native, gpu_ctx, sc)
    _, _, info = _dev(P, native, gpu_ctx, sc)
    assert info[1] == 1
    L = load_pkg("slam.core.landmark_utils")
    with pytest.raises(native.NativeError, match="candidate capacity"):
        P.reproject_and_match_2d3d(L.Map.from_reference(sc["wmap"]), sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                   ctx=gpu_ctx)


# ---- shape edges -----------------------------------------------------------------------------------------------------
def _dense_scene(seed, n_pts, n_kp, n_obs=None):
    """Every point projects into a 300 x 150 px window and every keypoint lies within a few pixels of some projection, so
    each ballot block of 64 keypoints and each workgroup of 4 points has work.  n_obs[i]: descriptors of point i
    (default: 0..6 in turn, then 8 observations with two of them stored without descriptor)."""
    rng = np.random.default_rng(seed)
    ang = 0.03
    Tcw = np.eye(4)
    Tcw[:3, :3] = [[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]
    Tcw[:3, 3] = [0.2, -0.1, 0.3]
    uv = np.stack([rng.uniform(400, 700, n_pts), rng.uniform(100, 250, n_pts)], 1)
    z = rng.uniform(5, 50, n_pts)
    Xc = np.stack([(uv[:, 0] - RS.K[0, 2]) / RS.K[0, 0] * z, (uv[:, 1] - RS.K[1, 2]) / RS.K[1, 1] * z, z], 1)
    X = (Xc - Tcw[:3, 3]) @ Tcw[:3, :3]
    base = _unit_rows(rng, n_pts)
    pts = []
    for i in range(n_pts):
        c = (i % 8) if n_obs is None else n_obs[i]
        noisy = [RS.unit(base[i] + 0.25 * rng.standard_normal(128) / np.sqrt(128)) for _ in range(8)]
        descs = noisy[:c] if c < 7 else [noisy[0], None, noisy[2], noisy[3], None, noisy[5], noisy[6], noisy[7]]
        pts.append(_mp(X[i], descs))
    of = rng.integers(0, n_pts, n_kp)
    kp = uv[of] + rng.normal(0, 3.0, (n_kp, 2))
    des = RS.unit(base[of] + 0.25 * rng.standard_normal((n_kp, 128)) / np.sqrt(128))
    return _scene(pts, RS.K, Tcw, kp, des, RS.W, RS.H)


@pytest.mark.parametrize("n_kp", [1, 63, 64, 65, 129], ids=lambda n: f"nkp-{n}")
def test_keypoint_counts_around_the_ballot_block(P, native, gpu_ctx, n_kp):
    sc = _dense_scene(n_kp, 37, n_kp)
    want, _, cand = _oracle(sc)
    reached = np.unique(np.concatenate([_in_range(sc, q) for q in np.flatnonzero(cand)]))
    assert reached[-1] == n_kp - 1 and (want >= 0).any()                # the last lane of the last (partial) block is in range
    _check(P, native, gpu_ctx, sc)


@pytest.mark.parametrize("n_pts", [1, 3, 4, 5, 1025], ids=lambda n: f"npts-{n}")
def test_point_counts_around_the_workgroup_of_four(P, native, gpu_ctx, n_pts):
    sc = _dense_scene(100 + n_pts, n_pts, max(100, 2 * n_pts), n_obs=[1 + (i % 6) for i in range(n_pts)])
    want, _, cand = _oracle(sc)
    assert max(len(_in_range(sc, q)) for q in range(n_pts)) <= RP_MAXC                # (in contract: no list overflows)
    assert cand.all() and len(_in_range(sc, n_pts - 1)) > 0 and want[-1] >= 0       # the last wave of the tail has work
    _check(P, native, gpu_ctx, sc)


def test_every_observation_count_in_one_call(P, native, gpu_ctx):
    sc = _dense_scene(9, 64, 300)                                                          # obs counts 0..6, 8 in turn
    _, _, cnt, _ = P.snapshot_map_points(sc["wmap"])
    assert sorted(set(cnt.tolist())) == [0, 1, 2, 3, 4, 5, 6]
    want, _, cand = _check(P, native, gpu_ctx, sc)
    assert not cand[cnt == 0].any() and (want[cnt == 0] == -1).all()                       # 0: the point is skipped
    for c in range(1, 7):
        assert (want[cnt == c] >= 0).any(), c


# ---- contention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", [False, True], ids=["contention", "contention-tie"])
def test_contention_for_the_same_keypoints(P, native, gpu_ctx, tie):
    """200 map points within the radius of the same 10 keypoints, near-equal descriptors: the greedy order and the `used`
    bitmap decide.  With a tie (two keypoints carrying the same descriptor) the lower index wins, as in the oracle."""
    rng = np.random.default_rng(10)
    b = _unit_rows(rng, 1)[0]
    near = lambda n: RS.unit(b + 0.02 * rng.standard_normal((n, 128)))
    kp = np.concatenate([[600.0, 200.0] + rng.uniform(-2, 2, (10, 2)), np.stack([rng.uniform(0, 300, 30), rng.uniform(0, 376, 30)], 1)])
    des = np.concatenate([near(10), _unit_rows(rng, 30)])
    perm = rng.permutation(len(kp))
    kp, des = kp[perm], des[perm]
    hot = np.sort(np.argsort(perm)[:10])                                                   # where the 10 contended keypoints went
    if tie:
        des[hot[7]] = des[hot[2]]
    pd = near(200)
    pts = [_mp([600.0 + rng.uniform(-2, 2), 200.0 + rng.uniform(-2, 2), 1.0], [pd[i]]) for i in range(200)]
    sc = _scene(pts, np.eye(3), np.eye(4), kp, des, 1241, 376)
    want, _, cand = _oracle(sc)
    assert cand.all() and sorted(want[want >= 0]) == list(hot)                              # 10 of the 200 win, all 10 are taken
    if tie:
        takers = {int(want[q]): q for q in np.flatnonzero(want >= 0)}
        assert takers[int(hot[2])] < takers[int(hot[7])]                                   # the lower index went first
    _check(P, native, gpu_ctx, sc)


# ---- a descriptor distance on the threshold --------------------------------------------------------------------------
def test_distance_on_the_threshold(P, native, gpu_ctx):
    """max_l2 = the smallest accepted distance is still accepted (`best_d > thr` rejects); the float64 just below rejects.
    The kernel sums the 128 squares in another order than numpy, so its float32 distance may differ in the last bit: that
    case is reported and bracketed with a threshold one float32 ulp away, never passed silently."""
    sc = RS.make_case(*RS.CASES[0])
    items = list(sc["wmap"].points.items())
    want, uv, cand = _oracle(sc)
    kp64, r2 = sc["kp"].astype(np.float64), sc["radius"] ** 2
    d32, d64, owner = [], [], []
    for q in np.flatnonzero(cand):
        obs = [np.asarray(d, F32) for _, _, d in items[q][1].observations[-6:] if d is not None]
        for i in np.flatnonzero(np.sum((kp64 - uv[q].astype(np.float64)) ** 2, axis=1) <= r2):
            d32.append(min(float(np.linalg.norm(o - sc["des"][i])) for o in obs))
            d64.append(min(float(np.linalg.norm((o - sc["des"][i]).astype(np.float64))) for o in obs))   # same float32 differences
            owner.append((q, i))
    d32, d64 = np.array(d32), np.array(d64)
    accepted = np.array([d32[owner.index((q, int(want[q])))] for q in np.flatnonzero(want >= 0)])
    d_min = float(accepted.min())
    # measured on the CPU: summing the 128 float32 squares in float32 moves a distance by at most `err` from the float64
    # sum of the same squares (1.4e-7 over this scene's candidate pairs, a few ulp); the nearest other candidate distance
    # is `gap` away from the probe (6.6e-4): far more than 100 x err, so only the probed pair can change sides
    err = float(np.abs(d32 - d64).max())
    gap = float(np.sort(np.abs(d32 - d_min))[1])
    print(f"\n[threshold probe] d_min {d_min!r}, float32-sum error {err:.3g}, gap to the next distance {gap:.3g}")
    assert err < 4 * np.spacing(F32(1.0)) and gap >= 100 * err and (d32 == d_min).sum() == 1
    ulp = float(np.spacing(F32(d_min)))

    def run(thr):
        s = dict(sc, max_l2=thr)
        w, _, _ = _oracle(s)
        out_h, _, _, _ = _host(P, native, gpu_ctx, s)
        out_d, _, _ = _dev(P, native, gpu_ctx, s)
        np.testing.assert_array_equal(out_d, out_h)
        return w, out_h

    w_at, g_at = run(d_min)
    assert (w_at >= 0).sum() == 1                                                          # the oracle accepts exactly that pair
    w_lo, g_lo = run(float(np.nextafter(d_min, 0.0)))
    assert (w_lo >= 0).sum() == 0                                                          # ... and rejects it just below
    if not np.array_equal(g_at, w_at):
        warnings.warn(f"threshold probe: the GPU's distance for the accepted pair is ABOVE numpy's {d_min!r}: comparing one float32 ulp up")
        w_up, g_up = run(d_min + ulp)
        np.testing.assert_array_equal(w_up, w_at)
        np.testing.assert_array_equal(g_up, w_up)
        np.testing.assert_array_equal(g_at, w_lo)                                          # (then it rejected at d_min, nothing else)
    elif not np.array_equal(g_lo, w_lo):
        warnings.warn(f"threshold probe: the GPU's distance for the accepted pair is BELOW numpy's {d_min!r}: comparing one float32 ulp down")
        w_dn, g_dn = run(float(np.nextafter(d_min - ulp, 0.0)))
        np.testing.assert_array_equal(w_dn, w_lo)
        np.testing.assert_array_equal(g_dn, w_dn)
        np.testing.assert_array_equal(g_lo, w_at)
    else:
        np.testing.assert_array_equal(g_at, w_at)
        np.testing.assert_array_equal(g_lo, w_lo)
