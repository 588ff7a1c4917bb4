"""PnP-RANSAC on the MI355X (csrc/pnp_kernels.hip) against the numpy restatement of OpenCV's classic
solvePnPRansac(SOLVEPNP_ITERATIVE) (oracle/pnp_ref.py), plus the host / device entries, the association -> PnP chain
on the device and the edge cases."""
import numpy as np
import pytest

import pnp_scenes as S
import reproject_scenes as RS
from conftest import load_pkg
from oracle import pnp_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    n = load_pkg("_native")
    if n.device_count() < 1:
        pytest.skip("needs an MI355X")
    return n


@pytest.fixture(scope="module")
def PN(native):
    return load_pkg("pnp")


def _compare(PN, sc, use_guess, iters=S.ITERS):
    p3, p2, K = sc["pts3d"], sc["pts2d"], sc["K"]
    ok, r, t, mask, info = O.solve_pnp_ransac(p3, p2, K, S.RANSAC_PX, use_guess, iters, S.CONF)
    gok, T, gmask, ginfo = PN.solve_pnp_ransac(p3, p2, K, S.RANSAC_PX, S.CONF, iters, use_guess=use_guess)
    assert gok == ok
    assert (ginfo["samples"], ginfo["sample"]) == (info["samples"], info["sample"])
    if not ok:
        return
    # masks: identical except where the restated error of the winner lies within 1e-5 relative of the threshold
    t2 = np.float32(np.float32(S.RANSAC_PX) ** 2)
    e = O.reproj_err(p3, p2, *O.epnp_model(p3[_subset(len(p3), info["sample"])], p2[_subset(len(p3), info["sample"])], K), K) \
        if info["sample"] >= 0 else np.zeros(len(p3), np.float32)
    near = np.abs(e.astype(np.float64) - t2) <= 1e-5 * t2
    assert near.sum() <= 1
    np.testing.assert_array_equal(gmask[~near], mask[~near])
    assert ginfo["inliers"] == int(gmask.sum())
    if not near.any():
        assert ginfo["inliers"] == info["inliers"]
    Tr = O.pose_matrix(r, t)
    assert S.rot_err_rad(T[:3, :3], Tr[:3, :3]) < 1e-6
    assert np.linalg.norm(T[:3, 3] - Tr[:3, 3]) < 1e-6 * (1 + np.linalg.norm(Tr[:3, 3]))
    return T, gmask, ginfo


def _subset(n, h):
    rng = O.CvRNG()
    for _ in range(h + 1):
        idx = []
        for _ in range(5):
            v = rng.uniform(0, n)
            while v in idx:
                v = rng.uniform(0, n)
            idx.append(v)
    return idx


@pytest.mark.parametrize("seed,n,frac,cam", S.GPU_GRID)
def test_matches_restatement(PN, seed, n, frac, cam):
    """n in {30, 100, 600, 2000, 6000} (6000: past the LM's LDS staging), 0 / 30 / 60 % outliers, no guess: the same
    sample count and winner, the same mask, the pose within 1e-6."""
    _compare(PN, S.make_scene(100 + seed, n, frac, cam), False)


@pytest.mark.parametrize("seed,n,frac,cam", [(1, 100, 0.3, "rand"), (2, 600, 0.3, "kitti"), (3, 2000, 0.6, "rand")])
def test_matches_restatement_with_guess(PN, seed, n, frac, cam):
    """With a guess (the tracker always passes Tcw_pred): the refinement starts at the last sample, as restated."""
    _compare(PN, S.make_scene(200 + seed, n, frac, cam), True)


def test_recovers_pose_on_kitti_tracking_scene(PN):
    sc = S.make_scene(7, 600, 0.3, "kitti")
    ok, T, mask, _ = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS)
    assert ok
    assert S.rot_err_deg(T[:3, :3], sc["Tcw"][:3, :3]) < 2.0 and np.linalg.norm(T[:3, 3] - sc["Tcw"][:3, 3]) < 0.1
    assert (mask & sc["inlier"]).sum() >= 0.95 * sc["inlier"].sum()


def test_two_calls_bit_identical(PN):
    sc = S.make_scene(8, 2000, 0.3, "kitti")
    a = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS, use_guess=True)
    b = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS, use_guess=True)
    assert a[0] and a[3] == b[3]
    assert a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


def _dev_call(native, PN, ctx, kop, xyz, kp, K, use_guess, iters=S.ITERS):
    Q = len(kop)
    d_kop, d_xyz, d_kp = ctx.upload(kop.astype(np.int32)), ctx.upload(xyz.astype(np.float64)), ctx.upload(kp.astype(np.float32))
    d_T, d_info, d_mask, d_n = ctx.malloc(128), ctx.malloc(16), ctx.malloc(Q), ctx.malloc(4)
    PN.solve_pnp_ransac_dev(ctx, Q, d_kop, d_xyz, d_kp, K, d_T, d_info, S.RANSAC_PX, S.CONF, iters, use_guess=use_guess,
                            mask_out_dev=d_mask, n_out_dev=d_n)
    ctx.sync()
    T, info, mask, n = np.empty(16), np.empty(4, np.int32), np.empty(Q, np.uint8), np.empty(1, np.int32)
    for h, d in ((T, d_T), (info, d_info), (mask, d_mask), (n, d_n)):
        ctx.d2h(h, d)
    for d in (d_kop, d_xyz, d_kp, d_T, d_info, d_mask, d_n):
        ctx.free(d)
    return T.reshape(4, 4), info, mask[:n[0]].astype(bool), int(n[0])


@pytest.mark.parametrize("use_guess", [False, True])
def test_host_and_device_entries_bit_identical(native, PN, use_guess):
    """The device entry compacts the association's output (map order, float32) and gives what the host entry gives."""
    ctx = native.default_context()
    sc = S.make_scene(9, 700, 0.3, "kitti")
    rng = np.random.default_rng(9)
    Q = 1500                                              # map points, 700 of them associated, in a shuffled order
    slots = np.sort(rng.choice(Q, 700, replace=False))
    kp = np.concatenate([sc["pts2d"], rng.uniform(0, 600, (300, 2))]).astype(np.float32)
    perm = rng.permutation(len(kp))                       # keypoints in arbitrary order
    kp_sh = np.empty_like(kp)
    kp_sh[perm] = kp
    kop = np.full(Q, -1, np.int32)
    kop[slots] = perm[:700]
    xyz = rng.uniform(-5, 5, (Q, 3))
    xyz[slots] = sc["pts3d"].astype(np.float64)
    T, info, mask, n = _dev_call(native, PN, ctx, kop, xyz, kp_sh, sc["K"], use_guess)
    ok, Th, mh, ih = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS, use_guess=use_guess)
    assert ok and n == 700
    assert T.tobytes() == Th.tobytes() and np.array_equal(mask, mh)
    assert list(info) == [ih["inliers"], ih["samples"], ih["sample"], ih["lm_iters"]]


def test_association_chain_on_device_equals_host_dropin(native, PN):
    """reproject_and_match_2d3d's device path (SoA map) -> sslam_pnp_ransac_dev on its device output, against the host
    drop-in solve_pnp_ransac on the Matches2D3D the overlay returns."""
    P = load_pkg("slam.core.pnp_utils")
    L = load_pkg("slam.core.landmark_utils")
    ctx = native.default_context()
    sc = RS.make_case(*RS.CASES[1])
    m = L.Map.from_reference(sc["wmap"])
    r = P.reproject_and_match_2d3d(m, sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"], radius_px=sc["radius"],
                                   max_l2=sc["max_l2"], use_cosine=sc["use_cosine"], ctx=ctx)
    assert len(r.pts3d) > 100
    Th, mh = P.solve_pnp_ransac(r.pts3d, r.pts2d, sc["K"], S.RANSAC_PX, Tcw_init=sc["Tcw"], iters=300, conf=S.CONF, ctx=ctx)
    assert Th is not None
    ids, _, _, _ = m.soa()
    d_pos, _, _ = m.device_arrays(ctx)
    scr = ctx.scratch["reproject"]
    Q = len(ids)
    d_T, d_info, d_mask, d_n = ctx.malloc(128), ctx.malloc(16), ctx.malloc(Q), ctx.malloc(4)
    PN.solve_pnp_ransac_dev(ctx, Q, scr["out"], d_pos, scr["kp"], sc["K"], d_T, d_info, S.RANSAC_PX, S.CONF, 300,
                            use_guess=True, mask_out_dev=d_mask, n_out_dev=d_n)
    ctx.sync()
    T, info, mask, n = np.empty(16), np.empty(4, np.int32), np.empty(Q, np.uint8), np.empty(1, np.int32)
    for h, d in ((T, d_T), (info, d_info), (mask, d_mask), (n, d_n)):
        ctx.d2h(h, d)
    for d in (d_T, d_info, d_mask, d_n):
        ctx.free(d)
    assert n[0] == len(r.pts3d)
    assert T.reshape(4, 4).tobytes() == Th.tobytes()
    np.testing.assert_array_equal(mask[:n[0]].astype(bool), mh)


def test_edge_cases_return_no_pose_without_error(native, PN):
    P = load_pkg("slam.core.pnp_utils")
    ctx = native.default_context()
    K = S.K_RAND
    for n in range(4):                                     # overlay: returns early
        assert P.solve_pnp_ransac(np.zeros((n, 3)), np.zeros((n, 2)), K, 2.5)[0] is None
    for n in (0, 1, 3, 4):                                 # device entry: fewer than 5 correspondences -> no pose
        kop = np.concatenate([np.arange(n), np.full(6, -1)]).astype(np.int32)
        T, info, mask, nn = _dev_call(native, PN, ctx, kop, np.ones((len(kop), 3)), np.ones((8, 2)), K, False)
        assert nn == n and info[0] == -1 and np.array_equal(T, np.eye(4))
    # n == 5: one EPnP on all points, all inliers, as restated
    sc = S.make_scene(31, 5, 0.0, "rand")
    ok, T, mask, info = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], K, S.RANSAC_PX, S.CONF, S.ITERS, use_guess=True)
    okr, r, t, mr, ir = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], K, S.RANSAC_PX, True, S.ITERS, S.CONF)
    assert ok and mask.all() and info == ir
    assert S.rot_err_rad(T[:3, :3], O.pose_matrix(r, t)[:3, :3]) < 1e-9
    # degenerate: every point identical
    ok, T, mask, info = PN.solve_pnp_ransac(np.tile([[0.5, -0.2, 4.0]], (40, 1)), np.tile([[310.0, 190.0]], (40, 1)), K,
                                            S.RANSAC_PX, S.CONF, 50)
    assert not ok and not mask.any() and info["inliers"] == -1
    assert P.solve_pnp_ransac(np.tile([[0.5, -0.2, 4.0]], (40, 1)), np.tile([[310.0, 190.0]], (40, 1)), K, 2.5)[0] is None
    # all outliers
    rng = np.random.default_rng(5)
    sc = S.make_scene(41, 60, 0.0, "rand")
    p2 = np.stack([rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)], 1).astype(np.float32)
    ok, T, mask, info = PN.solve_pnp_ransac(sc["pts3d"], p2, K, 0.01, S.CONF, 40)
    assert not ok and not mask.any() and info["samples"] == 40
    # refine_pose_pnp: no guess, 200 iterations, float64 (R, t)
    sc = S.make_scene(42, 300, 0.3, "rand")
    R, t = P.refine_pose_pnp(sc["K"], sc["pts3d"], sc["pts2d"], 2.5)
    assert R.dtype == np.float64 and t.shape == (3,) and S.rot_err_deg(R, sc["Tcw"][:3, :3]) < 2.0
