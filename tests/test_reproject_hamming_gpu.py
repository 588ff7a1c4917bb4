"""The Hamming branch of `reproject_and_match_2d3d` on the GPU (csrc/reproject_kernels.hip: rp_pairs_hamming_kernel,
`sslam_reproject_match_hamming_host` / `_dev`) - index arrays, pts3d and pts2d BIT FOR BIT:

* against the reference's own outputs (tests/golden/reproject_hamming.npz), through the dict-of-objects map (host entry)
  and through the SoA map (device entry);
* against the numpy restatement (tests/reproject_hamming_ref.py) on small scenes, each built for one edge of the kernel:
  point counts that do not fill a workgroup, keypoint counts around one ballot pass, 65 and 128 keypoints in range (the
  second lane pass, the full list), 129 (overflow), 0..6 stored rows, widths on each load path, tied minima, the threshold;
* the device chain (a device keypoint count smaller than the row bound) and the drop-in up to a pose."""
import types

import numpy as np
import pytest

import pnp_scenes as S
import reproject_hamming_ref as HR
import reproject_hamming_scenes as HS
from conftest import ROOT, load_pkg

pytestmark = pytest.mark.gpu
G = np.load(ROOT / "tests" / "golden" / "reproject_hamming.npz")
K, W, H = HS.K, HS.W, HS.H
Z = 10.0


@pytest.fixture(scope="module")
def P():
    return load_pkg("slam.core.pnp_utils")


@pytest.fixture(scope="module")
def L():
    return load_pkg("slam.core.landmark_utils")


def grid_uv(Q):
    """Projections 40 px apart (far more than any radius used here), inside the image."""
    q = np.arange(Q)
    return np.stack([100.0 + 40.0 * (q % 25), 60.0 + 40.0 * (q // 25)], 1)


def points_at(uv):
    return np.stack([(uv[:, 0] - K[0, 2]) * Z / K[0, 0], (uv[:, 1] - K[1, 2]) * Z / K[1, 1], np.full(len(uv), Z)], 1)


def make_map(X, obs_rows):
    """obs_rows[q]: list of uint8 rows (or None) in observation order."""
    wmap = types.SimpleNamespace(points={})
    for q in range(len(X)):
        obs = [(j, j, None if d is None else np.array(d, np.uint8)) for j, d in enumerate(obs_rows[q])]
        wmap.points[3 * q + 5] = types.SimpleNamespace(position=X[q].copy(), observations=obs)
    return wmap


def small_scene(seed, Q, N, B, obs_counts=None):
    """Q points on the grid with `obs_counts[q]` noisy rows each (default 1 + q % 6); keypoint i is a noisy view of point
    i % Q, within 3 px of its projection."""
    rng = np.random.default_rng(seed)
    uv = grid_uv(Q)
    base = rng.integers(0, 256, (Q, B), dtype=np.uint8)
    cnts = [1 + q % 6 for q in range(Q)] if obs_counts is None else obs_counts
    wmap = make_map(points_at(uv), [[HS.noisy(rng, base[q]) for _ in range(cnts[q])] for q in range(Q)])
    own = np.arange(N) % Q
    kp = (uv[own] + rng.uniform(-2.0, 2.0, (N, 2))).astype(np.float32)
    des = np.ascontiguousarray(HS.noisy(rng, base[own]))
    return wmap, kp, des


def both_paths(P, L, wmap, kp, des, radius, max_hamm):
    """The dict-of-objects map (host entry) and the SoA map (device entry) against the restatement, bit for bit.
    -> (restatement's kp indices, mp ids, tie count, decisions)."""
    p3, p2, kpi, mpi, ties, dec = HR.reproject_and_match_hamming(wmap, K, np.eye(4), kp, des, W, H, radius, max_hamm)
    for m in (wmap, L.Map.from_reference(wmap)):
        r = P.reproject_and_match_2d3d(m, K, np.eye(4), kp, des, W, H, radius_px=radius, max_hamm=max_hamm)
        np.testing.assert_array_equal(r.kp_indices, kpi)
        np.testing.assert_array_equal(r.mp_ids, mpi)
        assert r.pts3d.dtype == np.float32 and r.pts2d.dtype == np.float32
        np.testing.assert_array_equal(r.pts3d, p3)
        np.testing.assert_array_equal(r.pts2d, p2)
    return kpi, mpi, ties, dec


# ------------------------------------------------------------------ the reference's own outputs
@pytest.mark.parametrize("c", range(len(HS.CASES)))
def test_matches_reference_outputs(P, c):
    sc = HS.make_case(*HS.CASES[c])
    assert sc["digest"] == float(G[f"digest{c}"])
    m = P.reproject_and_match_2d3d(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                   radius_px=sc["radius"], max_hamm=sc["max_hamm"])
    np.testing.assert_array_equal(m.kp_indices, G[f"kp{c}"])
    np.testing.assert_array_equal(m.mp_ids, G[f"mp{c}"])
    np.testing.assert_array_equal(m.pts3d, G[f"pts3d{c}"])
    np.testing.assert_array_equal(m.pts2d, G[f"pts2d{c}"])


@pytest.mark.parametrize("c", range(len(HS.CASES)))
def test_soa_map_path_matches_reference_outputs(P, L, c):
    sc = HS.make_case(*HS.CASES[c])
    m = L.Map.from_reference(sc["wmap"])
    assert m.binary_width == sc["B"]
    r = P.reproject_and_match_2d3d(m, sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                   radius_px=sc["radius"], max_hamm=sc["max_hamm"])
    np.testing.assert_array_equal(r.kp_indices, G[f"kp{c}"])
    np.testing.assert_array_equal(r.mp_ids, G[f"mp{c}"])
    np.testing.assert_array_equal(r.pts3d, G[f"pts3d{c}"])
    np.testing.assert_array_equal(r.pts2d, G[f"pts2d{c}"])


# ------------------------------------------------------------------ kernel edges against the restatement
@pytest.mark.parametrize("N", [1, 63, 64, 65])
@pytest.mark.parametrize("Q", [1, 5, 7])
def test_point_and_keypoint_counts_off_the_tile(P, L, Q, N):
    """4 points per workgroup, 64 keypoints per ballot pass: counts below, at and above."""
    wmap, kp, des = small_scene(100 * Q + N, Q, N, 32)
    kpi, _, _, _ = both_paths(P, L, wmap, kp, des, 5.0, 64)
    assert len(kpi) == min(Q, N)


def cluster_scene(n_in, B=32, seed=3):
    """Three points; `n_in` keypoints within 5 px of point 0's projection, every one of them far in descriptor space but
    the LAST, which is an exact copy of point 0's stored row; 20 more keypoints outside the radius in front of them."""
    rng = np.random.default_rng(seed)
    uv = grid_uv(3)
    base = rng.integers(0, 256, (3, B), dtype=np.uint8)
    wmap = make_map(points_at(uv), [[base[q]] for q in range(3)])
    ang = rng.uniform(0, 2 * np.pi, n_in)
    inside = uv[0] + np.stack([np.cos(ang), np.sin(ang)], 1) * rng.uniform(0.0, 4.5, (n_in, 1))
    outside = uv[0] + np.stack([np.cos(ang[:20]), np.sin(ang[:20])], 1) * 7.0
    kp = np.concatenate([outside, inside]).astype(np.float32)
    des = rng.integers(0, 256, (len(kp), B), dtype=np.uint8)
    des[:20] = base[0]                                                   # (out of range: must never be taken)
    des[-1] = base[0]
    return wmap, kp, np.ascontiguousarray(des)


@pytest.mark.parametrize("n_in", [65, 128])
def test_dense_cluster_second_pass_and_full_list(P, L, n_in):
    wmap, kp, des = cluster_scene(n_in)
    kpi, mpi, _, dec = both_paths(P, L, wmap, kp, des, 5.0, 64)
    assert kpi[0] == len(kp) - 1 and mpi[0] == 5 and dec[0][2] == 0      # candidate n_in - 1 of the list: the last lane of the pass


def test_candidate_list_overflow_is_reported(P, L, native):
    wmap, kp, des = cluster_scene(129)
    for m in (wmap, L.Map.from_reference(wmap)):
        with pytest.raises(native.NativeError, match="keypoints within"):
            P.reproject_and_match_2d3d(m, K, np.eye(4), kp, des, W, H, radius_px=5.0, max_hamm=64)


@pytest.mark.parametrize("B", [2, 20, 32, 61, 64])
def test_observation_counts_0_to_6_and_every_stored_row_is_read(P, L, B):
    """Point q has q stored rows, all random but the LAST, which its keypoint copies exactly; with max_hamm = 0 a point is
    matched only if that row is read whole (every byte of the width, on the 16-byte, 4-byte and byte load paths) and no
    byte beyond it (rows are zero padded).  Point 0 has none and is never matched."""
    rng = np.random.default_rng(B)
    Q = 7
    uv = grid_uv(Q)
    obs = [[rng.integers(0, 256, B, dtype=np.uint8) for _ in range(q)] for q in range(Q)]
    wmap = make_map(points_at(uv), obs)
    kp = np.concatenate([uv + 1.0, uv - 1.0]).astype(np.float32)
    des = rng.integers(0, 256, (2 * Q, B), dtype=np.uint8)
    for q in range(1, Q):
        des[Q + q] = obs[q][-1]
        des[q] = obs[q][-1]
        des[q, -1] ^= 0x80                                               # the row's last bit differs: distance 1
    des = np.ascontiguousarray(des)
    kpi, mpi, _, dec = both_paths(P, L, wmap, kp, des, 5.0, 0)
    assert kpi == [Q + q for q in range(1, Q)] and mpi == [3 * q + 5 for q in range(1, Q)]
    kpi, _, _, dec = both_paths(P, L, wmap, kp[:Q], des[:Q], 5.0, 1)     # without the exact copies: distance 1 everywhere
    assert kpi == list(range(1, Q)) and all(d == 1 for _, _, d in dec)


@pytest.mark.parametrize("B", [2, 32, 61, 64])
def test_widths_on_noisy_scenes(P, L, B):
    wmap, kp, des = small_scene(B, 5, 65, B)
    kpi, _, ties, _ = both_paths(P, L, wmap, kp, des, 5.0, 2 * B)
    assert len(kpi) == 5
    if B == 2:
        assert ties > 0                                                  # 13 views of a 16-bit row: minima tie


def test_tied_minima_take_the_lowest_index(P, L):
    """Every keypoint row appears twice (i and i + 30, both within the radius of the same projection), so every accepted
    minimum is tied: the lower index must win, and the restatement counts the ties so the case cannot go vacuous."""
    wmap, kp, des = small_scene(9, 10, 30, 32)
    rng = np.random.default_rng(10)
    kp2 = np.concatenate([kp, kp + rng.uniform(-0.5, 0.5, kp.shape).astype(np.float32)])
    des2 = np.ascontiguousarray(np.concatenate([des, des]))
    kpi, _, ties, _ = both_paths(P, L, wmap, kp2, des2, 5.0, 64)
    assert ties == len(kpi) == 10 and max(kpi) < 30
    # the same with the copies in FRONT: the copy is now the lower index
    kpi, _, ties, _ = both_paths(P, L, wmap, np.concatenate([kp2[30:], kp2[:30]]), des2, 5.0, 64)
    assert ties == 10 and max(kpi) < 30


def test_threshold_is_inclusive(P, L):
    wmap, kp, des = small_scene(21, 1, 3, 32)
    _, _, _, dec = both_paths(P, L, wmap, kp, des, 5.0, 64)
    d0 = dec[0][2]
    assert 0 < d0 < 64
    assert both_paths(P, L, wmap, kp, des, 5.0, d0)[0] == [dec[0][1]]    # best_d == max_hamm: accepted
    assert both_paths(P, L, wmap, kp, des, 5.0, d0 - 1)[0] == []         # one less: rejected


def test_host_entry_refuses_bad_widths_and_counts(native):
    ctx = native.default_context()
    pts = np.array([[0.0, 0.0, Z]]); kp = np.zeros((1, 2), np.float32); out = np.zeros(1, np.int32)
    Kd, Td = np.ascontiguousarray(K).reshape(9), np.eye(4).reshape(16)
    Pt = native.ptr

    def call(cnt, B):
        return native.lib().sslam_reproject_match_hamming_host(
            ctx.handle, 1, Pt(pts), Pt(np.array([cnt], np.int32)), Pt(np.zeros((1, 6, 64), np.uint8)), Pt(Kd), Pt(Td), 1,
            Pt(kp), Pt(np.zeros((1, 64), np.uint8)), B, W, H, 5.0, 64.0, Pt(out), None, None)
    for B in (1, 65, 0, -4):
        with pytest.raises(native.NativeError, match="desc_bytes"):
            native.check(call(1, B))
    for cnt in (7, -1):
        with pytest.raises(native.NativeError, match="obs_cnt"):
            native.check(call(cnt, 32))
    native.check(call(6, 64))


# ------------------------------------------------------------------ device chain
def test_device_count_bounds_the_keypoint_rows(native, L):
    """`sslam_reproject_match_hamming_dev` with n_kp_dev: the detector's device count is smaller than the row bound n_kp.
    The rows at and beyond the count are exact copies of landmarks' stored rows AT their projections - the best possible
    match - so a kernel that ignores the count matches them."""
    ctx = native.default_context()
    Q, live, bound, B = 9, 40, 70, 32
    wmap, kp, des = small_scene(31, Q, live, B)
    uv = grid_uv(Q)
    stale_kp = uv[np.arange(bound - live) % Q].astype(np.float32)
    stale_des = np.stack([wmap.points[3 * (i % Q) + 5].observations[-1][2] for i in range(bound - live)])
    kp_all = np.concatenate([kp, stale_kp]); des_all = np.ascontiguousarray(np.concatenate([des, stale_des]))
    want = HR.reproject_and_match_hamming(wmap, K, np.eye(4), kp, des, W, H, 5.0, 64)
    fooled = HR.reproject_and_match_hamming(wmap, K, np.eye(4), kp_all, des_all, W, H, 5.0, 64)
    assert len(want[2]) == Q and max(fooled[2]) >= live                  # the stale rows WOULD win
    m = L.Map.from_reference(wmap)
    ids = m.soa_binary()[0]
    d_pos, d_cnt, d_rows = m.device_arrays_binary(ctx)
    d_kp, d_des = ctx.upload(kp_all), ctx.upload(des_all)
    d_n, d_out, d_info = ctx.malloc(4), ctx.malloc(4 * Q), ctx.malloc(16)
    Pt = native.ptr
    Kd, Td = np.ascontiguousarray(K).reshape(9), np.eye(4).reshape(16)

    def run(n_kp, count):
        if count is not None:
            ctx.h2d(d_n, np.array([count], np.int32))
        native.check(native.lib().sslam_reproject_match_hamming_dev(
            ctx.handle, Q, Pt(d_pos), Pt(d_cnt), Pt(d_rows), Pt(Kd), Pt(Td), n_kp, Pt(d_kp), Pt(d_des), B, W, H, 5.0, 64.0,
            Pt(d_out), None, Pt(d_info), None if count is None else Pt(d_n)), "sslam_reproject_match_hamming_dev")
        ctx.sync()
        out, info = np.empty(Q, np.int32), np.empty(4, np.int32)
        ctx.d2h(out, d_out); ctx.d2h(info, d_info)
        hit = np.flatnonzero(out >= 0)
        assert info[0] == len(hit) and info[1] == 0
        return [int(i) for i in out[hit]], [int(i) for i in ids[hit]]
    try:
        assert run(bound, live) == (want[2], want[3])                    # the count, not the bound
        assert run(live, None) == (want[2], want[3])                     # NULL: the bound
        assert run(live, 1 << 20) == (want[2], want[3])                  # a count beyond the bound is clamped to it
        assert run(bound, None) == (fooled[2], fooled[3])                # (and without a count the stale rows do win)
        assert run(bound, 0) == ([], [])
        assert run(bound, -3) == ([], [])
    finally:
        for d in (d_kp, d_des, d_n, d_out, d_info):
            ctx.free(d)


# ------------------------------------------------------------------ drop-in
def test_map_built_from_uint8_rows_tracks_to_a_pose(P, L):
    """Map.add_points / add_observation from uint8 rows -> reproject_and_match_2d3d -> solve_pnp_ransac recovers the
    scene's pose within the tolerance tests/test_pnp_gpu.py asks of the same solver (2 degrees, 0.1 m)."""
    sc = HS.make_case(5, 1500, 1000, 12.0, 32, 64, 0.5)
    m = L.Map()
    items = list(sc["wmap"].points.items())
    ids = m.add_points(np.stack([mp.position for _, mp in items]))
    for pid, (_, src) in zip(ids, items):
        for f, k, d in src.observations:
            if d is None:
                m.points[pid].observations.append((f, k, None))       # (stored without descriptor: not a call of add_observation)
            else:
                m.points[pid].add_observation(f, k, d)
    m.resync()
    assert m.binary_width == 32
    r = P.reproject_and_match_2d3d(m, sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"], radius_px=sc["radius"],
                                   max_hamm=sc["max_hamm"])
    want = HR.reproject_and_match_hamming(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                          sc["radius"], sc["max_hamm"])
    assert len(r.kp_indices) > 300 and want[4] == 0
    np.testing.assert_array_equal(r.kp_indices, want[2])
    new_id = dict(zip(sc["wmap"].points, ids))                          # scene id -> the id add_points gave
    np.testing.assert_array_equal(r.mp_ids, [new_id[i] for i in want[3]])
    T, mask = P.solve_pnp_ransac(r.pts3d, r.pts2d, sc["K"], S.RANSAC_PX, Tcw_init=sc["Tcw"], iters=S.ITERS, conf=S.CONF)
    assert T is not None and mask.sum() > 0.8 * len(mask)
    assert S.rot_err_deg(T[:3, :3], sc["Tcw"][:3, :3]) < 2.0 and np.linalg.norm(T[:3, 3] - sc["Tcw"][:3, 3]) < 0.1
    # a new observation on a matched landmark travels to the device mirror before the next call
    pid = r.mp_ids[0]
    m.points[pid].add_observation(99, 0, np.zeros(32, np.uint8))
    m.points[pid].observations.append((100, 0, None))                    # last observation without descriptor: skipped now
    m.resync()
    r2 = P.reproject_and_match_2d3d(m, sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"], radius_px=sc["radius"],
                                    max_hamm=sc["max_hamm"])
    assert pid not in r2.mp_ids and len(r2.mp_ids) >= len(r.mp_ids) - 1


def test_refusals_and_empty_records(P, L):
    import reproject_scenes as RS
    fsc = RS.make_case(*RS.CASES[4])                                     # a float-descriptor map
    n = len(fsc["kp"])
    frame = np.zeros((n, 32), np.uint8)
    for m in (fsc["wmap"], L.Map.from_reference(fsc["wmap"])):
        with pytest.raises(NotImplementedError, match="float-descriptor map"):
            P.reproject_and_match_2d3d(m, fsc["K"], fsc["Tcw"], fsc["kp"], frame, fsc["W"], fsc["H"])
    # a map with no descriptor at all: the empty record
    bare = types.SimpleNamespace(points={1: types.SimpleNamespace(position=np.array([0.0, 0.0, Z]), observations=[]),
                                         2: types.SimpleNamespace(position=np.array([1.0, 0.0, Z]), observations=[(0, 0, None)])})
    for m in (bare, L.Map.from_reference(bare)):
        e = P.reproject_and_match_2d3d(m, K, np.eye(4), fsc["kp"], frame, W, H)
        assert e.pts3d.shape == (0, 3) and e.pts2d.shape == (0, 2) and e.kp_indices == [] and e.mp_ids == []
    # widths: an SoA map fixed at 32 bytes against a 61-byte frame; more than 64 bytes
    wmap, kp, des = small_scene(41, 5, 10, 32)
    m = L.Map.from_reference(wmap)
    with pytest.raises(ValueError, match="61.*32|32.*61"):
        P.reproject_and_match_2d3d(m, K, np.eye(4), kp, np.zeros((10, 61), np.uint8), W, H)
    for mm in (wmap, m):
        with pytest.raises(ValueError, match="65"):
            P.reproject_and_match_2d3d(mm, K, np.eye(4), kp, np.zeros((10, 65), np.uint8), W, H)
    # a dict-of-objects map of another width has no row of the frame's width and no float row: no match
    assert P.reproject_and_match_2d3d(wmap, K, np.eye(4), kp, np.zeros((10, 61), np.uint8), W, H).kp_indices == []
    # keypoint objects and the ignored use_cosine
    types_ = load_pkg("slam.core.types")
    kps = [types_.KeyPoint(float(x), float(y), 1.0) for x, y in kp]
    a = P.reproject_and_match_2d3d(wmap, K, np.eye(4), kps, des, W, H, radius_px=5.0, use_cosine=True)
    b = P.reproject_and_match_2d3d(wmap, K, np.eye(4), kp, des, W, H, radius_px=5.0)
    assert a.kp_indices == b.kp_indices and len(b.kp_indices) == 5
