"""Views of larger arrays through the host entries on the device: every call on a view (a column slice, a row stride, a negative
stride, the planes of an interleaved map, `kps[:, :2]`, `[N,1,2]` float64 points, `desc[::2]`, `desc[:, :D]`) returns the bits
of the same call on `np.ascontiguousarray(view)`.  The wrappers copy such a view for the library; the binding's pointer keeps
nothing alive, so the copy has to be referenced until the call returns (tests/test_binding_probe.py shows the failure without
a device).  The images are views of a 1400 x 420 canvas and the maps 640 x 480: a freed copy of that size is unmapped rather
than recycled."""
import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]])
DIST = np.array([-0.3, 0.1, 0.001, -0.001, 0.0])


def _canvas(seed, channels=3):
    """16 x 16 blocks of noise under a fine grain: corners for the detectors, texture for the tracker"""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(30, 220, (27, 88, channels)), np.ones((16, 16, 1), np.int64))[:420, :1400]
    return (blocks + rng.integers(-12, 13, blocks.shape)).clip(0, 255).astype(np.uint8)


CANVAS = _canvas(1)
VIEWS = {"column slice": lambda c, dy=0, dx=0: c[20 + dy:396 + dy, 100 + dx:1341 + dx],
         "row stride": lambda c, dy=0, dx=0: c[20 + dy:396 + dy, 100 + dx:1341 + dx][::2],
         "negative stride": lambda c, dy=0, dx=0: c[20 + dy:396 + dy, 100 + dx:1341 + dx][:, ::-1]}


def _same(a, b, what=""):
    """equality of bits, through tuples, lists and dicts"""
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, what
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{what}: {int((a != b).sum())} elements differ"
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), what
    else:
        assert a == b, what


def _view(name, canvas=CANVAS, **shift):
    v = VIEWS[name](canvas, **shift)
    assert not v.flags["C_CONTIGUOUS"]
    return v, np.ascontiguousarray(v)


@pytest.mark.parametrize("name", list(VIEWS))
def test_optical_flow_takes_views(gpu_ctx, name):
    OF = load_pkg("optical_flow")
    (prev, prev_c), (nxt, nxt_c) = _view(name), _view(name, dy=2, dx=2)
    h, w = prev.shape[:2]
    ys, xs = np.meshgrid(np.arange(32, h - 32, 32), np.arange(32, w - 32, 48), indexing="ij")
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    assert 64 <= len(pts) <= 300
    want = OF.calc_optical_flow_pyr_lk(prev_c, nxt_c, pts, ctx=gpu_ctx)
    assert want[1].sum() > len(pts) // 2                                  # (most points are tracked: the result says something)
    _same(OF.calc_optical_flow_pyr_lk(prev, nxt, pts.reshape(-1, 1, 2).astype(np.float64), ctx=gpu_ctx), want, "calc_optical_flow_pyr_lk")
    wide = np.hstack([pts, np.ones((len(pts), 5), np.float32)])
    _same(OF.calc_optical_flow_pyr_lk(prev[..., 0], nxt[..., 0], wide[:, :2], ctx=gpu_ctx),
          OF.calc_optical_flow_pyr_lk(np.ascontiguousarray(prev[..., 0]), np.ascontiguousarray(nxt[..., 0]), pts, ctx=gpu_ctx), "grey planes")
    _same(OF.bgr_to_gray(prev, ctx=gpu_ctx), OF.bgr_to_gray(prev_c, ctx=gpu_ctx), "bgr_to_gray")
    res = []
    for a, b in ((prev, nxt), (prev_c, nxt_c)):
        klt = OF.KLTTracker((w, h), ctx=gpu_ctx, max_points=512)
        klt.push(a)
        gray0 = klt.levels()["gray"]
        klt.push(b)
        res.append((gray0, klt.levels()["gray"], klt.track(wide[:, :2] if a is prev else pts, with_masks=True)))
        klt.close()
    assert res[1][2][2][4] > len(pts) // 2
    _same(res[0], res[1], "KLTTracker")
    _same(res[1][0], OF.bgr_to_gray(prev_c, ctx=gpu_ctx), "levels()['gray']")


@pytest.fixture(scope="module")
def undistorter(gpu_ctx):
    und = load_pkg("undistort").Undistorter(K, DIST, (1241, 376), ctx=gpu_ctx)
    yield und
    und.close()


@pytest.mark.parametrize("name", list(VIEWS))
def test_undistort_takes_image_views(gpu_ctx, undistorter, name):
    U = load_pkg("undistort")
    img, img_c = _view(name)
    want = undistorter.remap_host(img_c)
    assert want.any()
    _same(undistorter.remap_host(img), want, "remap_host")
    _same(np.array(undistorter.remap(img)), want, "remap")
    _same(undistorter.remap_host(img[..., 1]), undistorter.remap_host(np.ascontiguousarray(img[..., 1])), "remap_host of one plane")
    mapx, mapy = undistorter.maps()
    _same(np.array(U.remap(img, mapx, mapy, ctx=gpu_ctx)), want, "module remap")


def test_undistort_takes_map_views(gpu_ctx):
    U = load_pkg("undistort")
    rng = np.random.default_rng(3)
    ys, xs = np.meshgrid(np.arange(500, dtype=np.float32), np.arange(700, dtype=np.float32), indexing="ij")
    big = np.stack([xs * np.float32(0.9) + rng.uniform(-3, 3, xs.shape).astype(np.float32),
                    ys * np.float32(0.75) + rng.uniform(-3, 3, ys.shape).astype(np.float32)], -1)       # [500, 700, 2] interleaved
    img = np.ascontiguousarray(CANVAS[:400, :660])
    cases = {"planes of an interleaved map": (big[:480, :640, 0], big[:480, :640, 1]),
             "crop of larger maps": (np.ascontiguousarray(big[..., 0])[10:490, 30:670], np.ascontiguousarray(big[..., 1])[10:490, 30:670])}
    for what, (mx, my) in cases.items():
        assert mx.shape == (480, 640) and not mx.flags["C_CONTIGUOUS"] and not my.flags["C_CONTIGUOUS"]
        und = U.Undistorter.from_maps(mx, my, ctx=gpu_ctx)
        ref = U.Undistorter.from_maps(np.ascontiguousarray(mx), np.ascontiguousarray(my), ctx=gpu_ctx)
        got_x, got_y = und.maps()
        _same(got_x, np.ascontiguousarray(mx), f"{what}: mapx")
        _same(got_y, np.ascontiguousarray(my), f"{what}: mapy")
        _same(und.fixed_maps(), ref.fixed_maps(), f"{what}: fixed maps")
        want = ref.remap_host(img)
        assert want.any()
        _same(und.remap_host(img), want, f"{what}: remap_host")
        _same(np.array(U.remap(img, mx, my, ctx=gpu_ctx)), want, f"{what}: module remap")
        und.close(); ref.close()


@pytest.mark.parametrize("name", list(VIEWS))
def test_thumbnail_takes_views(gpu_ctx, name):
    T = load_pkg("thumbnail")
    img, img_c = _view(name)
    th = T.Thumbnailer((1241, 376), (320, 96), 70, ctx=gpu_ctx)
    want = th.encode(img_c)
    assert len(want) > 1000
    assert th.encode(img) == want
    _same(th.resize(img), th.resize(img_c), "resize")
    assert th.encode(img[..., 2]) == th.encode(np.ascontiguousarray(img[..., 2]))
    th.close()


@pytest.fixture(scope="module")
def detectors(gpu_ctx):
    made = {}

    def get(name):
        if name not in made:
            kw = dict(max_h=376, max_w=1241, ctx=gpu_ctx)
            made[name] = {"orb": lambda: load_pkg("orb").ORB(500, **kw), "sift": lambda: load_pkg("sift").SIFT(500, **kw),
                          "akaze": lambda: load_pkg("akaze").AKAZE(**kw)}[name]()
        return made[name]
    yield get
    for d in made.values():
        d.close()


@pytest.mark.parametrize("name", list(VIEWS))
@pytest.mark.parametrize("det", ["orb", "sift", "akaze"])
def test_detectors_take_views(detectors, det, name):
    d = detectors(det)
    img, img_c = _view(name)
    want = d.detect_arrays(img_c)
    assert len(want[0]) >= 50, f"{det}: {len(want[0])} keypoints"
    _same(d.detect_arrays(img), want, det)
    _same(d.detect_arrays(img[..., 0]), d.detect_arrays(np.ascontiguousarray(img[..., 0])), f"{det}, one plane")


@pytest.mark.parametrize("name", list(VIEWS))
def test_aliked_takes_views(gpu_ctx, name):
    al = load_pkg("aliked").AlikedHIP(max_num_keypoints=512, max_h=376, max_w=1241, ctx=gpu_ctx)
    img, img_c = _view(name)
    want = al.extract(img_c, return_scores=True)
    _same(al.extract(img, return_scores=True), want, "extract")
    _same(al.extract(img[..., 1]), al.extract(np.ascontiguousarray(img[..., 1])), "extract of one plane")
    al.close()


# ---- points and descriptors
def _two_views(n, seed, outliers=0.2):
    """n matches of a rigid scene in two KITTI-like views, a fifth of them wrong -> (X [n,3], x1 [n,2], x2 [n,2], T1, T2) float64"""
    rng = np.random.default_rng(seed)
    X = np.column_stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(6, 30, n)])
    c, s = np.cos(0.05), np.sin(0.05)
    T1, T2 = np.eye(4), np.eye(4)
    T2[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T2[:3, 3] = [-0.6, 0.02, 0.1]

    def proj(T):
        Xc = X @ T[:3, :3].T + T[:3, 3]
        return (Xc[:, :2] / Xc[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    x1, x2 = proj(T1), proj(T2) + rng.normal(0, 0.2, (n, 2))
    bad = rng.random(n) < outliers
    x2[bad] += rng.uniform(-60, 60, (int(bad.sum()), 2))
    return X, x1, x2, T1, T2


def _point_forms(p):
    """float32-exact points as the views a caller holds -> {form: array}, and the contiguous float32 copy"""
    p32 = np.ascontiguousarray(p, np.float32)
    d = p32.shape[1]
    forms = {"[N,1,d] float64": p32.astype(np.float64).reshape(-1, 1, d),
             "kps[:, :d]": np.hstack([p32, np.ones((len(p32), 7 - d), np.float32)])[:, :d],
             "row stride": np.repeat(p32, 2, axis=0)[::2],
             "negative stride": np.ascontiguousarray(p32[:, ::-1])[:, ::-1]}
    for k, v in forms.items():
        assert not v.flags["C_CONTIGUOUS"] or v.dtype != np.float32, k
    return forms, p32


@pytest.mark.parametrize("n", [64, 300])
def test_geometry_entries_take_point_views(gpu_ctx, n):
    X, x1, x2, T1, T2 = _two_views(n, seed=n)
    (f1, c1), (f2, c2), (f3, c3) = _point_forms(x1), _point_forms(x2), _point_forms(X)
    EP, ES, HO, PNP, RP, TR = (load_pkg(m) for m in ("epipolar", "essential", "homography", "pnp", "relative_pose", "triangulation"))
    Kv = np.hstack([K, np.zeros((3, 2))])[:, :3]                              # K itself as a view
    want_F = EP.find_fundamental_ransac(c1, c2, ctx=gpu_ctx)
    want_E = ES.find_essential_mat_ransac(c1, c2, K, ctx=gpu_ctx)
    want_H = HO.find_homography_ransac(c1, c2, ctx=gpu_ctx)
    want_P = PNP.solve_pnp_ransac(c3, c2, K, ctx=gpu_ctx)
    assert want_F[0] is not None and want_F[1].sum() >= n // 2 and want_E[0] is not None and want_P[0] and want_P[2].sum() >= n // 2
    E, maskE = want_E[0], want_E[1]
    want_R = RP.recover_pose(E, c1, c2, K, mask=maskE, ctx=gpu_ctx, want_info=True)
    want_M = RP.two_view_metrics(K, want_R[1], want_R[2], c1, c2, sel=maskE.ravel(), want_points=True, ctx=gpu_ctx)
    want_T = TR.triangulate_2view(c1, c2, K, T1, T2, parallax_min_deg=0.5, reproj_px_max=2.0, want_diag=True, ctx=gpu_ctx)
    assert want_R[0] >= n // 4 and len(want_T[0]) >= n // 4
    for form in f1:
        a, b, x = f1[form], f2[form], f3[form]
        _same(EP.find_fundamental_ransac(a, b, ctx=gpu_ctx), want_F, f"F, {form}")
        _same(ES.find_essential_mat_ransac(a, b, Kv, ctx=gpu_ctx), want_E, f"E, {form}")
        _same(HO.find_homography_ransac(a, b, ctx=gpu_ctx), want_H, f"H, {form}")
        _same(PNP.solve_pnp_ransac(x, b, Kv, ctx=gpu_ctx), want_P, f"PnP, {form}")
        _same(RP.recover_pose(np.asfortranarray(E), a, b, Kv, mask=np.repeat(maskE, 2, axis=1)[:, :1], ctx=gpu_ctx, want_info=True), want_R,
              f"recover_pose, {form}")
        _same(RP.two_view_metrics(Kv, np.asfortranarray(want_R[1]), want_R[2][:, 0], a, b, sel=np.repeat(maskE.ravel(), 2)[::2], want_points=True,
                                  ctx=gpu_ctx), want_M, f"two_view_metrics, {form}")
        _same(TR.triangulate_2view(a, b, Kv, np.asfortranarray(T1), np.asfortranarray(T2), parallax_min_deg=0.5, reproj_px_max=2.0, want_diag=True, ctx=gpu_ctx), want_T,
              f"triangulate_2view, {form}")


@pytest.mark.parametrize("n", [64, 300])
def test_multiview_triangulator_takes_views(gpu_ctx, n):
    MV = load_pkg("multiview")
    X, x1, x2, T1, T2 = _two_views(n, seed=7 + n, outliers=0.0)
    T3 = T2.copy(); T3[:3, 3] = [-1.2, 0.0, 0.3]
    Xc = X @ T3[:3, :3].T + T3[:3, 3]
    x3 = (Xc[:, :2] / Xc[:, 2:]) * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
    uv = np.ascontiguousarray(np.stack([x1, x2, x3], 1).reshape(-1, 2), np.float32)           # track i: views 0, 1, 2
    off, view = np.arange(0, 3 * n + 1, 3, dtype=np.int32), np.tile(np.arange(3, dtype=np.int32), n)
    Tcw = np.stack([T1, T2, T3])
    want = MV.triangulate_tracks(K, Tcw, off, view, uv, max_rep_err=3.0, want_diag=True, ctx=gpu_ctx)
    assert len(want[0]) >= n // 2
    forms, _ = _point_forms(uv)
    pad = np.stack([Tcw, Tcw], 1)[:, 0]                                                       # [3,4,4] with a row stride
    assert not pad.flags["C_CONTIGUOUS"]
    for form, p in forms.items():
        got = MV.triangulate_tracks(np.asfortranarray(K), pad, np.repeat(off.astype(np.int64), 2)[::2], np.repeat(view.astype(np.int64), 2)[::2], p,
                                    max_rep_err=3.0, want_diag=True, ctx=gpu_ctx)
        _same(got, want, f"triangulate_tracks, {form}")


@pytest.mark.parametrize("norm,dtype,D", [(4, np.float32, 128), (6, np.uint8, 32), (6, np.uint8, 61)])
def test_matchers_take_descriptor_views(gpu_ctx, norm, dtype, D):
    BF = load_pkg("bf_matcher")
    rng = np.random.default_rng(D)
    big_q = (rng.standard_normal((2 * 150, D + 5)) if dtype == np.float32 else rng.integers(0, 256, (2 * 150, D + 5))).astype(dtype)
    big_t = (rng.standard_normal((2 * 130, D + 3)) if dtype == np.float32 else rng.integers(0, 256, (2 * 130, D + 3))).astype(dtype)
    q, t = big_q[::2, :D], big_t[::2, 3:]                 # desc[::2] and desc[:, :D] at once; the train rows a column slice
    assert not q.flags["C_CONTIGUOUS"] and not t.flags["C_CONTIGUOUS"] and q.shape == (150, D) and t.shape == (130, D)
    qc, tc = np.ascontiguousarray(q), np.ascontiguousarray(t)
    for cross in (False, True):
        m = BF.BFMatcher(norm, cross, ctx=gpu_ctx)
        want = m.match_arrays(qc, tc)
        assert len(want[0]) > 0
        _same(m.match_arrays(q, t), want, f"match_arrays, crossCheck={cross}")
    m = BF.BFMatcher(norm, False, ctx=gpu_ctx)
    _same(m.knn_match_arrays(q, t, 3), m.knn_match_arrays(qc, tc, 3), "knn_match_arrays")
    _same(m.ratio_match_arrays(q, t, 0.9), m.ratio_match_arrays(qc, tc, 0.9), "ratio_match_arrays")
    flat = lambda res: [[(d.queryIdx, d.trainIdx, d.distance) for d in row] for row in res]
    assert flat(m.knnMatch(q, t, 2)) == flat(m.knnMatch(qc, tc, 2))
    assert flat(BF.BFMatcher(norm, True, ctx=gpu_ctx).knnMatch(q[::-1], t, 1)) == flat(BF.BFMatcher(norm, True, ctx=gpu_ctx).knnMatch(qc[::-1].copy(), tc, 1))


def test_lightglue_takes_views(gpu_ctx):
    W = load_pkg("weights")
    lg = load_pkg("lightglue").LightGlueHIP(W.random_lightglue_state_dict(1, match_gain=4.0, match_bias=3.0), max_kpts=512, ctx=gpu_ctx)
    rng = np.random.default_rng(5)
    M, N = 200, 180
    xy0 = rng.uniform(0, [1241, 376], (M, 2)).astype(np.float32)
    perm = rng.permutation(M)[:N]
    xy1 = (xy0[perm] + rng.normal(0, 1.5, (N, 2))).astype(np.float32)
    d0 = rng.standard_normal((M, 128)).astype(np.float32)
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    d1 = d0[perm] + 0.05 * rng.standard_normal((N, 128)).astype(np.float32)
    d1 = (d1 / np.linalg.norm(d1, axis=1, keepdims=True)).astype(np.float32)
    want = lg.match(xy0, d0, xy1, d1, 0.1)
    want_sized = lg.match(xy0, d0, xy1, d1, 0.1, (1241, 376), (1241, 376))
    kps0 = np.hstack([xy0, np.ones((M, 5), np.float32)])[:, :2]
    kps1 = xy1.astype(np.float64).reshape(-1, 1, 2)
    wide0 = np.hstack([d0, np.zeros((M, 64), np.float32)])[:, :128]
    odd1 = np.repeat(d1, 2, axis=0)[::2]
    assert not kps0.flags["C_CONTIGUOUS"] and not wide0.flags["C_CONTIGUOUS"] and not odd1.flags["C_CONTIGUOUS"]
    _same(lg.match(kps0, wide0, kps1, odd1, 0.1), want, "match")
    _same(lg.match(kps0, wide0, kps1, odd1, 0.1, np.array([1241.0, 376.0, 0.0])[:2], [1241, 376]), want_sized, "match with sizes")
    lg.close()
