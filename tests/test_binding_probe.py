"""The layer between a caller's numpy array and the library, without a GPU (tests/binding_probe.py does the watching).

`_native.ptr` keeps nothing alive, so `lib.f(P(np.ascontiguousarray(view)))` hands the library freed memory: the copy dies when
`P` returns.  Here every host entry of every wrapper is run over a probed library with a canonical contiguous input and with
every view, cast and read-only form its documented contract accepts.  For every run: no probe report (owner released, not
contiguous, wrong dtype, an argument ctypes would refuse), the bytes the library saw for each `const` array are those of the
canonical run, and the caller's arrays are unchanged.  A last test demands that the table reaches every header prototype
with a data pointer."""
import ctypes as C
import gc
import types
from collections import namedtuple

import numpy as np
import pytest

import binding_probe as B
from conftest import PKG_NAME, load_pkg


@pytest.fixture
def probe(monkeypatch):
    gc.collect()
    gc.freeze()                          # (the collection before every probed call then walks this test's objects only)
    p = B.install(monkeypatch)
    yield p
    _release(p)
    gc.unfreeze()


def _release(p):
    """while the library is still the probe: empty the wrappers' instance caches and disarm whatever instance a failed
    test's traceback keeps alive, so that no fake handle ever reaches the real library's destroy entries"""
    for mod, names in (("optical_flow", ("_instances",)), ("thumbnail", ("_instances",)), ("stereo", ("_instances",)),
                       ("undistort", ("_by_maps", "_returned"))):
        m = load_pkg(mod)
        for n in names:
            getattr(m, n).clear()
    gc.collect()
    for o in gc.get_objects():
        if type(o).__module__.startswith(PKG_NAME) and isinstance(getattr(o, "__dict__", {}).get("handle"), C.c_void_p):
            o.handle = None


# ---------------------------------------------------------------------------------------------- the probe's own tests
def _toy(probe, fn, *args):
    return getattr(probe.native.lib(), fn)(*args)


def test_probe_reports_a_copy_that_died_before_the_call(probe):
    P = probe.native.ptr
    canvas = np.arange(6 * 10 * 3, dtype=np.uint8).reshape(6, 10, 3)
    view = canvas[:, 1:9]
    _toy(probe, "sslam_klt_gray_host", probe.ctx.handle, P(np.ascontiguousarray(view)), 6, 8, 3, P(np.empty((6, 8), np.uint8)))
    assert any("sslam_klt_gray_host: parameter img:" in r and "released before the call" in r for r in probe.reports), probe.reports
    probe.clear()
    kept = np.ascontiguousarray(view)
    out = np.empty((6, 8), np.uint8)
    _toy(probe, "sslam_klt_gray_host", probe.ctx.handle, P(kept), 6, 8, 3, P(out))
    assert probe.reports == []
    assert probe.const_bytes() == [("sslam_klt_gray_host", "img", view.tobytes())]


def test_probe_reports_a_wrong_dtype(probe):
    P = probe.native.ptr
    p1, p2 = np.zeros((8, 2), np.float64), np.zeros((8, 2), np.float32)
    mask = np.zeros(8, np.uint8)
    _toy(probe, "sslam_fmat_ransac_host", probe.ctx.handle, 8, P(p1), P(p2), 1.0, 0.99, 100, P(mask), None, None)
    assert probe.reports == ["sslam_fmat_ransac_host: parameter pts1: the array is float64, the header says const float*"]
    probe.clear()
    pos, idx = np.zeros((4, 3)), np.zeros(4, np.int64)                # int64 indices where the header says int32_t
    _toy(probe, "sslam_close_pairs_host", probe.ctx.handle, 4, P(pos), 0.1, 4, P(idx), C.byref(C.c_int64()))
    assert probe.reports == ["sslam_close_pairs_host: parameter pairs_out: the array is int64, the header says int32_t*"]


def test_probe_reports_a_non_contiguous_array(probe):
    P = probe.native.ptr
    img = np.zeros((6, 16), np.uint8)
    _toy(probe, "sslam_klt_push_host", C.c_void_p(1), P(img[:, ::2]), 6, 8, 1)
    assert len(probe.reports) == 1 and "sslam_klt_push_host: parameter img:" in probe.reports[0] and "not C-contiguous" in probe.reports[0]


def test_probe_accepts_a_temporary_view_of_a_live_array(probe):
    P = probe.native.ptr
    K = np.arange(9.0).reshape(3, 3)
    h = C.c_void_p()
    _toy(probe, "sslam_undistort_create", probe.ctx.handle, P(K.reshape(9)), P(np.zeros(4)[:4]), 4, None, P(K.T.copy().T.reshape(9)[:9]),
         8, 6, C.byref(h))
    # (the last one is a temporary COPY: reshape of a Fortran-ordered array copies - the probe must tell the two apart)
    assert len(probe.reports) == 2 and all("released before the call" in r for r in probe.reports), probe.reports
    assert "parameter D:" in probe.reports[0] and "parameter newK9:" in probe.reports[1]
    assert h.value                                                    # (the reply wrote a handle)
    assert probe.const_bytes()[0] == ("sslam_undistort_create", "K9", K.tobytes())


def test_probe_reports_what_ctypes_would_refuse(probe):
    P = probe.native.ptr
    img = np.zeros((2, 2), np.uint8)
    _toy(probe, "sslam_klt_push_host", C.c_void_p(1), P(img), 2.5, 2, 1)
    assert len(probe.reports) == 1 and "parameter h: ctypes refuses float as c_int" in probe.reports[0]
    probe.clear()
    _toy(probe, "sslam_klt_push_host", C.c_void_p(1), P(img), 2, 2)
    assert probe.reports == ["sslam_klt_push_host: 4 arguments, the header declares 5"]


def test_probe_follows_an_asynchronous_upload_to_the_next_synchronisation(probe):
    ctx = probe.ctx
    d = ctx.malloc(64)
    ctx.h2d_async(d, np.ascontiguousarray(np.zeros((8, 16), np.uint8)[:, :8]))
    assert probe.reports == []                                        # (alive across the call itself: ctypes holds the argument)
    ctx.sync()
    assert len(probe.reports) == 1 and "sslam_memcpy_h2d_async: parameter src_host:" in probe.reports[0] and "sslam_ctx_sync" in probe.reports[0]
    probe.clear()
    src = np.zeros(64, np.uint8)
    ctx.h2d_async(d, src)
    ctx.d2h(np.empty(64, np.uint8), d)
    assert probe.reports == []


# ---------------------------------------------------------------------------------------------------- variants of an input
def _embed(a, axis):
    """`a` as a slice of a wider array along `axis`"""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (2, 3)
    big = np.pad(a, pad, constant_values=7)
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(2, 2 + a.shape[axis])
    return big[tuple(sl)]


def _stride2(a):
    return np.repeat(a, 2, axis=0)[::2]


def _negative(a, axis):
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(None, None, -1)
    return np.ascontiguousarray(a[tuple(sl)])[tuple(sl)]


def _readonly(a):
    b = a.copy()
    b.setflags(write=False)
    return b


def _views(a, inner=True):
    v = {"row stride 2": _stride2(a), "negative stride": _negative(a, 1 if a.ndim > 1 else 0), "read-only": _readonly(a)}
    if a.ndim > 1 and inner:
        v["column slice"] = _embed(a, 1)
    if a.ndim > 1:
        v["negative row stride"] = _negative(a, 0)
    return v


def _image(a):
    v = _views(a)
    if a.ndim == 3 and a.shape[2] == 3:
        v["channel slice of BGRA"] = np.concatenate([a, np.full_like(a[..., :1], 9)], axis=2)[..., :3]
    return v


def _points(a):
    """[N,2] float32 under a 'cast to float32' contract"""
    v = _views(a, inner=False)
    v["kps[:, :2] of [N,7]"] = np.hstack([a, np.full((len(a), 5), 3, a.dtype)])[:, :2]
    v["[N,1,2]"] = a.reshape(-1, 1, 2).copy()
    v["[N,1,2] float64"] = a.reshape(-1, 1, 2).astype(np.float64)
    v["float64"] = a.astype(np.float64)
    v["list"] = a.tolist()
    return v


def _points_n2(a):
    """the same for an entry whose contract is (N, 2) arrays only"""
    return {k: v for k, v in _points(a).items() if not k.startswith("[N,1,2]")}


def _matrix(a):
    """a float64 matrix or vector under a 'cast to float64' contract"""
    v = _views(a)
    v["list"] = a.tolist()
    if a.ndim == 2:
        v["Fortran order"] = np.asfortranarray(a)
    return v


def _rows(a):
    """descriptor rows: the dtype is the contract, views are not"""
    return _views(a)


def _rows_cast(a):
    v = _views(a)
    v["float64"] = a.astype(np.float64)
    v["list"] = a.tolist()
    return v


def _index(a):
    """int32 indices under a cast contract"""
    return {"int64": a.astype(np.int64), "list": a.tolist(), "row stride 2": _stride2(a), "read-only": _readonly(a)}


def _index_arrays(a):
    """the same for a field that is documented as an ndarray"""
    return {k: v for k, v in _index(a).items() if k != "list"}


def _plain(a):
    """an internal entry that is handed checked arrays: the canonical form, read-only too"""
    return {"read-only": _readonly(a)}


def _in_out(a):
    """an array the entry writes its result to: any writable view"""
    v = _views(a)
    v.pop("read-only")
    return v


def _fixed(a):
    return {}


# ------------------------------------------------------------------------------------------------------------ the table
Row = namedtuple("Row", "id setup run inputs joint")
ROWS = []


def row(id, run, setup=None, joint=None, **inputs):
    """inputs: name = (canonical value, variants function); joint: {variant name: function(canonical inputs) -> replaced inputs}"""
    ROWS.append(Row(id, setup, run, inputs, joint or {}))


rng = np.random.default_rng(7)
H, W = 6, 8
GRAY = rng.integers(0, 255, (H, W), dtype=np.uint8)
BGR = rng.integers(0, 255, (H, W, 3), dtype=np.uint8)
BGRA = rng.integers(0, 255, (H, W, 4), dtype=np.uint8)
PTS = rng.uniform(1, 5, (9, 2)).astype(np.float32)
PTS2 = rng.uniform(1, 5, (9, 2)).astype(np.float32)
PTS3 = rng.uniform(1, 5, (9, 3)).astype(np.float32)
K = np.array([[718.5, 0, 607.25], [0, 718.5, 185.125], [0, 0, 1]])
T1, T2 = np.eye(4), np.eye(4) + 0.125 * np.arange(16.0).reshape(4, 4)
E = np.arange(9.0).reshape(3, 3) / 8
DIST = np.array([-0.25, 0.125, 0.001953125, -0.0009765625, 0.0625])
MAPX = rng.uniform(0, W, (H, W)).astype(np.float32)
MAPY = rng.uniform(0, H, (H, W)).astype(np.float32)
D32 = rng.standard_normal((10, 128)).astype(np.float32)
T32 = rng.standard_normal((12, 128)).astype(np.float32)
DU8 = rng.integers(0, 255, (10, 32), dtype=np.uint8)
TU8 = rng.integers(0, 255, (12, 32), dtype=np.uint8)
XY10 = rng.uniform(0, 50, (10, 2)).astype(np.float32)
XY12 = rng.uniform(0, 50, (12, 2)).astype(np.float32)
CRIT = (3, 30, 0.01)
DEV = [0x100000 + 0x1000 * i for i in range(24)]     # stand-ins for device addresses (plain ints, as sslam_malloc returns them)


def mod(name):
    return load_pkg(name)


# ---- optical_flow
def _klt(pushes=2, cls="_Instance"):
    def setup(probe):
        OF = mod("optical_flow")
        inst = OF._Instance((W, H), (21, 21), 3, 64, None) if cls == "_Instance" else OF.KLTTracker((W, H), max_points=64)
        for _ in range(pushes):
            inst.push(BGR)
        return inst
    return setup


row("optical_flow.bgr_to_gray", lambda s, img: mod("optical_flow").bgr_to_gray(img), img=(BGR, _image))
row("optical_flow.bgr_to_gray[BGRA]", lambda s, img: mod("optical_flow").bgr_to_gray(img), img=(BGRA, _image))
row("optical_flow._Instance.push", lambda s, img: s.push(img), _klt(0), img=(BGR, _image))
row("optical_flow._Instance.push[gray]", lambda s, img: s.push(img), _klt(0), img=(GRAY, _image))
row("optical_flow._Instance.flow", lambda s, p, i: s.flow(p, i, CRIT, 4, 1e-4), _klt(), p=(PTS, _plain), i=(PTS2, _plain))
row("optical_flow._Instance.flow[no init]", lambda s, p: s.flow(p, None, CRIT, 0, 1e-4, reverse=True), _klt(), p=(PTS, _plain))
row("optical_flow._Instance.flow_fb", lambda s, p: s.flow_fb(p, CRIT, 1e-4, 12.0, 1.5), _klt(), p=(PTS, _plain))
row("optical_flow._Instance.levels", lambda s: s.levels(), _klt(1))
row("optical_flow._Instance.dev entries", lambda s: (s.push_dev(DEV[0], H, W, 3), s.flow_dev(9, DEV[1], DEV[2], CRIT, 4, 1e-4, DEV[3], DEV[4], DEV[5]),
                                                     s.flow_fb_dev(9, DEV[1], CRIT, 1e-4, 12.0, 1.5, DEV[6], DEV[7], DEV[8], DEV[9], DEV[10])), _klt())
row("optical_flow.KLTTracker.push", lambda s, img: s.push(img), _klt(0, "KLTTracker"), img=(BGR, _image))
row("optical_flow.KLTTracker.track", lambda s, p: s.track(p, with_masks=True), _klt(2, "KLTTracker"), p=(PTS, _points))


def _push_undistorted(s, img):
    und, klt = s
    klt.push(und.remap(img))                 # (read on the device where the remap left it: sslam_klt_push_dev)


row("optical_flow.KLTTracker.push[an Undistorter's result]", _push_undistorted,
    lambda probe: (mod("undistort").Undistorter(K, DIST, (W, H)), _klt(0, "KLTTracker")(probe)), img=(BGR, _image))
row("optical_flow.calc_optical_flow_pyr_lk",
    lambda s, a, b, p, q: mod("optical_flow").calc_optical_flow_pyr_lk(a, b, p, q, flags=4),
    a=(GRAY, _image), b=(BGR, _image), p=(PTS, _points), q=(PTS2, _points))
row("optical_flow.calc_optical_flow_pyr_lk[defaults]", lambda s, a, b, p: mod("optical_flow").calc_optical_flow_pyr_lk(a, b, p),
    a=(BGR, _image), b=(BGR[::-1].copy(), _image), p=(PTS, _points))

# ---- undistort
R3 = np.eye(3) + 0.03125 * np.arange(9.0).reshape(3, 3)
NEWK = K * 0.5


def _und(probe):
    return mod("undistort").Undistorter(K, DIST, (W, H))


def _interleaved(c):
    m = np.stack([c["mapx"], c["mapy"]], -1)
    return dict(mapx=m[..., 0], mapy=m[..., 1])


def _cropped(c):
    return dict(mapx=np.pad(c["mapx"], 3)[3:-3, 3:-3], mapy=np.pad(c["mapy"], 3)[3:-3, 3:-3])


row("undistort.Undistorter.__init__", lambda s, K_, D, R, nK: mod("undistort").Undistorter(K_, D, (W, H), R=R, new_K=nK),
    K_=(K, _matrix), D=(DIST, _matrix), R=(R3, _matrix), nK=(NEWK, _matrix))
row("undistort.Undistorter.__init__[optimal new K]", lambda s, K_, D: mod("undistort").Undistorter(K_, D, (W, H), alpha=0.5), K_=(K, _matrix), D=(DIST, _matrix))
row("undistort.Undistorter.from_maps", lambda s, mapx, mapy: mod("undistort").Undistorter.from_maps(mapx, mapy),
    joint={"planes of an interleaved [H,W,2] map": _interleaved, "crop of larger maps": _cropped}, mapx=(MAPX, _views), mapy=(MAPY, _views))
row("undistort.Undistorter.maps", lambda s: (s.maps(), s.fixed_maps()), _und)
row("undistort.Undistorter.remap_host", lambda s, img: s.remap_host(img), _und, img=(BGR, _image))
row("undistort.Undistorter.remap_host[gray]", lambda s, img: s.remap_host(img), _und, img=(GRAY, _image))
row("undistort.Undistorter.remap", lambda s, img: s.remap(img), _und, img=(BGR, _image))
row("undistort.Undistorter.remap[BGRA]", lambda s, img: s.remap(img), _und, img=(BGRA, _image))
row("undistort.Undistorter.remap_dev", lambda s: s.remap_dev(DEV[0], H, W, 3, DEV[1]), _und)
row("undistort.remap", lambda s, img, mapx, mapy: mod("undistort").remap(img, mapx, mapy),
    joint={"planes of an interleaved [H,W,2] map": _interleaved, "crop of larger maps": _cropped},
    img=(BGR, _image), mapx=(MAPX, _views), mapy=(MAPY, _views))

# ---- thumbnail
def _thumb(probe):
    return mod("thumbnail").Thumbnailer((2 * W, 2 * H), (4, 3), 70)


row("thumbnail.Thumbnailer.encode", lambda s, img: (s.encode(img), s.stage_read("resized"), s.stage_read("coef")), _thumb, img=(BGR, _image))
row("thumbnail.Thumbnailer.encode[gray]", lambda s, img: (s.encode(img), s.stage_read("y")), _thumb, img=(GRAY, _image))
row("thumbnail.Thumbnailer.resize", lambda s, img: s.resize(img), _thumb, img=(BGRA, _image))
row("thumbnail.Thumbnailer.encode_dev", lambda s: s.encode_dev(DEV[0], H, W, 3, DEV[1], DEV[2]), _thumb)
row("thumbnail.resize", lambda s, img: mod("thumbnail").resize(img, (4, 3)), img=(BGR, _image))
row("thumbnail.imencode_jpg", lambda s, img: mod("thumbnail").imencode_jpg(img, 80), img=(GRAY, _image))

# ---- stereo
LEFT = rng.integers(0, 255, (H, 40), dtype=np.uint8)
RIGHT = rng.integers(0, 255, (H, 40), dtype=np.uint8)
LEFT3 = rng.integers(0, 255, (H, 40, 3), dtype=np.uint8)
RIGHT3 = rng.integers(0, 255, (H, 40, 3), dtype=np.uint8)
DISP16 = rng.integers(0, 16 * 30, (H, W)).astype(np.int16)
DISPF = (DISP16.astype(np.float32) / np.float32(16.0))
QPTS = rng.uniform(0, 5, (9, 2)).astype(np.float32)
PROJ = np.hstack([K, np.zeros((3, 1))])
PROJR = np.hstack([K, np.array([[-386.125], [0], [0]])])


def _sgbm(probe):
    return mod("stereo").StereoSGBM_create(0, 32, 5, 8 * 25, 32 * 25)


row("stereo.StereoSGBM.compute", lambda s, l, r: (s.compute(l, r), s.stage_read("pf_left"), s.stage_read("S"), s.stage_read("checked")), _sgbm,
    l=(LEFT, _image), r=(RIGHT, _image))
row("stereo.compute_stereo_disparity", lambda s, l, r: mod("stereo").compute_stereo_disparity(l, r, s), _sgbm, l=(LEFT3, _image), r=(RIGHT3, _image))
row("stereo.StereoSGBM.compute_dev", lambda s: s.compute_dev(DEV[0], DEV[1], H, 40, DEV[2]), _sgbm)
row("stereo.lift[int16 image]", lambda s, q, d, a, b: mod("stereo").lift(q, d, a, b), q=(QPTS, _points), d=(DISP16, _views), a=(PROJ, _matrix), b=(PROJR, _matrix))
row("stereo.lift[float32 image]", lambda s, q, d: mod("stereo").lift(q, d, PROJ, PROJR), q=(QPTS, _points), d=(DISPF, _views))
row("stereo.calculate_right_features", lambda s, q1, q2, d1, d2: mod("stereo").calculate_right_features(q1, q2, d1, d2),
    q1=(QPTS, _views), q2=(PTS, _views), d1=(DISPF, _views), d2=(DISPF[::-1].copy(), _views))
row("stereo.get_stereo_3d_pts", lambda s, a, b, c, d, p, pr: mod("stereo").get_stereo_3d_pts(a, b, c, d, p, pr),
    a=(QPTS, _points), b=(PTS, _points), c=(PTS2, _points), d=(QPTS[::-1].copy(), _points), p=(PROJ, _matrix), pr=(PROJR, _matrix))
row("stereo.lift_dev", lambda s, a, b: mod("stereo").lift_dev(mod("_native").default_context(), 9, DEV[0], DEV[1], DEV[2], H, W, a, b, 0.0, 100.0, DEV[3],
                                                              DEV[4], DEV[5], DEV[6]), a=(PROJ, _matrix), b=(PROJR, _matrix))

# ---- detectors
IMG16 = rng.integers(0, 255, (16, 16), dtype=np.uint8)
IMG16C = rng.integers(0, 255, (16, 16, 3), dtype=np.uint8)
PATTERN = rng.integers(-15, 15, (512, 2)).astype(np.int8)


def _det(name, **kw):
    return lambda probe: getattr(mod(name), name.upper())(max_h=16, max_w=16, **kw)


for _name in ("orb", "sift", "akaze"):
    row(f"{_name}.detect_arrays", lambda s, img: s.detect_arrays(img), _det(_name), img=(IMG16C, _image))
    row(f"{_name}.detectAndCompute[gray]", lambda s, img: s.detectAndCompute(img), _det(_name), img=(IMG16, _image))
    row(f"{_name}.stage reads", lambda s: (s.detect_arrays(IMG16), s.stage_read(0), getattr(s, "overflow", int)()), _det(_name))
row("orb.ORB[pattern]", lambda s, pattern: mod("orb").ORB(pattern=pattern, max_h=16, max_w=16).detect_arrays(IMG16), pattern=(PATTERN, _views))
row("orb.default_pattern", lambda s: mod("orb").default_pattern())
row("orb.detect_dev", lambda s: s.detect_dev(DEV[0], 16, 16, 1, DEV[1], DEV[2], DEV[3], DEV[4]), _det("orb"))
row("sift.detect_dev", lambda s: s.detect_dev(DEV[0], 16, 16, 1, DEV[1], DEV[2], DEV[3], DEV[4], DEV[5]), _det("sift"))
row("akaze.detect_dev", lambda s: s.detect_dev(DEV[0], 16, 16, 1, DEV[1], DEV[2], DEV[3], DEV[4], DEV[5]), _det("akaze"))

# ---- ALIKED, LightGlue
def _aliked(probe):
    return mod("aliked").AlikedHIP(max_num_keypoints=16, max_h=16, max_w=16, max_frames=2)


def _lg(probe):
    return mod("lightglue").LightGlueHIP(max_kpts=64, max_pairs=2)


row("aliked.AlikedHIP.extract", lambda s, img: s.extract(img, return_scores=True), _aliked, img=(IMG16C, _image))
row("aliked.AlikedHIP.extract[gray]", lambda s, img: s.extract(img, max_kpts=8), _aliked, img=(IMG16, _image))
row("aliked.AlikedHIP.dev entries", lambda s: (s.extract_dev(DEV[0], 16, 16, 3, DEV[1], DEV[2], DEV[3], DEV[4]),
                                                s.extract_batch_dev(DEV[0:2], 16, 16, 3, DEV[2:4], DEV[4:6], None, DEV[6:8]),
                                                s.debug_read(0, (4, 4)), s.range_overflow(), s.use_graphs(False)), _aliked)
row("lightglue.LightGlueHIP.match", lambda s, a, b, c, d: s.match(a, b, c, d), _lg,
    a=(XY10, _points), b=(D32, _rows_cast), c=(XY12, _points), d=(T32, _rows_cast))
row("lightglue.LightGlueHIP.match[sizes]", lambda s, a, c, s0, s1: s.match(a, D32, c, T32, 0.5, s0, s1), _lg,
    a=(XY10, _points), c=(XY12, _points), s0=(np.array([1241.0, 376.0], np.float32), _rows_cast), s1=(np.array([640.0, 480.0], np.float32), _rows_cast))
row("lightglue.LightGlueHIP.dev entries",
    lambda s: (s.match_dev(DEV[0], DEV[1], 10, DEV[2], DEV[3], 12, DEV[4], DEV[5], DEV[6], m_dev=DEV[7], n_dev=DEV[8]),
               s.match_batch_dev([(DEV[0], DEV[1], 10, DEV[2], DEV[3], 12), (DEV[0], DEV[1], 10, DEV[2], DEV[3], 12, DEV[7], DEV[8])],
                                 DEV[4], DEV[5], DEV[6], 16),
               s.debug_read(0, (4, 4)), s.debug_share_info(), s.profile_read(), s.range_overflow()), _lg)


def _lg_direct(s, a, b, c, d):
    """the unsized host entry has no wrapper: called through the binding, the way tests and tools call the library"""
    N = mod("_native")
    P, ij, sc, k, stop = N.ptr, np.empty((10, 2), np.int32), np.empty(10, np.float32), C.c_int(), C.c_int()
    N.check(N.lib().sslam_lightglue_match_host(s.handle, P(a), P(b), 10, P(c), P(d), 12, 0.5, P(ij), P(sc), C.byref(k), C.byref(stop)))


row("_native: sslam_lightglue_match_host", _lg_direct, _lg, a=(XY10, _plain), b=(D32, _plain), c=(XY12, _plain), d=(T32, _plain))

# ---- matchers
def _bf(norm, cross=False):
    return lambda probe: mod("bf_matcher").BFMatcher(norm, cross)


for _tag, _norm, _q, _t in (("L2", 4, D32, T32), ("HAMMING", 6, DU8, TU8)):
    row(f"bf_matcher.match_arrays[{_tag}]", lambda s, q, t: s.match_arrays(q, t), _bf(_norm, True), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.match[{_tag}]", lambda s, q, t: s.match(q, t), _bf(_norm), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.knn_match_arrays[{_tag}]", lambda s, q, t: s.knn_match_arrays(q, t, 3), _bf(_norm), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.knnMatch[{_tag}]", lambda s, q, t: s.knnMatch(q, t, 2), _bf(_norm), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.knnMatch[{_tag}, crossCheck]", lambda s, q, t: s.knnMatch(q, t, 1), _bf(_norm, True), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.ratio_match_arrays[{_tag}]", lambda s, q, t: s.ratio_match_arrays(q, t, 0.75), _bf(_norm), q=(_q, _rows), t=(_t, _rows))
    row(f"bf_matcher.ratio_match[{_tag}]", lambda s, q, t: s.ratio_match(q, t), _bf(_norm), q=(_q, _rows), t=(_t, _rows))
row("bf_matcher.dev entries", lambda s: (s.match_dev(mod("_native").default_context(), 32, DEV[0], 10, DEV[1], 12, DEV[2], DEV[3], DEV[4], DEV[5], DEV[6]),
                                         s.knn_match_dev(mod("_native").default_context(), 32, DEV[0], 10, DEV[1], 12, 2, DEV[2], DEV[3], DEV[4], DEV[5]),
                                         s.ratio_match_dev(mod("_native").default_context(), 32, DEV[0], 10, DEV[1], 12, DEV[2], DEV[3], DEV[4])), _bf(6))
_flann = lambda lsh: lambda probe: mod("flann_matcher").FlannBasedMatcher(dict(algorithm=6) if lsh else None)
row("flann_matcher.match", lambda s, q, t: s.match(q, t), _flann(False), q=(D32, _rows), t=(T32, _rows))
row("flann_matcher.knnMatch", lambda s, q, t: s.knnMatch(q, t, 2), _flann(True), q=(DU8, _rows), t=(TU8, _rows))
row("flann_matcher.ratio_match", lambda s, q, t: s.ratio_match(q, t, 0.7), _flann(False), q=(D32, _rows), t=(T32, _rows))

# ---- geometry
MASK = (np.arange(9) % 2).astype(np.uint8)
TVEC = np.array([0.5, -0.25, 1.0])
row("epipolar.find_fundamental_ransac", lambda s, a, b: mod("epipolar").find_fundamental_ransac(a, b), a=(PTS, _points), b=(PTS2, _points))
row("epipolar.filter_matches_dev", lambda s: mod("epipolar").filter_matches_dev(mod("_native").default_context(), 9, DEV[0], DEV[1], DEV[2], DEV[3], DEV[4], DEV[5],
                                                                               mask_out_dev=DEV[6], F_out_dev=DEV[7]))
row("essential.find_essential_mat_ransac", lambda s, a, b, k: mod("essential").find_essential_mat_ransac(a, b, k),
    a=(PTS, _points), b=(PTS2, _points), k=(K, _matrix))
row("homography.find_homography_ransac", lambda s, a, b: mod("homography").find_homography_ransac(a, b), a=(PTS, _points), b=(PTS2, _points))
row("pnp.solve_pnp_ransac", lambda s, a, b, k: mod("pnp").solve_pnp_ransac(a, b, k, use_guess=True), a=(PTS3, _rows_cast), b=(PTS, _points), k=(K, _matrix))
row("pnp.solve_pnp_ransac_dev", lambda s, k: mod("pnp").solve_pnp_ransac_dev(mod("_native").default_context(), 9, DEV[0], DEV[1], DEV[2], k, DEV[3], DEV[4],
                                                                             use_guess=True, mask_out_dev=DEV[5], n_out_dev=DEV[6]), k=(K, _matrix))
row("relative_pose.recover_pose", lambda s, e, a, b, k, m: mod("relative_pose").recover_pose(e, a, b, k, mask=m, want_info=True),
    e=(E, _matrix), a=(PTS, _points), b=(PTS2, _points), k=(K, _matrix), m=(MASK, lambda a: dict(_views(a), **{"[n,1]": a.reshape(-1, 1).copy(), "bool": a.astype(bool)})))
row("relative_pose.two_view_metrics", lambda s, k, r, t, a, b, sel: mod("relative_pose").two_view_metrics(k, r, t, a, b, sel, want_points=True, want_info=True),
    k=(K, _matrix), r=(R3, _matrix), t=(TVEC, _matrix), a=(PTS, _points), b=(PTS2, _points),
    sel=(MASK, lambda a: dict(_views(a), **{"bool": a.astype(bool)})))
row("relative_pose.relative_pose_2d2d", lambda s, a, b, k: mod("relative_pose").relative_pose_2d2d(a, b, k, 1.0), a=(PTS, _points), b=(PTS2, _points), k=(K, _matrix))
row("triangulation.triangulate_2view", lambda s, a, b, k, t1, t2: mod("triangulation").triangulate_2view(a, b, k, t1, t2, want_diag=True),
    a=(PTS, _points), b=(PTS2, _points), k=(K, _matrix), t1=(T1, _matrix), t2=(T2, _matrix))
row("triangulation.triangulate_2view_dev",
    lambda s, k: mod("triangulation").triangulate_2view_dev(mod("_native").default_context(), 9, DEV[0], DEV[1], DEV[2], DEV[3], k, DEV[4], DEV[5], DEV[6], DEV[7],
                                                           DEV[8], reason_out_dev=DEV[9], diag_out_dev=DEV[10]), k=(K, _matrix))
OFF = np.array([0, 2, 5, 9], np.int32)
VIEW = np.array([0, 1, 0, 1, 2, 0, 1, 2, 0], np.int32)
TCW = np.stack([T1, T2, T2.T.copy()])
row("multiview.triangulate_tracks", lambda s, k, t, off, view, uv: mod("multiview").triangulate_tracks(k, t, off, view, uv, want_diag=True),
    k=(K, _matrix), t=(TCW, lambda a: {"list": a.tolist(), "row stride 2": _stride2(a), "read-only": _readonly(a), "negative stride": _negative(a, 2)}),
    off=(OFF, _index), view=(VIEW, _index), uv=(PTS, _points))
POS = rng.uniform(0, 1, (9, 3))


def _overlay_map(des=None):
    LU = mod("slam.core.landmark_utils")
    m = LU.Map()
    ids = m.add_points(POS.copy())
    for j, pid in enumerate(ids):
        if des is not None:
            m.points[pid].add_observation(0, j, des[j])
    return m


def _plain_map(des):
    pts = {j: types.SimpleNamespace(position=POS[j].copy(), observations=[(0, j, des[j])]) for j in range(len(POS))}
    return types.SimpleNamespace(points=pts, get_point_array=lambda: np.array([p.position for p in pts.values()]))


row("landmark_fusion.close_pairs", lambda s, pos: mod("landmark_fusion").close_pairs(pos, 0.1, pair_capacity=16),
    pos=(POS, _matrix))
row("landmark_fusion.close_pairs[device mirror]", lambda s: mod("landmark_fusion").close_pairs(s, 0.1), lambda probe: _overlay_map())
row("landmark_fusion.fuse_closeby", lambda s: mod("landmark_fusion").fuse_closeby(s, 0.1), lambda probe: _plain_map(D32))

# ---- 2D-3D association (the overlay's pnp_utils is the wrapper of the four reproject entries)
def _reproject(s, kps, des, k, t):
    return mod("slam.core.pnp_utils").reproject_and_match_2d3d(s, k, t, kps, des, 1241, 376)


def _synced_map(des):
    """an overlay map whose device mirror is up to date: every later call uploads the same (positions, counts, frame)"""
    def setup(probe):
        m = _overlay_map(des)
        _reproject(m, KPS9, des[:9], K, T2)
        return m
    return setup


KPS9 = rng.uniform(0, 300, (9, 2)).astype(np.float32)
row("pnp_utils.reproject_and_match_2d3d[float, host]", _reproject, lambda probe: _plain_map(D32),
    kps=(KPS9, _points_n2), des=(D32[:9].copy(), _rows_cast), k=(K, _matrix), t=(T2, _matrix))
row("pnp_utils.reproject_and_match_2d3d[binary, host]", _reproject, lambda probe: _plain_map(DU8),
    kps=(KPS9, _points_n2), des=(DU8[:9].copy(), _rows), k=(K, _matrix), t=(T2, _matrix))
row("pnp_utils.reproject_and_match_2d3d[float, device map]", _reproject, _synced_map(D32),
    kps=(KPS9, _points_n2), des=(D32[:9].copy(), _rows_cast), k=(K, _matrix), t=(T2, _matrix))
row("pnp_utils.reproject_and_match_2d3d[binary, device map]", _reproject, _synced_map(DU8),
    kps=(KPS9, _points_n2), des=(DU8[:9].copy(), _rows), k=(K, _matrix), t=(T2, _matrix))

# ---- bundle adjustment
def _ba_problem(q, t, X, intr, obs_pose, obs_point, obs_uv):
    return mod("ba_solver").BAProblem(q=q, t=t, pose_const=np.array([True, False, False]), X=X, intr=intr, obs_pose=obs_pose, obs_point=obs_point,
                                      obs_uv=obs_uv)


BA = dict(q=(np.tile([0.0, 0, 0, 1], (3, 1)), _in_out), t=(rng.uniform(-1, 1, (3, 3)), _in_out), X=(rng.uniform(1, 5, (4, 3)), _in_out),
          intr=(np.array([718.5, 718.5, 607.25, 185.125]), _views), obs_pose=(np.array([0, 1, 2, 0, 1, 2, 1], np.int32), _index_arrays),
          obs_point=(np.array([0, 0, 1, 1, 2, 3, 3], np.int32), _index_arrays), obs_uv=(rng.uniform(0, 300, (7, 2)), _views))
row("ba_solver.solve_host (_Evaluator)", lambda s, **a: mod("ba_solver").solve_host(_ba_problem(**a), 3), **BA)
row("ba_solver._Evaluator[residual only]", lambda s, **a: mod("ba_solver")._Evaluator(_ba_problem(**a), mod("_native").default_context())(a["q"], a["t"], a["X"], False),
    **BA)
row("ba_solver.solve_device", lambda s, **a: mod("ba_solver").solve_device(_ba_problem(**a), 3), **BA)
row("ba_solver.solve_pose_only", lambda s, **a: mod("ba_solver").solve_pose_only(_ba_problem(**a), 3), **BA)


# ---- the context's own helpers
def _context(s):
    N = mod("_native")
    ctx = N.default_context()
    d, e = ctx.malloc(256), ctx.malloc(256)
    a, back = np.arange(64, dtype=np.float32), np.empty(64, np.float32)
    ctx.h2d(d, a[::-1]); ctx.h2d_async(e, a); ctx.d2d_async(e, d, 256); ctx.memset_async(d, 0, 256); ctx.d2h_async(back, e); ctx.sync()
    ctx.d2h(back, d)
    pinned = ctx.host_alloc(64)
    ctx.h2d_async(d, pinned); ctx.sync()
    ev, t0, t1 = ctx.event(), ctx.timing_event(), ctx.timing_event()
    ctx.record(ev); ctx.wait(ev); ctx.record(t0); ctx.record(t1); ctx.elapsed_ms(t0, t1)
    ctx.timer_start(); ctx.timer_stop()
    ctx.free(ctx.upload(a.reshape(8, 8)[:, :3]))
    assert N.device_count() == 1
    own = N.Context(0, stream=0x5000)                                # the real class over the probed library
    own.host_alloc(32); own.stream; own.close()


row("_native.Context", _context)


# ---------------------------------------------------------------------------------------------------------- running a row
def _snapshot(inputs):
    return {k: (v.copy(), v.dtype, v.shape, v.strides, v.flags.writeable) if isinstance(v, np.ndarray) else repr(v) for k, v in inputs.items()}


def _run(probe, r, state, inputs):
    """-> the const arrays the library saw, in order; asserts no report and untouched inputs"""
    probe.clear()
    before = _snapshot(inputs)
    r.run(state, **inputs)
    assert probe.reports == [], probe.reports
    for k, v in inputs.items():
        if r.inputs[k][1] is _in_out:
            continue                         # (the entry's result is written there, by contract)
        if isinstance(v, np.ndarray):
            c, dt, sh, st, wr = before[k]
            assert (v.dtype, v.shape, v.strides, v.flags.writeable) == (dt, sh, st, wr) and np.array_equal(v, c, equal_nan=True), f"the call changed its input `{k}`"
        else:
            assert repr(v) == before[k], f"the call changed its input `{k}`"
    seen = probe.const_bytes()
    assert all(b is not None for _, _, b in seen)
    return seen


def _canonical(r):
    return {k: (np.array(v[0], copy=True) if isinstance(v[0], np.ndarray) else v[0]) for k, v in r.inputs.items()}


def _variants(r):
    """[(name, inputs)]: one input replaced at a time, then the joint replacements"""
    out = []
    for k, (value, make) in r.inputs.items():
        for name, v in make(np.array(value, copy=True)).items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, value, equal_nan=True) or v.size == value.size and np.array_equal(v.reshape(value.shape), value), (r.id, k, name)
            out.append((f"{k}: {name}", dict(_canonical(r), **{k: v})))
    for name, fn in r.joint.items():
        c = _canonical(r)
        out.append((name, dict(c, **fn(c))))
    return out


@pytest.mark.parametrize("r", ROWS, ids=[r.id for r in ROWS])
def test_host_entry_keeps_its_arrays_alive_and_typed(probe, r):
    state = r.setup(probe) if r.setup else None
    want = _run(probe, r, state, _canonical(r))
    if r.inputs:
        assert want or r.id.endswith("dev entries"), "the canonical call handed the library no const array: the row checks nothing"
    for name, inputs in _variants(r):
        try:
            got = _run(probe, r, state, inputs)
        except AssertionError as e:
            raise AssertionError(f"{r.id} with {name}: {e}") from None
        assert [(f, p) for f, p, _ in got] == [(f, p) for f, p, _ in want], (r.id, name)
        for (f, p, g), (_, _, w) in zip(got, want):
            assert g == w, f"{r.id} with {name}: {f} saw other bytes for `{p}` than with the canonical input"
    del state


# ---- coverage: every prototype with a data pointer is reached by the table, or excused with a reason
NOT_REACHED = {
    "sslam_aliked_create": "no Python caller: aliked.py always builds through sslam_aliked_create_batched",
    "sslam_lightglue_create": "no Python caller: lightglue.py always builds through sslam_lightglue_create_batched",
    "sslam_lightglue_batch_capacity": "no Python caller; its only data pointer is an int out-parameter",
    "sslam_event_destroy": "no Python caller in the package (Context keeps its events for the process's life)",
    "sslam_ba_residual_jacobian_dev": "no wrapper: the benchmark and the GPU tests call it with device addresses only",
}


def test_the_table_reaches_every_prototype_with_a_data_pointer(probe):
    assert len(NOT_REACHED) <= 10 and not any(n.endswith("_host") for n in NOT_REACHED)
    for r in ROWS:
        state = r.setup(probe) if r.setup else None
        r.run(state, **_canonical(r))
        del state
    assert probe.reports == [], probe.reports
    need = {n for n, proto in probe.model.items() if any(p.cls != "pointer-to-pointer" and p.cls == "pointer" and not B.is_handle(p)
                                                          or p.cls == "pointer-to-pointer" and not B.is_handle(p) for p in proto.params)}
    assert set(NOT_REACHED) <= need, "an excused function has no data pointer (or is gone)"
    missing = sorted(need - probe.reached - set(NOT_REACHED))
    assert not missing, f"no table row reaches {missing}"
    excused_but_reached = sorted(set(NOT_REACHED) & probe.reached)
    assert not excused_but_reached, f"{excused_but_reached} are reached: take them off the list"
