"""Lens undistortion on the GPU (csrc/undistort_kernels.hip, undistort.py) against the numpy restatement tests/undistort_ref.py:
the fp64 map kernel (one float32 step is the bar; the same bits are asserted on top), the fixed-point form and the integer remap
bit for bit."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref as R
import undistort_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAP_SCENES = [(c, a, S.MAP_SIZE) for c in sorted(S.CAMERAS) for a in S.ALPHAS] + [("tum_fr1", 0.0, (640, 480))]
REMAP_CASES = [(size, c) for size in S.SIZES for c in S.CHANNELS]

_REF = {}          # references computed once and shared (never modified)
_UND = {}          # instances, one per scene, closed with the module


@pytest.fixture(scope="module")
def U():
    return load_pkg("undistort")


@pytest.fixture(scope="module", autouse=True)
def _close_instances():
    yield
    for u in _UND.values():
        u.close()
    _UND.clear()


def _new_K(cam, alpha, size):
    K, D = S.camera(cam, size)
    return R.get_optimal_new_camera_matrix(K, D, size, alpha)[0] if S.has_optimal_matrix(size) else K


def _direct(cam, alpha, size):
    key = ("direct", cam, alpha, size)
    if key not in _REF:
        K, D = S.camera(cam, size)
        mx, my = R.init_undistort_rectify_map(K, D, None, _new_K(cam, alpha, size), size, "direct")
        mx.setflags(write=False); my.setflags(write=False)
        _REF[key] = (mx, my)
    return _REF[key]


def _und(U, gpu_ctx, cam, alpha, size):
    key = (cam, alpha, size)
    if key not in _UND:
        K, D = S.camera(cam, size)
        _UND[key] = (U.Undistorter(K, D, size, alpha, ctx=gpu_ctx) if S.has_optimal_matrix(size)
                     else U.Undistorter(K, D, size, new_K=K, ctx=gpu_ctx))
    return _UND[key]


def _hand(U, gpu_ctx):
    if "hand" not in _UND:
        mapx, mapy = S.hand_maps()
        S.assert_categories(mapx, mapy)
        _UND["hand"] = U.Undistorter.from_maps(mapx, mapy, ctx=gpu_ctx)
    return _UND["hand"]


# ---------------------------------------------------------------------------------------------------------------- maps
@pytest.mark.parametrize("cam,alpha,size", MAP_SCENES)
def test_maps_against_the_direct_restatement(U, gpu_ctx, cam, alpha, size):
    """Two fp64 evaluations, each good to about 1e-13, can land on either side of a float32 rounding step and no further: one
    np.spacing everywhere, and different at all in at most 0.1 % of the entries.  (Where fx xd + cx cancels - column 0 of the
    zero camera's identity map is 2e-15 - one np.spacing is far below any fp64 reordering error: there the bar already means
    the same bits.)"""
    und = _und(U, gpu_ctx, cam, alpha, size)
    np.testing.assert_allclose(und.new_K, _new_K(cam, alpha, size), rtol=1e-12, atol=0)
    got, want = und.maps(), _direct(cam, alpha, size)
    differ = 0
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == (size[1], size[0])
        assert (np.abs(g.astype(np.float64) - w) <= np.spacing(np.maximum(np.abs(g), np.abs(w)))).all()
        differ += int((g != w).sum())
    share = differ / (2 * want[0].size)
    print(f"{cam} alpha {alpha} {size}: {differ} of {2 * want[0].size} map entries differ from `direct` ({100 * share:.4f} %)")
    assert share <= 1e-3
    # stricter than the two bars above: the kernel is compiled without fused multiply-adds and its divisions are IEEE, so it
    # performs `direct`'s operations one for one - the maps are the same bits
    assert differ == 0


@pytest.mark.parametrize("cam,alpha,size", MAP_SCENES)
def test_fixed_maps_are_convert_maps_of_the_instances_own_maps(U, gpu_ctx, cam, alpha, size):
    und = _und(U, gpu_ctx, cam, alpha, size)
    ixy, al = und.fixed_maps()
    wixy, wal = R.convert_maps(*und.maps())
    assert ixy.dtype == np.int16 and al.dtype == np.uint16
    np.testing.assert_array_equal(ixy, wixy)
    np.testing.assert_array_equal(al, wal)


def test_fixed_maps_of_the_hand_made_maps(U, gpu_ctx):
    und = _hand(U, gpu_ctx)
    mapx, mapy = S.hand_maps()
    gx, gy = und.maps()
    np.testing.assert_array_equal(gx.view(np.uint32), mapx.view(np.uint32))      # (bitwise: NaN included)
    np.testing.assert_array_equal(gy.view(np.uint32), mapy.view(np.uint32))
    ixy, al = und.fixed_maps()
    wixy, wal = R.convert_maps(mapx, mapy)
    np.testing.assert_array_equal(ixy, wixy)
    np.testing.assert_array_equal(al, wal)


# --------------------------------------------------------------------------------------------------------------- remap
def _remap_dev_copy(gpu_ctx, und, img):
    Hs, Ws = img.shape[:2]
    Cn = 1 if img.ndim == 2 else img.shape[2]
    W, H = und.size
    out = np.empty((H, W) if img.ndim == 2 else (H, W, Cn), np.uint8)
    src = gpu_ctx.upload(img)
    dst = gpu_ctx.malloc(max(out.nbytes, 16))
    try:
        und.remap_dev(src, Hs, Ws, Cn, dst)
        gpu_ctx.d2h(out, dst)
    finally:
        gpu_ctx.free(src); gpu_ctx.free(dst)
    return out


@pytest.mark.parametrize("size,Cn", REMAP_CASES)
def test_remap_is_the_restatement_on_the_instances_fixed_maps(U, gpu_ctx, size, Cn):
    und = _und(U, gpu_ctx, "tum_fr1", 0.0, size)
    img = S.image(size, Cn, seed=1)
    want = R.remap_linear(img, *und.fixed_maps())
    got = und.remap(img)
    assert got.dtype == np.uint8 and got.shape == img.shape and not got.flags.writeable
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(und.remap_host(img), want)
    np.testing.assert_array_equal(_remap_dev_copy(gpu_ctx, und, img), want)
    np.testing.assert_array_equal(und.remap(img), want)                          # a second call: the same bytes


@pytest.mark.parametrize("cam,alpha", [(c, a) for c in sorted(S.CAMERAS) for a in S.ALPHAS])
def test_remap_of_every_camera(U, gpu_ctx, cam, alpha):
    und = _und(U, gpu_ctx, cam, alpha, S.MAP_SIZE)
    img = S.image(S.MAP_SIZE, 3, seed=2)
    np.testing.assert_array_equal(und.remap(img), R.remap_linear(img, *und.fixed_maps()))


@pytest.mark.parametrize("Cn", S.CHANNELS)
def test_remap_of_the_hand_made_maps(U, gpu_ctx, Cn):
    und = _hand(U, gpu_ctx)
    img = S.image(S.HAND_SRC, Cn, seed=5)
    want = R.remap_linear(img, *und.fixed_maps())
    np.testing.assert_array_equal(und.remap(img), want)
    np.testing.assert_array_equal(und.remap_host(img), want)
    np.testing.assert_array_equal(_remap_dev_copy(gpu_ctx, und, img), want)


@pytest.mark.parametrize("src_size", [(11, 9), (20, 15), (5, 31)])
def test_a_source_of_another_size(U, gpu_ctx, src_size):
    """The maps fix the destination; the source's size is an argument of every call (the hand-made maps against three sources:
    what is a half-outside blend on one is inside on the next)."""
    und = _hand(U, gpu_ctx)
    img = S.image(src_size, 3, seed=6)
    want = R.remap_linear(img, *und.fixed_maps())
    assert want.shape == (S.HAND_DST[1], S.HAND_DST[0], 3)
    np.testing.assert_array_equal(und.remap(img), want)
    np.testing.assert_array_equal(und.remap_host(img), want)


def test_the_literal_stand_in_keeps_one_instance_per_pair_of_maps(U, gpu_ctx):
    mapx, mapy = S.hand_maps()
    img = S.image(S.HAND_SRC, 3, seed=5)
    want = R.remap_linear(img, *R.convert_maps(mapx, mapy))
    np.testing.assert_array_equal(U.remap(img, mapx, mapy, ctx=gpu_ctx), want)
    first = U._by_maps[0][5]
    np.testing.assert_array_equal(U.remap(img, mapx, mapy, ctx=gpu_ctx), want)
    assert U._by_maps[0][5] is first                                             # the same arrays, unchanged: the same instance
    mapx[3, 4] = 2.5                                                             # edited in place: identity holds, the content does not
    want2 = R.remap_linear(img, *R.convert_maps(mapx, mapy))
    np.testing.assert_array_equal(U.remap(img, mapx, mapy, ctx=gpu_ctx), want2)
    assert U._by_maps[0][5] is not first and first.handle is None
    for e in U._by_maps:
        e[5].close()
    U._by_maps.clear()


# ------------------------------------------------------------------------------------------ end to end against `direct`
@pytest.mark.parametrize("cam,alpha,size", MAP_SCENES)
def test_end_to_end_against_the_direct_maps(U, gpu_ctx, cam, alpha, size):
    """Equal float maps give equal bytes.  Where a map entry sits on the other side of a float32 step its fixed-point coordinate
    moves by at most 1 / 32 px, so the pixel moves by at most (the largest difference among the samples it can reach) / 32, + 1
    for the two roundings: `undistort_ref.neighbour_bound`, exercised on the CPU by tests/test_undistort_ref.py (the kernel
    performs `direct`'s operations, so here no entry differs and the loop below is empty)."""
    und = _und(U, gpu_ctx, cam, alpha, size)
    img = S.image(size, 3, seed=4)
    got = und.remap(img)
    dmx, dmy = _direct(cam, alpha, size)
    wixy, wal = R.convert_maps(dmx, dmy)
    want = R.remap_linear(img, wixy, wal)
    gmx, gmy = und.maps()
    same = (gmx == dmx) & (gmy == dmy)
    np.testing.assert_array_equal(got[same], want[same])
    worst = 0
    for y, x in zip(*np.nonzero(~same)):
        d = np.abs(got[y, x].astype(np.int64) - want[y, x])
        worst = max(worst, int(d.max()))
        assert (d <= R.neighbour_bound(img, wixy, y, x)).all(), (y, x, d)
    print(f"{cam} alpha {alpha} {size}: {int((~same).sum())} pixels with another float map entry, worst byte difference {worst}")


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refused_arguments(native, gpu_ctx, U):
    L = native.lib()
    P = native.ptr
    K9 = np.array([500.0, 0, 80, 0, 500.0, 48, 0, 0, 1])
    D = np.zeros(8)
    h = C.c_void_p()

    def refused(rc, word):
        assert rc != 0
        msg = L.sslam_last_error().decode()
        assert word in msg, msg

    refused(L.sslam_undistort_create(gpu_ctx.handle, P(K9), P(D), 3, None, P(K9), 161, 97, C.byref(h)), "coefficients")
    refused(L.sslam_undistort_create(gpu_ctx.handle, P(K9), P(D), 4, None, P(K9), 0, 97, C.byref(h)), "size")
    refused(L.sslam_undistort_create(gpu_ctx.handle, P(K9), P(D), 4, None, P(K9), 161, 16385, C.byref(h)), "size")
    mx = np.zeros((3, 5), np.float32)
    refused(L.sslam_undistort_create_from_maps(gpu_ctx.handle, P(mx), P(mx), 0, 3, C.byref(h)), "size")
    refused(L.sslam_undistort_create_from_maps(gpu_ctx.handle, None, P(mx), 5, 3, C.byref(h)), "NULL")
    assert not h.value
    und = _hand(U, gpu_ctx)
    src = np.zeros(64, np.uint8)
    dst = np.zeros(13 * 7 * 4, np.uint8)
    refused(L.sslam_undistort_remap_host(und.handle, P(src), 4, 4, 2, P(dst)), "channels")
    refused(L.sslam_undistort_remap_host(und.handle, P(src), 16385, 4, 1, P(dst)), "size")
    refused(L.sslam_undistort_remap_host(und.handle, P(src), 4, 0, 1, P(dst)), "size")
    refused(L.sslam_undistort_remap_host(und.handle, None, 4, 4, 1, P(dst)), "NULL")
    refused(L.sslam_undistort_remap_dev(und.handle, P(src), 4, 4, 2, P(dst)), "channels")
    refused(L.sslam_undistort_remap_dev(None, P(src), 4, 4, 1, P(dst)), "NULL")
    with pytest.raises(native.NativeError, match="channels|size"):
        und.remap_dev(1 << 20, 16385, 4, 3, 1 << 21)
