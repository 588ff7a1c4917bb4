"""Semi-global stereo on the device against tests/stereo_ref.py: every stage `sslam_sgbm_stage_read` returns and the final image
are EQUAL to the restatement (integers throughout), over the scenes of tests/stereo_scenes.py; the host and device entries agree;
a smaller image on a used instance leaves no stale state; three channels equal grey-then-compute."""
import numpy as np
import pytest

import stereo_ref as R
import stereo_scenes as SC
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CASES = SC.gpu_cases()
STAGE_NAMES = ("pf_left", "pf_right", "C", "S", "raw", "right", "checked")


@pytest.fixture(scope="module")
def stereo(gpu_ctx):
    return load_pkg("stereo")


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_equals_the_restatement(stereo, gpu_ctx, name):
    left, right, kw = CASES[name]
    want = R.compute_stages(left, right, R.Params(**kw))
    sg = stereo.StereoSGBM_create(**kw, ctx=gpu_ctx)
    got = sg.compute(left, right)
    assert got.dtype == np.int16 and got.shape == left.shape
    for k in STAGE_NAMES:
        st = sg.stage_read(k)
        assert st.shape == want[k].shape and st.dtype == want[k].dtype, k
        assert np.array_equal(st, want[k]), (name, k, int((st != want[k]).sum()))
    assert np.array_equal(got, want["final"]), (name, int((got != want["final"]).sum()))


def test_constant_image_takes_the_lowest_d_and_the_largest_x(stereo, gpu_ctx):
    left, right, kw = CASES["constant"]
    sg = stereo.StereoSGBM_create(**kw, ctx=gpu_ctx)
    out = sg.compute(left, right)
    assert (sg.stage_read("raw")[:, 32:] == 0).all()                     # every cost ties: d* = 0
    rv = sg.stage_read("right")
    assert (rv[:, 32:] == 0).all() and (rv[:, :32] == -16).all()         # x2 = x: only computed columns land, each on itself
    assert (out[:, 33:] == 0).all()


def test_device_entry_equals_the_host_entry_and_a_smaller_image_leaves_no_stale_state(stereo, gpu_ctx):
    kw = dict(numDisparities=32, blockSize=5, P1=200, P2=800)
    big = SC.smooth_pair(120, 30, 9, seed=21)
    small = SC.smooth_pair(71, 11, 6, seed=22)
    inst = stereo.cached((120, 30), stereo.StereoSGBM_create(**kw).args, gpu_ctx)
    p = R.Params(**kw)
    first = inst.compute(*big)
    assert np.array_equal(first, R.compute(*big, p))
    got_small = inst.compute(*small)                                     # the same instance, a smaller pair
    want_small = R.compute_stages(*small, p)
    assert np.array_equal(got_small, want_small["final"])
    for k in STAGE_NAMES:
        assert np.array_equal(inst.stage_read(k), want_small[k]), k
    assert np.array_equal(inst.compute(*big), first)
    d = [gpu_ctx.upload(big[0]), gpu_ctx.upload(big[1]), gpu_ctx.malloc(120 * 30 * 2)]
    try:
        inst.compute_dev(d[0], d[1], 30, 120, 1, d[2])
        gpu_ctx.sync()
        out = np.empty((30, 120), np.int16)
        gpu_ctx.d2h(out, d[2])
    finally:
        for ptr in d:
            gpu_ctx.free(ptr)
    assert np.array_equal(out, first)


def test_sliced_views_give_the_contiguous_pairs_result(stereo, gpu_ctx):
    """cv2 takes views such as img[:, :W]; the wrapper's contiguous copies must live across the library call (the canvases are large
    enough that a freed copy is unmapped)"""
    kw = dict(numDisparities=32, blockSize=3, P1=72, P2=288)
    canvas_l, canvas_r = SC.smooth_pair(1400, 420, 9, seed=50)
    left, right = canvas_l[20:396, 100:1341], canvas_r[20:396, 100:1341]
    assert not left.flags["C_CONTIGUOUS"] and not right.flags["C_CONTIGUOUS"]
    sg = stereo.StereoSGBM_create(**kw, ctx=gpu_ctx)
    want = sg.compute(np.ascontiguousarray(left), np.ascontiguousarray(right))
    assert np.array_equal(sg.compute(left, right), want)
    assert np.array_equal(sg.compute(left[::2], right[::2]), sg.compute(np.ascontiguousarray(left[::2]), np.ascontiguousarray(right[::2])))
    small = R.compute(np.ascontiguousarray(left[:9, :80]), np.ascontiguousarray(right[:9, :80]), R.Params(**kw))
    assert np.array_equal(sg.compute(left[:9, :80], right[:9, :80]), small)
    col_l, col_r = np.stack([left] * 3, 2)[:, ::2], np.stack([right] * 3, 2)[:, ::2]      # colour views through the helper
    assert not col_l.flags["C_CONTIGUOUS"]
    assert np.array_equal(stereo.compute_stereo_disparity(col_l, col_r, sg),
                          stereo.compute_stereo_disparity(np.ascontiguousarray(col_l), np.ascontiguousarray(col_r), sg))


def test_an_evicted_instance_says_so(stereo, gpu_ctx):
    sg = stereo.StereoSGBM_create(numDisparities=16, ctx=gpu_ctx)
    img = np.zeros((4, 20), np.uint8)
    sg.compute(img, img)
    for w in range(21, 21 + 5):                                          # five more sizes push the first instance out of the cache
        sg2 = stereo.StereoSGBM_create(numDisparities=16, ctx=gpu_ctx)
        sg2.compute(np.zeros((4, w), np.uint8), np.zeros((4, w), np.uint8))
    with pytest.raises(ValueError, match="the instance was closed"):
        sg.stage_read("raw")
    assert sg.compute(img, img).shape == (4, 20) and sg.stage_read("raw").shape == (4, 20)


@pytest.mark.parametrize("channels", [3, 4])
def test_colour_input_equals_grey_then_compute(stereo, gpu_ctx, channels):
    left, right = SC.planted_pair(90, 14, 16, 5, seed=30, channels=channels)
    kw = SC.planted_params(16, 3)
    sg = stereo.StereoSGBM_create(**kw, ctx=gpu_ctx)
    got = stereo.compute_stereo_disparity(left, right, sg)
    gl, gr = R.bgr_to_grey(left), R.bgr_to_grey(right)
    assert got.dtype == np.float32
    assert np.array_equal(got, R.compute(gl, gr, R.Params(**kw)).astype(np.float32) / np.float32(16))
    assert np.array_equal(got, sg.compute(gl, gr).astype(np.float32) / np.float32(16))
    with pytest.raises(ValueError, match="compute_stereo_disparity"):
        sg.compute(left, right)


def test_refusals_of_the_library_name_the_value(stereo, gpu_ctx, native):
    import ctypes as C
    h = C.c_void_p()
    L = native.lib()
    ok = (0, 32, 5, 0, 0, 0, 0, 0, 0, 0, 0)
    for i, v, text in ((10, 1, "mode 1"), (8, 50, "speckleWindowSize 50"), (0, -1, "minDisparity -1"), (1, 24, "numDisparities 24"), (2, 4, "blockSize 4"),
                       (2, 13, "blockSize 13"), (6, 64, "preFilterCap 64"), (7, 101, "uniquenessRatio 101"), (4, 32000, "largest block cost")):
        a = list(ok)
        a[i] = v
        assert L.sslam_sgbm_create(gpu_ctx.handle, 64, 20, *a, C.byref(h)) != 0
        assert text in L.sslam_last_error().decode(), text
    assert L.sslam_sgbm_create(gpu_ctx.handle, 0, 20, *ok, C.byref(h)) != 0 and "image size 0x20" in L.sslam_last_error().decode()
    assert L.sslam_sgbm_create(gpu_ctx.handle, 16384, 16384, *ok, C.byref(h)) != 0 and "workspace of" in L.sslam_last_error().decode()
    inst = stereo.cached((64, 20), ok, gpu_ctx)
    img = np.zeros((21, 64), np.uint8)
    with pytest.raises(ValueError, match="larger than the instance's 64x20"):
        inst.compute(img, img)
