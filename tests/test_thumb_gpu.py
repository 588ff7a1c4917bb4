"""The thumbnail pipeline on the GPU against tests/thumb_ref.py: stage by stage (resized image, Y / Cb / Cr planes, quantised
coefficients, per-block bit offsets), then the stream byte for byte.  Every stage is integer arithmetic defined exactly, so every
comparison is for equality.  Shapes are the smallest at which each path can go wrong: one pixel, one block, partial blocks, the
dummy row and column of the 16 x 16 MCU grid, odd sizes, more than one workgroup, down- and upscaling, one / three / four
channels, the ends of the quality scale, the coder's hard cases, and KITTI's 1241 x 376 -> 640 x 360 once."""
import io

import numpy as np
import pytest

import thumb_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu


def _img(h, w, c, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 255 // max(w - 1, 1) + yy * 64 // max(h - 1, 1)) % 256          # a ramp (smooth) plus noise (busy)
    a = base[:, :, None] + rng.integers(-40, 40, (h, w, max(c, 1)))
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[:, :, 0] if c == 1 else a


# (source h, w, channels, thumbnail (w, h), quality)
CASES = [
    (1, 1, 3, (1, 1), 70),
    (8, 8, 3, (8, 8), 70),                   # identity
    (7, 9, 3, (9, 7), 70),
    (16, 16, 3, (16, 16), 70),
    (24, 40, 3, (40, 24), 70),               # a dummy block row
    (40, 24, 3, (24, 40), 70),               # a dummy block column
    (17, 33, 3, (33, 17), 70),
    (60, 100, 3, (50, 30), 70),
    (4, 5, 3, (23, 19), 70),                 # upscale
    (60, 100, 1, (50, 30), 70),
    (17, 33, 1, (33, 17), 70),
    (60, 100, 4, (50, 30), 70),
    (60, 100, 3, (50, 30), 1),
    (60, 100, 3, (50, 30), 100),
    (60, 100, 1, (50, 30), 100),
    (376, 1241, 3, (640, 360), 70),
]
CASES += [(img.shape[0], img.shape[1], name, wh, q) for name, img, wh, q in R.hard_inputs()]


def _source(case):
    h, w, c, wh, q = case
    if isinstance(c, str):
        return next(img for name, img, _, _ in R.hard_inputs() if name == c)
    return _img(h, w, c, h * 1000 + w)


def _check_stages(th, ref):
    g = ref["g"]
    assert np.array_equal(th.stage_read("resized"), ref["resized"])
    assert np.array_equal(th.stage_read("y"), ref["y"])
    if g["ncomp"] == 3:
        assert np.array_equal(th.stage_read("cb"), ref["cb"])
        assert np.array_equal(th.stage_read("cr"), ref["cr"])
    assert np.array_equal(th.stage_read("coef"), ref["coef"])
    assert np.array_equal(th.stage_read("bitoff").astype(np.int64), ref["bitoff"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}x{c[0]}-{c[2]}-to-{c[3][0]}x{c[3][1]}-q{c[4]}")
def test_every_stage_and_the_stream_equal_the_restatement(case, gpu_ctx):
    T = load_pkg("thumbnail")
    h, w, c, wh, q = case
    img = _source(case)
    ref = R.encode(img, wh, q)
    th = T.Thumbnailer((w, h), wh, q, ctx=gpu_ctx)
    try:
        assert th.capacity == R.capacity(*wh)
        got = th.encode(img)
        _check_stages(th, ref)
        assert len(got) == len(ref["jpeg"]) <= th.capacity
        assert got == ref["jpeg"]
        assert np.array_equal(th.resize(img), ref["resized"])
    finally:
        th.close()


def test_the_hard_case_inputs_reach_every_hard_case_on_the_device(gpu_ctx):
    """the streams of the hard-case inputs are equal to the restatement's, and the restatement counted each case at least once"""
    T = load_pkg("thumbnail")
    hard = {}
    for name, img, wh, q in R.hard_inputs():
        ref = R.encode(img, wh, q, hard)
        th = T.Thumbnailer((img.shape[1], img.shape[0]), wh, q, ctx=gpu_ctx)
        try:
            assert th.encode(img) == ref["jpeg"], name
        finally:
            th.close()
    assert all(hard.get(k, 0) > 0 for k in R.HARD_CASES), hard


def test_a_second_encode_does_not_see_the_bits_of_the_first(gpu_ctx):
    """busy noise, then a constant, through one instance: a bit buffer that is not zeroed again would keep the noise's bits"""
    T = load_pkg("thumbnail")
    noise = np.random.default_rng(3).integers(0, 256, (60, 100, 3), dtype=np.uint8)
    flat = np.full((60, 100, 3), 77, np.uint8)
    grey = np.full((60, 100), 200, np.uint8)
    th = T.Thumbnailer((100, 60), (50, 30), 70, ctx=gpu_ctx)
    try:
        for img in (noise, flat, noise, grey, flat):            # (also: one component after three, on the same buffers)
            assert th.encode(img) == R.encode(img, (50, 30), 70)["jpeg"]
    finally:
        th.close()


def test_the_device_entry_leaves_the_count_on_the_device_and_the_host_entrys_bytes(gpu_ctx):
    T = load_pkg("thumbnail")
    img = _img(60, 100, 3, 11)
    th = T.Thumbnailer((100, 60), (50, 30), 70, ctx=gpu_ctx)
    src = gpu_ctx.upload(img)
    out, cnt = gpu_ctx.malloc(th.capacity), gpu_ctx.malloc(4)
    try:
        want = th.encode(img)
        gpu_ctx.memset_async(cnt, 0xFF, 4)
        th.encode_dev(src, 60, 100, 3, out, cnt)
        n = np.empty(1, np.int32)
        gpu_ctx.d2h(n, cnt)                                     # (the first synchronisation)
        assert n[0] == len(want)
        got = np.empty(int(n[0]), np.uint8)
        gpu_ctx.d2h(got, out)
        assert got.tobytes() == want
        assert np.array_equal(th.stage_read("resized"), R.resize(img, (50, 30)))     # from the caller's device copy
    finally:
        th.close()
        for p in (src, out, cnt):
            gpu_ctx.free(p)


def test_two_instances_on_one_context(gpu_ctx):
    T = load_pkg("thumbnail")
    img = _img(60, 100, 3, 12)
    a = T.Thumbnailer((100, 60), (50, 30), 70, ctx=gpu_ctx)
    b = T.Thumbnailer((100, 60), (33, 17), 25, ctx=gpu_ctx)
    try:
        ja, jb, ja2 = a.encode(img), b.encode(img), a.encode(img)
        assert ja == ja2 == R.encode(img, (50, 30), 70)["jpeg"]
        assert jb == R.encode(img, (33, 17), 25)["jpeg"]
    finally:
        a.close()
        b.close()


def test_the_free_functions_stand_in_for_cv2(gpu_ctx):
    from PIL import Image
    T = load_pkg("thumbnail")
    img = _img(60, 100, 3, 13)
    small = T.resize(img, (50, 30), ctx=gpu_ctx)
    assert np.array_equal(small, R.resize(img, (50, 30)))
    ok, enc = T.imencode_jpg(small, 70, ctx=gpu_ctx)
    assert ok is True and enc.dtype == np.uint8 and enc.ndim == 1
    assert enc.tobytes() == R.encode(small, (50, 30), 70)["jpeg"] == T.Thumbnailer((100, 60), (50, 30), 70, ctx=gpu_ctx).encode(img)
    im = Image.open(io.BytesIO(enc.tobytes()))
    im.load()
    assert im.size == (50, 30) and im.mode == "RGB"
    ok, enc95 = T.imencode_jpg(small, ctx=gpu_ctx)              # cv2's default quality
    assert enc95.tobytes() == R.encode(small, (50, 30), 95)["jpeg"]
    assert T.resize(img, (50, 30), ctx=gpu_ctx) is not small and len(T._instances) <= T._INSTANCES_KEEP


def test_refusals_of_the_library_name_the_value(gpu_ctx, native):
    T = load_pkg("thumbnail")
    import ctypes as C
    h = C.c_void_p()
    for args, text in (((100, 60, 50, 30, 0), "quality 0 outside 1..100"), ((100, 60, 50, 30, 101), "quality 101 outside 1..100"),
                       ((100, 60, 4097, 30, 70), "thumbnail size 4097x30 outside 1..4096"), ((100, 60, 50, 0, 70), "thumbnail size 50x0 outside 1..4096"),
                       ((16385, 60, 50, 30, 70), "source size 16385x60 outside 1..16384")):
        assert native.lib().sslam_thumb_create(gpu_ctx.handle, *args, C.byref(h)) != 0
        assert native.lib().sslam_last_error().decode() == "sslam_thumb_create: " + text
    th = T.Thumbnailer((100, 60), (50, 30), 70, ctx=gpu_ctx)
    try:
        src, out, n = np.zeros((61, 100, 3), np.uint8), np.zeros(th.capacity, np.uint8), C.c_int(0)
        P = native.ptr
        assert native.lib().sslam_thumb_encode_host(th.handle, P(src), 61, 100, 3, P(out), th.capacity, C.byref(n)) != 0
        assert native.lib().sslam_last_error().decode() == "sslam_thumb_encode_host: source 100x61 is larger than the instance's 100x60"
        assert native.lib().sslam_thumb_encode_host(th.handle, P(src), 60, 100, 2, P(out), th.capacity, C.byref(n)) != 0
        assert native.lib().sslam_last_error().decode() == "sslam_thumb_encode_host: 2 channels (want 1, 3 or 4)"
        assert native.lib().sslam_thumb_encode_host(th.handle, P(src), 60, 100, 3, P(out), 10, C.byref(n)) != 0
        assert "out holds 10" in native.lib().sslam_last_error().decode()
    finally:
        th.close()
