"""Pyramidal Lucas-Kanade on the MI355X against the numpy restatement (tests/klt_ref.py): the pyramid and the tracker perform
the restatement's operations one for one, so every bar is EQUALITY - grey, levels and derivatives byte for byte, status equal,
next_pts and err the same float32 bits.  If a difference shows, the kernel's float tail (contraction, operation order) is what
changes, not the bar.  Parity with cv2 itself is unpinned (klt_ref's docstring)."""
import ctypes as C

import numpy as np
import pytest

import klt_ref as R
import klt_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu
CASES = list(S.CASES)


@pytest.fixture(scope="module")
def O(gpu_ctx):
    return load_pkg("optical_flow")


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


def _same_result(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=what + ": status")
    _same_bits(got[0], want[0], what + ": next_pts")
    _same_bits(got[2], want[2], what + ": err")


def _check_levels(O, gpu_ctx, img, win, max_level, what):
    inst = O._Instance((img.shape[1], img.shape[0]), win, max_level, 16, gpu_ctx)
    try:
        inst.push(img)
        got = inst.levels()
        ref = R.Pyramid(img, win, max_level)
        assert inst.info()[0] == ref.max_level == len(got["levels"]) - 1, what
        np.testing.assert_array_equal(got["gray"], ref.gray, err_msg=what + ": grey")
        for l in range(ref.max_level + 1):
            np.testing.assert_array_equal(got["levels"][l], ref.levels[l], err_msg=f"{what}: level {l}")
            np.testing.assert_array_equal(got["dx"][l], ref.dx[l], err_msg=f"{what}: dx of level {l}")
            np.testing.assert_array_equal(got["dy"][l], ref.dy[l], err_msg=f"{what}: dy of level {l}")
    finally:
        inst.close()


@pytest.mark.parametrize("name", CASES)
def test_pyramid_equals_the_restatement_byte_for_byte(O, gpu_ctx, name):
    f0, _, _, win, max_level = S.scene(name)
    _check_levels(O, gpu_ctx, f0, win, max_level, name)
    assert S.pyramids(name)[0].max_level == S.EFFECTIVE_LEVELS[name]


@pytest.mark.parametrize("channels", [3, 4])
def test_pyramid_of_a_colour_frame_with_distinct_planes(O, gpu_ctx, channels):
    h, w, win, max_level = S.CASES["odd_sizes"]
    img = S.frame(0, h, w, channels)
    assert not np.array_equal(img[..., 0], img[..., 1]) and not np.array_equal(img[..., 1], img[..., 2])
    _check_levels(O, gpu_ctx, img, win, max_level, f"odd_sizes x {channels}")
    np.testing.assert_array_equal(O.bgr_to_gray(img, gpu_ctx), R.bgr_to_gray(img))


def test_pyramid_of_tiny_frames(O, gpu_ctx):
    """sizes 1 and 2 in either direction: reflect-101 folds more than once, a length of 1 maps to index 0"""
    rng = np.random.default_rng(11)
    for h, w in ((1, 1), (1, 9), (9, 1), (2, 3), (7, 2)):
        _check_levels(O, gpu_ctx, rng.integers(0, 256, (h, w), dtype=np.uint8), (5, 3), 2, f"{h}x{w}")


@pytest.mark.parametrize("name", CASES)
def test_flow_forward_then_backward_has_the_restatements_bits(O, gpu_ctx, name):
    f0, f1, pts, win, max_level = S.scene(name)
    fwd = O.calc_optical_flow_pyr_lk(f0, f1, pts, None, winSize=win, maxLevel=max_level, criteria=S.CRITERIA, ctx=gpu_ctx)
    assert fwd[0].shape == (S.N_POINTS, 1, 2) and fwd[1].shape == (S.N_POINTS, 1) and fwd[2].shape == (S.N_POINTS, 1)
    _same_result(fwd, S.forward(name)[:3], name + " forward")
    bwd = O.calc_optical_flow_pyr_lk(f1, f0, fwd[0], None, winSize=win, maxLevel=max_level, criteria=S.CRITERIA, ctx=gpu_ctx)
    _same_result(bwd, S.backward(name)[:3], name + " backward")


VARIANTS = {
    "initial_flow": dict(flags=R.OPTFLOW_USE_INITIAL_FLOW),
    "min_eigenvals": dict(flags=R.OPTFLOW_LK_GET_MIN_EIGENVALS),
    "initial_flow_and_min_eigenvals": dict(flags=R.OPTFLOW_USE_INITIAL_FLOW | R.OPTFLOW_LK_GET_MIN_EIGENVALS),
    "single_level": dict(maxLevel=0),
    "one_iteration": dict(criteria=(3, 1, 0.0)),
    "hundred_iterations": dict(criteria=(3, 100, 0.0)),
    "main4": dict(criteria=S.MAIN4["criteria"]),
    "strict_min_eig": dict(minEigThreshold=0.05),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", CASES)
def test_flow_variants_have_the_restatements_bits(O, gpu_ctx, name, variant):
    f0, f1, pts, win, max_level = S.scene(name)
    kw = dict(winSize=win, maxLevel=max_level, criteria=S.CRITERIA)
    kw.update(VARIANTS[variant])
    guess = None
    if kw.get("flags", 0) & R.OPTFLOW_USE_INITIAL_FLOW:
        guess = (pts + np.random.default_rng(3).uniform(-1.5, 1.5, pts.shape)).astype(np.float32)
    p0, p1 = (S.pyramids(name) if kw["maxLevel"] == max_level else (f0, f1))
    want = R.calc_optical_flow_pyr_lk(p0, p1, pts, guess, **kw)
    got = O.calc_optical_flow_pyr_lk(f0, f1, pts, guess, ctx=gpu_ctx, **kw)
    _same_result(got, want, f"{name} {variant}")
    if variant == "hundred_iterations":
        assert (want[1] == 1).any()
    if variant == "strict_min_eig":
        assert (want[1] == 0).sum() > (S.forward(name)[1] == 0).sum()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1500])
def test_point_counts_across_block_and_grid_boundaries(O, gpu_ctx, n):
    """four points per block: 1 (a block with three idle waves), 63 / 64 / 65 (the last block full, full, one point), 1 500"""
    name = "stop_at_2"
    f0, f1, _, win, max_level = S.scene(name)
    pts = S.points(f0.shape[0], f0.shape[1], n)
    want = R.calc_optical_flow_pyr_lk(*S.pyramids(name), pts, winSize=win, maxLevel=max_level)
    got = O.calc_optical_flow_pyr_lk(f0, f1, pts.reshape(n, 1, 2), winSize=win, maxLevel=max_level, ctx=gpu_ctx)
    _same_result(got, want, f"{n} points")


@pytest.mark.parametrize("name", CASES)
def test_boundary_far_and_non_finite_points(O, gpu_ctx, name):
    f0, f1, _, win, max_level = S.scene(name)
    h, w = f0.shape
    inf, nan = np.inf, np.nan
    pts = np.array([[-0.5, -0.5], [w - 1, h - 1], [0, 0], [w - 0.5, h - 0.5],
                    [w + win[0], h + win[1]], [-win[0] - 12, 5], [1e9, 5], [5, -1e9], [3e38, 3e38], [-3e38, 5],
                    [nan, 5], [5, nan], [nan, nan], [inf, 5], [5, -inf], [-inf, inf], [w / 2, h / 2]], np.float32)
    want = R.calc_optical_flow_pyr_lk(*S.pyramids(name), pts, winSize=win, maxLevel=max_level)
    got = O.calc_optical_flow_pyr_lk(f0, f1, pts, winSize=win, maxLevel=max_level, ctx=gpu_ctx)
    _same_result(got, want, name + " boundary points")
    assert (got[1][4:16] == 0).all() and (got[2][4:16] == 0).all()         # far outside, NaN, +-inf: status 0, err 0
    # a guess that is not finite, or far away, beside a point inside the image: the mid-iteration bounds test
    inside = np.array([[w / 2, h / 2]] * 4, np.float32)
    guess = np.array([[nan, h / 2], [inf, -inf], [1e9, 5], [-1e6, h / 2]], np.float32)
    want = R.calc_optical_flow_pyr_lk(*S.pyramids(name), inside, guess, winSize=win, maxLevel=max_level, flags=R.OPTFLOW_USE_INITIAL_FLOW)
    got = O.calc_optical_flow_pyr_lk(f0, f1, inside, guess, winSize=win, maxLevel=max_level, flags=R.OPTFLOW_USE_INITIAL_FLOW, ctx=gpu_ctx)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    np.testing.assert_array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert (got[1] == 0).all() and (got[2] == 0).all()


def test_identical_frames_give_zero_flow_on_the_eighth_pixel_grid(O, gpu_ctx):
    f0, _, pts, win, max_level = S.scene("odd_sizes")
    grid = (np.round(pts * 8) / 8).astype(np.float32)
    nxt, st, err = O.calc_optical_flow_pyr_lk(f0, f0, grid, winSize=win, maxLevel=max_level, ctx=gpu_ctx)
    ok = st.reshape(-1) == 1
    assert ok.sum() > S.N_POINTS // 2
    _same_bits(nxt.reshape(-1, 2)[ok], grid[ok], "zero flow")
    assert (err == 0).all()


def test_library_refuses_bad_track_arguments_and_launches_nothing(O, gpu_ctx):
    native = load_pkg("_native")
    lib, P = native.lib(), native.ptr
    inst = O._Instance((64, 48), (5, 5), 1, 8, gpu_ctx)
    try:
        pts = np.full((8, 2), 20, np.float32)
        nxt, st, err = np.full((8, 2), -7, np.float32), np.full(8, 9, np.uint8), np.full(8, -7, np.float32)
        cnt = np.full(5, -7, np.int32)

        def refused(rc, *words):
            msg = lib.sslam_last_error().decode()
            assert rc != 0 and all(w in msg for w in words), (rc, msg)
        args = (0, 3, 30, 0.01, 1e-4)
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, *args, P(nxt), P(st), P(err)), "two pushed frames")
        img = S.frame(0, 48, 64)
        inst.push(img)
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, *args, P(nxt), P(st), P(err)), "two pushed frames")
        refused(lib.sslam_klt_levels_read(inst.handle, 1, 0, P(np.empty((48, 64), np.uint8)), None, None), "previous")
        inst.push(img)
        refused(lib.sslam_klt_track_host(inst.handle, 0, 9, P(pts), None, *args, P(nxt), P(st), P(err)), "capacity")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 0, P(pts), None, *args, P(nxt), P(st), P(err)), "capacity")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, None, None, *args, P(nxt), P(st), P(err)), "NULL")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, *args, P(nxt), None, P(err)), "NULL")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, 4, 3, 30, 0.01, 1e-4, P(nxt), P(st), P(err)), "initial guess")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, 3, 3, 30, 0.01, 1e-4, P(nxt), P(st), P(err)), "flags")
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, 0, 3, 30, float("nan"), 1e-4, P(nxt), P(st), P(err)), "finite")
        refused(lib.sslam_klt_track_fb_host(inst.handle, 9, P(pts), 3, 30, 0.01, 1e-4, 12.0, 1.5, None, P(nxt), P(nxt), P(cnt), None), "capacity")
        refused(lib.sslam_klt_track_fb_host(inst.handle, 8, P(pts), 3, 30, 0.01, 1e-4, 12.0, 1.5, None, P(nxt), P(nxt), None, None), "NULL")
        refused(lib.sslam_klt_levels_read(inst.handle, 0, 2, P(np.empty((48, 64), np.uint8)), None, None), "level 2")
        refused(lib.sslam_klt_push_host(inst.handle, P(img), 48, 65, 1), "maximum")
        refused(lib.sslam_klt_push_host(inst.handle, P(img), 48, 64, 2), "channels")
        refused(lib.sslam_klt_push_host(inst.handle, None, 48, 64, 1), "NULL")
        with pytest.raises(ValueError, match="capacity"):
            inst.flow(np.zeros((9, 2), np.float32), None, (3, 30, 0.01), 0, 1e-4)
        gpu_ctx.sync()
        assert (nxt == -7).all() and (st == 9).all() and (err == -7).all() and (cnt == -7).all()      # nothing was written
        # the instance still works, and a smaller frame than the maximum is legal while two frames of different sizes are not
        got = inst.flow(pts, None, (3, 30, 0.01), 0, 1e-4)
        assert (got[1] == 1).any()
        inst.size = (50, 40)                                                # (the Python wrapper pins one size; the library does not)
        inst.push(np.ascontiguousarray(img[:40, :50]))
        refused(lib.sslam_klt_track_host(inst.handle, 0, 8, P(pts), None, *args, P(nxt), P(st), P(err)), "differ in size")
    finally:
        inst.close()
    inst.close()


def test_smaller_frames_than_the_instance_maximum(O, gpu_ctx):
    """an instance made for 160 x 120 tracks a 75 x 61 pair: strides and the zero ring of the derivatives follow the frame"""
    f0, f1, pts, win, max_level = S.scene("non_square")
    inst = O._Instance((160, 120), win, max_level, 256, gpu_ctx)
    try:
        big = S.frame(0, 120, 160)
        inst.push(big); inst.push(big)                                     # other content in both slots first
        inst.size = (f0.shape[1], f0.shape[0])                             # (the Python wrapper pins one size; the library does not)
        inst.push(f0); inst.push(f1)
        got = inst.flow(pts, None, S.CRITERIA, 0, 1e-4)
        want = S.forward("non_square")
        np.testing.assert_array_equal(got[1], want[1].reshape(-1))
        _same_bits(got[0], want[0].reshape(-1, 2), "next_pts")
        _same_bits(got[2], want[2].reshape(-1), "err")
    finally:
        inst.close()
