"""The numpy restatement of calcOpticalFlowPyrLK (tests/klt_ref.py) and its scenes (tests/klt_scenes.py) on the CPU: the
pieces have the properties OpenCV's have, every branch of the tracker occurs in every scene, and the planted shift is found.
Parity with cv2 is unpinned; klt_ref's docstring names what could not be confirmed."""
import numpy as np
import pytest

import klt_ref as R
import klt_scenes as S

CASES = list(S.CASES)


def test_grey_of_equal_planes_is_that_plane_under_either_coefficient_set():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for c in (3, 4):
        img = np.repeat(v[:, :, None], c, axis=2)
        if c == 4:
            img[..., 3] = 7                                              # alpha is not read
        for bits in (15, 14):
            np.testing.assert_array_equal(R.bgr_to_gray(img, bits), v)
    assert R.bgr_to_gray(v) is v                                         # 2-D input passes through


def test_grey_coefficients_sum_to_one_and_round_to_nearest():
    img = np.zeros((1, 3, 3), np.uint8)
    img[0, 0] = (255, 0, 0); img[0, 1] = (0, 255, 0); img[0, 2] = (0, 0, 255)
    np.testing.assert_array_equal(R.bgr_to_gray(img, 15)[0], [29, 150, 76])      # 0.114, 0.587, 0.299 of 255, rounded
    np.testing.assert_array_equal(R.bgr_to_gray(img, 14)[0], [29, 150, 76])


def test_pyr_down_of_a_constant_and_of_strips():
    for h, w in ((7, 9), (8, 8), (1, 9), (9, 1), (1, 1), (2, 3)):
        out = R.pyr_down(np.full((h, w), 93, np.uint8))
        assert out.shape == ((h + 1) // 2, (w + 1) // 2)
        assert (out == 93).all()
    strip = np.arange(0, 90, 10, dtype=np.uint8)[None, :]                 # 1 x 9: the column filter sees one row five times
    row = R.pyr_down(strip)[0]
    np.testing.assert_array_equal(row, R.pyr_down(np.repeat(strip, 5, axis=0))[0])
    np.testing.assert_array_equal(R.pyr_down(strip.T)[:, 0], row)
    # interior of a ramp: [1 4 6 4 1] / 16 leaves a linear function unchanged
    np.testing.assert_array_equal(row[1:-1], strip[0, 2:-2:2])


def test_reflect101_folds_any_distance():
    np.testing.assert_array_equal(R.reflect101(np.arange(-7, 8), 3), [1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1])
    np.testing.assert_array_equal(R.reflect101(np.arange(-3, 4), 1), 0)


def test_scharr_of_a_horizontal_ramp():
    slope = 3
    img = (np.arange(20, dtype=np.int32) * slope)[None, :].repeat(11, 0).astype(np.uint8)
    dx, dy = R.scharr(img)
    assert dx.dtype == np.int16 and dy.dtype == np.int16
    assert (dx[:, 1:-1] == 32 * slope).all()
    assert (dx[:, [0, -1]] == 0).all()                                    # reflect-101: the two neighbours of an edge pixel are one pixel
    assert (dy == 0).all()
    dxt, dyt = R.scharr(np.ascontiguousarray(img.T))
    np.testing.assert_array_equal(dyt, dx.T)
    np.testing.assert_array_equal(dxt, dy.T)


@pytest.mark.parametrize("name", CASES)
def test_effective_levels(name):
    p0, p1 = S.pyramids(name)
    assert p0.max_level == p1.max_level == S.EFFECTIVE_LEVELS[name]
    h, w, win, _ = S.CASES[name]
    for lv in p0.levels[1:]:
        assert lv.shape[1] > win[0] and lv.shape[0] > win[1]


@pytest.mark.parametrize("name", CASES)
def test_scene_has_the_flat_patch_and_points_outside(name):
    f0, f1, pts, _, _ = S.scene(name)
    h, w = f0.shape
    assert (f0[:h // 3, :w // 3] == 128).all() and (f1[:h // 3, :w // 3] == 128).all()
    assert pts.shape == (S.N_POINTS, 2) and pts.dtype == np.float32
    assert (pts[:, 0] < 0).any() and (pts[:, 0] > w - 1).any() and (pts[:, 1] < 0).any() and (pts[:, 1] > h - 1).any()


@pytest.mark.parametrize("name", CASES)
def test_every_level0_outcome_occurs(name):
    got = S.outcomes(name)
    for reason in (R.EXIT_EPS, R.EXIT_OSCILLATION, R.EXIT_BUDGET, R.EXIT_MIN_EIG):
        assert got.get(reason, 0) >= 1, (name, reason, got)
    nxt, st, err, ex = S.forward(name)
    assert ((st.reshape(-1) == 0) == np.isin(ex, (R.EXIT_OUTSIDE, R.EXIT_MIN_EIG, R.EXIT_LEFT_IMAGE))).all()
    ok = st.reshape(-1) == 1
    assert (err.reshape(-1)[ok] < 12.0).any() and (err.reshape(-1)[ok] >= 12.0).any()     # both sides of main4's gate


@pytest.mark.parametrize("name", CASES)
def test_planted_shift_is_found(name):
    _, _, pts, _, _ = S.scene(name)
    nxt, st, _, _ = S.forward(name)
    ok = st.reshape(-1) == 1
    d = nxt.reshape(-1, 2)[ok] - pts[ok]
    near = (np.abs(d[:, 0] - S.SHIFT) < 0.5) & (np.abs(d[:, 1]) < 0.5)
    assert near.mean() >= 0.75, (name, near.mean())


@pytest.mark.parametrize("name", CASES)
def test_far_and_non_finite_points_take_the_out_of_image_branch(name):
    f0, f1, _, win, max_level = S.scene(name)
    h, w = f0.shape
    pts = np.array([[w + win[0], h + win[1]], [1e9, 5], [5, -1e9], [np.nan, 5], [5, np.inf], [-np.inf, np.nan]], np.float32)
    p0, p1 = S.pyramids(name)
    _, st, err, ex = R.calc_optical_flow_pyr_lk(p0, p1, pts, winSize=win, maxLevel=max_level, return_exits=True)
    assert (st == 0).all() and (err == 0).all() and (ex == R.EXIT_OUTSIDE).all()


@pytest.mark.parametrize("name", CASES)
def test_identical_frames_give_exactly_zero_flow(name):
    """OpenCV iterates on nextPt - halfWin and reports (nextPt - halfWin + delta) + halfWin, so even with delta = 0 a point
    comes back with the rounding of that subtraction and addition.  On points of the 1/8-pixel grid both are exact at every
    level (coordinates below 2^8 need 11 + 3 + 3 bits), and there the flow is exactly zero with err 0; the scene's raw points
    come back within the rounding, far below any tracking tolerance."""
    _, _, pts, win, max_level = S.scene(name)
    p0, _ = S.pyramids(name)
    grid = (np.round(pts * 8) / 8).astype(np.float32)
    nxt, st, err = R.calc_optical_flow_pyr_lk(p0, p0, grid, winSize=win, maxLevel=max_level)
    ok = st.reshape(-1) == 1
    assert ok.sum() > S.N_POINTS // 2
    np.testing.assert_array_equal(nxt.reshape(-1, 2)[ok].view(np.uint32), grid[ok].view(np.uint32))
    assert (err == 0).all()
    nxt, st, err = R.calc_optical_flow_pyr_lk(p0, p0, pts, winSize=win, maxLevel=max_level)
    ok = st.reshape(-1) == 1
    assert np.abs(nxt.reshape(-1, 2)[ok] - pts[ok]).max() < 1e-3


@pytest.mark.parametrize("name", CASES)
def test_forward_backward_gate_keeps_most_points_in_order(name):
    f0, f1, pts, win, max_level = S.scene(name)
    p0, p1 = S.pyramids(name)
    a, b, counts = R.track_forward_backward(p0, p1, pts, winSize=win, maxLevel=max_level, **S.MAIN4)
    raw, st1, err_ok, fb_ok, kept = counts
    assert raw == S.N_POINTS and raw >= st1 >= err_ok >= fb_ok == kept == len(a) == len(b)
    assert 82 <= kept <= 127
    # the kept prev points are a subsequence of the input, in its order
    pos = [int(np.nonzero((pts == q).all(1))[0][0]) for q in a]
    assert pos == sorted(pos)


def test_criteria_are_clamped_as_opencv_clamps_them():
    assert R.criteria_values((3, 500, 50.0)) == (100, 100.0)
    assert R.criteria_values((3, -4, -1.0)) == (0, 0.0)
    assert R.criteria_values((2, 7, 0.5)) == (30, 0.25)                   # no COUNT bit: 30 iterations
    assert R.criteria_values((1, 7, 0.5)) == (7, 0.01 * 0.01)            # no EPS bit: 0.01


def test_zero_iterations_leave_the_start_and_still_measure_err():
    name = "one_level"
    _, _, pts, win, max_level = S.scene(name)
    p0, p1 = S.pyramids(name)
    nxt, st, err = R.calc_optical_flow_pyr_lk(p0, p1, pts, winSize=win, maxLevel=max_level, criteria=(3, 0, 0.01))
    ok = st.reshape(-1) == 1
    np.testing.assert_array_equal(nxt.reshape(-1, 2)[ok], pts[ok])
    assert (err.reshape(-1)[ok] > 0).any()
