"""The numpy restatement of the undistortion functions (tests/undistort_ref.py) against properties that do not depend on it,
and the product's numpy routine `undistort.get_optimal_new_camera_matrix` against the restatement.  No GPU."""
import numpy as np
import pytest
import scipy.ndimage

import undistort_ref as R
import undistort_scenes as S
from conftest import load_pkg

CAMS = sorted(S.CAMERAS)
SCENES = [(c, a) for c in CAMS for a in S.ALPHAS]

# max |distort(undistort(p)) - p| over the 9 x 9 grid in source pixels, as the restatement's five fixed iterations leave it at
# MAP_SIZE (161 x 97): the inverse is a fixed-point iteration that contracts slowly under strong distortion - the strong barrel
# is 0.83 px off after five steps.  Asserted with a factor 10 on top.
RESIDUAL_PX = {"tum_fr1": 2.03e-2, "barrel": 8.26e-1, "pincushion": 8.61e-4, "rational8": 5.56e-2, "zero": 1e-13}


def _identity_maps(W, H, dx=0.0, dy=0.0):
    mx = np.tile(np.arange(W, dtype=np.float32) + np.float32(dx), (H, 1))
    my = np.tile((np.arange(H, dtype=np.float32) + np.float32(dy))[:, None], (1, W))
    return mx, my


@pytest.mark.parametrize("C", S.CHANNELS)
def test_identity_map_returns_the_image_exactly(C):
    img = S.image((37, 23), C)
    ixy, al = R.convert_maps(*_identity_maps(37, 23))
    assert not al.any()
    np.testing.assert_array_equal(R.remap_linear(img, ixy, al), img)


def test_integer_shift_returns_the_shifted_image_with_a_zero_border():
    img = S.image((37, 23), 3)
    ixy, al = R.convert_maps(*_identity_maps(37, 23, 3.0, -2.0))
    want = np.zeros_like(img)
    want[2:, :37 - 3] = img[:23 - 2, 3:]
    np.testing.assert_array_equal(R.remap_linear(img, ixy, al), want)


def test_half_pixel_shift_rounds_the_mean_up():
    img = S.image((37, 23), 1)
    ixy, al = R.convert_maps(*_identity_maps(37, 23, 0.5, 0.0))
    a = img.astype(np.int64)
    b = np.zeros_like(a)
    b[:, :-1] = a[:, 1:]                                                 # the neighbour beyond the last column counts as 0
    np.testing.assert_array_equal(R.remap_linear(img, ixy, al), ((a + b + 1) >> 1).astype(np.uint8))


def _float_bilinear(img, ixy, al):
    """scipy's float bilinear (order 1, constant 0 outside) at the QUANTISED coordinates"""
    nd = scipy.ndimage
    x = ixy[..., 0].astype(np.float64) + (al & 31) / 32.0
    y = ixy[..., 1].astype(np.float64) + (al >> 5) / 32.0
    src = img.reshape(img.shape[0], img.shape[1], -1).astype(np.float64)
    return np.stack([nd.map_coordinates(src[..., c], [y, x], order=1, mode="grid-constant", cval=0.0) for c in range(src.shape[2])], -1)


@pytest.mark.parametrize("cam,alpha", SCENES)
def test_remap_against_an_independent_float_bilinear(cam, alpha):
    size = S.MAP_SIZE
    K, D = S.camera(cam, size)
    newK, _ = R.get_optimal_new_camera_matrix(K, D, size, alpha)
    ixy, al = R.convert_maps(*R.init_undistort_rectify_map(K, D, None, newK, size))
    img = S.image(size, 3, seed=3)
    got = R.remap_linear(img, ixy, al).astype(np.float64)
    want = _float_bilinear(img, ixy, al)
    assert np.abs(got - want).max() <= 0.5 + 1e-3


def test_remap_of_the_hand_made_maps_against_float_bilinear_on_finite_records():
    mapx, mapy = S.hand_maps()
    S.assert_categories(mapx, mapy)
    ixy, al = R.convert_maps(mapx, mapy)
    Ws, Hs = S.HAND_SRC
    img = S.image(S.HAND_SRC, 3, seed=5)
    got = R.remap_linear(img, ixy, al).astype(np.float64)
    want = _float_bilinear(img, ixy, al)
    inrange = (np.abs(ixy[..., 0].astype(np.int64)) < 32767) & (np.abs(ixy[..., 1].astype(np.int64)) < 32767)
    assert inrange.sum() > 40
    assert np.abs(got - want)[inrange].max() <= 0.5 + 1e-3
    assert not got[~inrange].any()                                       # saturated and void records read nothing
    bad = ~np.isfinite(mapx) | ~np.isfinite(mapy) | (np.abs(mapx) >= 2.0 ** 26) | (np.abs(mapy) >= 2.0 ** 26)
    assert bad.any() and (ixy[bad] == -32768).all() and not al[bad].any()
    # ties of x 32 round to even, in both directions
    t = np.float32([2 + 1 / 64, 2 + 3 / 64, -(2 + 1 / 64), -(2 + 3 / 64)])[None, :]
    ixy_t, al_t = R.convert_maps(t, np.zeros_like(t))
    assert (ixy_t[0, :, 0].astype(int) * 32 + (al_t[0] & 31)).tolist() == [64, 66, -64, -66]


@pytest.mark.parametrize("size", [S.MAP_SIZE, (640, 480)])
def test_zero_distortion_keeps_K_and_the_pixel_grid(size):
    K, D = S.camera("zero", size)
    for alpha in S.ALPHAS:
        newK, roi = R.get_optimal_new_camera_matrix(K, D, size, alpha)
        np.testing.assert_allclose(newK, K, rtol=1e-9, atol=0)
        for variant in ("direct", "rowsum"):
            mx, my = R.init_undistort_rectify_map(K, D, None, K, size, variant)
            gx, gy = _identity_maps(*size)
            # (1e-9 relative per entry; column 0 / row 0 cancel to an absolute 1e-14 or so off 0, hence the floor)
            np.testing.assert_allclose(mx, gx, rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(my, gy, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("cam", CAMS)
def test_distorting_the_undistorted_grid_returns_the_grid(cam):
    W, H = S.MAP_SIZE
    K, D = S.camera(cam, S.MAP_SIZE)
    k = R.k8(D)
    u, v = R.grid_points(W, H)
    x0, y0 = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    xd, yd = R.distort_normalised(*R.undistort_normalised(x0, y0, k), k)
    res = max(np.abs(xd - x0).max() * K[0, 0], np.abs(yd - y0).max() * K[1, 1])
    print(f"{cam}: round-trip residual {res:.3e} px (recorded {RESIDUAL_PX[cam]:.3e})")
    assert res <= 10 * RESIDUAL_PX[cam]
    # more iterations do better: the residual is the iteration count's, not an error of the model's restatement
    xd, yd = R.distort_normalised(*R.undistort_normalised(x0, y0, k, iters=200), k)
    assert max(np.abs(xd - x0).max() * K[0, 0], np.abs(yd - y0).max() * K[1, 1]) <= 1e-9


@pytest.mark.parametrize("cam", S.BARREL)
def test_alpha_0_maps_of_the_barrel_cameras_stay_inside_the_source(cam):
    """Every map coordinate reads inside the source, without a tolerance.  (The inner rectangle comes from the five-iteration
    inverse at the border's grid points and can sit off the true border by that camera's round-trip residual; on these cameras
    the inverse overshoots inwards, and the maps stay inside.)"""
    W, H = S.MAP_SIZE
    K, D = S.camera(cam, S.MAP_SIZE)
    newK, roi = R.get_optimal_new_camera_matrix(K, D, S.MAP_SIZE, 0.0)
    mx, my = R.init_undistort_rectify_map(K, D, None, newK, S.MAP_SIZE)
    print(f"{cam}: mapx [{mx.min():.4f}, {mx.max():.4f}] of [0, {W - 1}], mapy [{my.min():.4f}, {my.max():.4f}] of [0, {H - 1}], roi {roi}")
    assert mx.min() >= 0 and mx.max() <= W - 1 and my.min() >= 0 and my.max() <= H - 1


@pytest.mark.parametrize("cam", CAMS)
def test_rectangle_corners_under_the_new_matrix(cam):
    """alpha = 0: the INNER rectangle of the undistorted grid, projected by new_K, is the viewport (0, 0, W - 1, H - 1); alpha = 1:
    the OUTER one is - every source pixel is kept.  To 1e-9 of the image side: both are a few fp64 operations on the same grid."""
    W, H = S.MAP_SIZE
    K, D = S.camera(cam, S.MAP_SIZE)
    k = R.k8(D)
    for alpha, which in ((0.0, 0), (1.0, 1)):
        newK, roi = R.get_optimal_new_camera_matrix(K, D, S.MAP_SIZE, alpha)
        rect = R.rectangles(K, k, W, H, newK)[which]
        np.testing.assert_allclose(rect, (0, 0, W - 1, H - 1), rtol=0, atol=1e-9 * W)
        assert 0 <= roi[0] and 0 <= roi[1] and roi[0] + roi[2] <= W and roi[1] + roi[3] <= H and roi[2] > 0 and roi[3] > 0
    inner1 = R.rectangles(K, k, W, H, R.get_optimal_new_camera_matrix(K, D, S.MAP_SIZE, 1.0)[0])[0]
    assert inner1[0] >= -1e-9 and inner1[1] >= -1e-9 and inner1[0] + inner1[2] <= W - 1 + 1e-9 and inner1[1] + inner1[3] <= H - 1 + 1e-9


@pytest.mark.parametrize("cam,alpha", SCENES + [("tum_fr1", -1.0)])
def test_rowsum_against_direct(cam, alpha):
    """OpenCV's running sums against the kernel's direct evaluation: never more than one float32 step apart, and different at all
    in at most 0.1 % of the entries (a condition on the scenes).  alpha -1: the 640 x 480 scene."""
    size = S.MAP_SIZE if alpha >= 0 else (640, 480)
    K, D = S.camera(cam, size)
    newK, _ = R.get_optimal_new_camera_matrix(K, D, size, max(alpha, 0.0))
    d = R.init_undistort_rectify_map(K, D, None, newK, size, "direct")
    r = R.init_undistort_rectify_map(K, D, None, newK, size, "rowsum")
    differ = 0
    for a, b in zip(d, r):
        assert (np.abs(a.astype(np.float64) - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all()
        differ += int((a != b).sum())
    share = differ / (2 * d[0].size)
    print(f"{cam} alpha {alpha} {size}: {differ} of {2 * d[0].size} entries differ ({100 * share:.4f} %)")
    assert share <= 1e-3


@pytest.mark.parametrize("cam,alpha", SCENES)
def test_product_new_camera_matrix_is_the_restatements(cam, alpha):
    """The product's routine and the restatement are two copies of one reading of OpenCV (grid, five iterations, rectangles,
    blend, ROI): equality to 1e-12 catches a slip in one copy, not a shared misreading - parity with cv2 is unpinned.  The
    evidence that the reading is sound are the property tests above: the rectangles land on the viewport, D = 0 gives K and
    the pixel grid, the barrel maps stay inside the source."""
    U = load_pkg("undistort")
    K, D = S.camera(cam, S.MAP_SIZE)
    got, roi = U.get_optimal_new_camera_matrix(K, D, S.MAP_SIZE, alpha)
    want, roi_w = R.get_optimal_new_camera_matrix(K, D, S.MAP_SIZE, alpha)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert tuple(roi) == tuple(roi_w)


@pytest.mark.parametrize("axis,direction", [(0, 1), (0, -1), (1, 1), (1, -1)])
def test_one_float32_step_of_a_map_entry_moves_a_pixel_within_the_neighbour_bound(axis, direction):
    """What tests/test_undistort_gpu.py's end-to-end test asserts where a float map entry differs, driven on purpose: every
    entry of one map is a tie of x 32 ((k + 1/2) / 32, exact in float32), so one float32 step up or down changes the
    fixed-point coordinate of about every other pixel by 1 / 32 - across pixel boundaries and across the source's border too."""
    Ws, Hs = S.HAND_SRC
    kx = np.arange(-70, 32 * Ws + 40, 9)                                 # ties from 2 px left of the source to 1 px right of it
    ky = np.arange(-70, 32 * Hs + 40, 11)
    mapx = np.tile(((kx + 0.5) / 32).astype(np.float32), (len(ky), 1))
    mapy = np.tile(((ky + 0.5) / 32).astype(np.float32)[:, None], (1, len(kx)))
    assert ((kx % 32) == 31).any() and ((ky % 32) == 31).any()           # a step that carries into the next pixel
    img = S.image(S.HAND_SRC, 3, seed=8)
    ixy, al = R.convert_maps(mapx, mapy)
    want = R.remap_linear(img, ixy, al)
    moved = [mapx, mapy]
    moved[axis] = np.nextafter(moved[axis], np.float32(direction * np.inf))
    ixy2, al2 = R.convert_maps(*moved)
    got = R.remap_linear(img, ixy2, al2)
    same = (ixy == ixy2).all(-1) & (al == al2)
    np.testing.assert_array_equal(got[same], want[same])
    changed = list(zip(*np.nonzero(~same)))
    assert len(changed) > mapx.size // 4
    s32 = lambda i, a: i.astype(np.int64)[..., axis] * 32 + ((a >> (5 * axis)) & 31)
    assert (np.abs(s32(ixy2, al2) - s32(ixy, al))[~same] == 1).all()     # exactly 1 / 32 px
    differing = 0
    for y, x in changed:
        d = np.abs(got[y, x].astype(np.int64) - want[y, x])
        differing += int(d.any())
        assert (d <= R.neighbour_bound(img, ixy, y, x)).all(), (y, x, d)
    assert differing > len(changed) // 2                                 # the bound was exercised on pixels that did move
