"""The prototype's stereo chain on the device (refrences/sfm_lightglue_aliked.py:357-396): compute_stereo_disparity on a
planted-plane pair, calculate_right_features, get_stereo_3d_pts with KITTI's Proj / Proj_r.

Depth: the pair is rectified, so the DLT system has an exact null vector and Z = f B / d.  The keypoints lie on quarter pixels and
d on sixteenths, so x - d is exact in float32 and f B / d is the value to meet.  The tolerance is the one
tests/test_triangulate_gpu.py holds sslam_triangulate_2view to, 100 x its measured Jacobi-against-LAPACK floor: 3.4e-11 relative."""
import numpy as np
import pytest

import stereo_ref as R
import stereo_scenes as SC
from conftest import load_pkg

pytestmark = pytest.mark.gpu

X_BAR = 100 * 3.4e-13
F, CX, CY, FB = 718.856, 607.1928, 185.2157, 386.1448
PROJ = np.array([[F, 0, CX, 0], [0, F, CY, 0], [0, 0, 1, 0]], np.float64)
PROJ_R = np.array([[F, 0, CX, -FB], [0, F, CY, 0], [0, 0, 1, 0]], np.float64)
W, H, D, D0 = 200, 40, 32, 12


@pytest.fixture(scope="module")
def stereo(gpu_ctx):
    return load_pkg("stereo")


@pytest.fixture(scope="module")
def scene(stereo, gpu_ctx):
    sg = stereo.StereoSGBM_create(**SC.planted_params(D, 11), ctx=gpu_ctx)
    pairs = [SC.planted_pair(W, H, D, D0, seed=s, channels=3) for s in (40, 41)]
    disp = [stereo.compute_stereo_disparity(l, r, sg) for l, r in pairs]
    rng = np.random.default_rng(42)
    q = [np.column_stack([rng.integers(0, 4 * W, 300), rng.integers(0, 4 * H, 300)]).astype(np.float32) / np.float32(4) for _ in range(2)]
    return dict(sg=sg, disp=disp, q=q, pairs=pairs)


def _prototype_check(q, disp, min_disp, max_disp):
    q_idx = q.astype(int)
    vals = disp.T[q_idx[:, 0], q_idx[:, 1]]
    return vals, (vals > min_disp) & (vals < max_disp)


def test_disparity_is_the_planted_plane(scene):
    for (l, r), disp in zip(scene["pairs"], scene["disp"]):
        assert disp.dtype == np.float32 and disp.shape == (H, W)
        assert (disp[:, :D] == -1).all() and np.abs(disp[:, D:] - D0).max() <= 0.5
        want = R.compute(R.bgr_to_grey(l), R.bgr_to_grey(r), R.Params(**SC.planted_params(D, 11)))
        assert np.array_equal(disp, want.astype(np.float32) / np.float32(16))


def test_right_features_equal_the_prototypes_numpy_expressions(stereo, scene, gpu_ctx):
    q1, q2 = scene["q"]
    d1, d2 = scene["disp"]
    v1, m1 = _prototype_check(q1, d1, 0.0, 100.0)
    v2, m2 = _prototype_check(q2, d2, 0.0, 100.0)
    a_vals, a_mask = stereo.apply_disparity_check(q1, d1, 0.0, 100.0)
    assert np.array_equal(a_vals, v1) and np.array_equal(a_mask, m1)
    in_bounds = m1 & m2
    assert 50 < in_bounds.sum() < 300                                    # keypoints in the uncomputed columns are masked out
    want_1r, want_2r = q1[in_bounds].copy(), q2[in_bounds].copy()
    want_1r[:, 0] -= v1[in_bounds]
    want_2r[:, 0] -= v2[in_bounds]
    q1_l, q1_r, q2_l, q2_r, got = stereo.calculate_right_features(q1, q2, d1, d2, ctx=gpu_ctx)
    assert np.array_equal(got, in_bounds)
    assert np.array_equal(q1_l, q1[in_bounds]) and np.array_equal(q2_l, q2[in_bounds])
    assert np.array_equal(q1_r, want_1r) and np.array_equal(q2_r, want_2r)
    # a narrower window, as the prototype's min_disp / max_disp arguments give
    lo = stereo.calculate_right_features(q1, q2, d1, d2, min_disp=12.0, max_disp=100.0, ctx=gpu_ctx)[4]
    assert np.array_equal(lo, _prototype_check(q1, d1, 12.0, 100.0)[1] & _prototype_check(q2, d2, 12.0, 100.0)[1])


def test_lifted_depth_is_f_b_over_d(stereo, scene, gpu_ctx):
    q1, q2 = scene["q"]
    d1, d2 = scene["disp"]
    q1_l, q1_r, q2_l, q2_r, _ = stereo.calculate_right_features(q1, q2, d1, d2, ctx=gpu_ctx)
    Q1, Q2 = stereo.get_stereo_3d_pts(q1_l, q1_r, q2_l, q2_r, PROJ, PROJ_R, ctx=gpu_ctx)
    worst = 0.0
    for ql, qr, Q in ((q1_l, q1_r, Q1), (q2_l, q2_r, Q2)):
        assert Q.shape == (len(ql), 3) and Q.dtype == np.float64 and np.isfinite(Q).all()
        ql64 = ql.astype(np.float64)                                     # (float32 - Python float stays float32: the expectation is float64)
        d = ql64[:, 0] - qr[:, 0].astype(np.float64)
        Z = FB / d
        want = np.column_stack([(ql64[:, 0] - CX) * Z / F, (ql64[:, 1] - CY) * Z / F, Z])
        err = np.abs(Q - want).max(1) / np.linalg.norm(want, axis=1)
        worst = max(worst, err.max())
    print("worst relative error against f B / d:", worst)
    assert worst <= X_BAR
    # the one-call form: lookup, mask, right pixel and point together, against the restatement with LAPACK's SVD
    disp16 = np.rint(d1 * 16).astype(np.int16)
    q = np.concatenate([q1, np.float32([[-3.0, 5.0], [W, 3.0], [10.0, H + 0.25], [np.nan, 2.0], [-0.5, -0.75]])])
    d, mask, xr, X = stereo.lift(q, disp16, PROJ, PROJ_R, 0.0, 100.0, ctx=gpu_ctx)
    rd, rmask, rxr, rX = R.lift(q, disp16, PROJ, PROJ_R, 0.0, 100.0)
    assert np.array_equal(mask, rmask) and not mask[-5:-1].any()         # outside the image: unmasked, not an error
    assert np.array_equal(d, rd, equal_nan=True) and np.array_equal(xr, rxr, equal_nan=True)
    assert np.isnan(X[~mask]).all()
    assert (np.abs(X[mask] - rX[mask]).max(1) <= X_BAR * np.linalg.norm(rX[mask], axis=1)).all()


def test_device_form_with_a_device_count_writes_nothing_beyond_it(stereo, scene, gpu_ctx):
    q = scene["q"][0][:12]
    disp16 = np.rint(scene["disp"][0] * 16).astype(np.int16)
    n_max, n = 12, 5
    sent_f, sent_d, sent_m = np.float32(-777.0), -777.0, np.uint8(99)
    bufs = [gpu_ctx.upload(q), gpu_ctx.upload(disp16), gpu_ctx.upload(np.int32([n])), gpu_ctx.upload(np.full(n_max, sent_f)),
            gpu_ctx.upload(np.full((n_max, 2), sent_f)), gpu_ctx.upload(np.full((n_max, 3), sent_d)), gpu_ctx.upload(np.full(n_max, sent_m))]
    try:
        stereo.lift_dev(gpu_ctx, n_max, bufs[2], bufs[0], bufs[1], H, W, PROJ, PROJ_R, 0.0, 100.0, bufs[3], bufs[4], bufs[5], bufs[6])
        gpu_ctx.sync()
        d, xr, X, mask = np.empty(n_max, np.float32), np.empty((n_max, 2), np.float32), np.empty((n_max, 3)), np.empty(n_max, np.uint8)
        for arr, ptr in ((d, bufs[3]), (xr, bufs[4]), (X, bufs[5]), (mask, bufs[6])):
            gpu_ctx.d2h(arr, ptr)
    finally:
        for ptr in bufs:
            gpu_ctx.free(ptr)
    assert (d[n:] == sent_f).all() and (xr[n:] == sent_f).all() and (X[n:] == sent_d).all() and (mask[n:] == sent_m).all()
    hd, hmask, hxr, hX = stereo.lift(q[:n], disp16, PROJ, PROJ_R, 0.0, 100.0, ctx=gpu_ctx)
    assert np.array_equal(mask[:n].astype(bool), hmask) and np.array_equal(d[:n], hd, equal_nan=True)
    assert np.array_equal(xr[:n], hxr, equal_nan=True) and np.array_equal(X[:n], hX, equal_nan=True)
