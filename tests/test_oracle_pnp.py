"""The numpy restatement of OpenCV's solvePnPRansac(SOLVEPNP_ITERATIVE) (oracle/pnp_ref.py) against ground truth:
the yardstick of the GPU tests has to be right first."""
import numpy as np
import pytest

import pnp_scenes as S
from oracle import pnp_ref as O


def _pose(r, t):
    return O.pose_matrix(r, t)


@pytest.mark.parametrize("seed,n,cam", [(11, 40, "kitti"), (12, 200, "rand"), (13, 60, "rand")])
def test_noise_free_recovers_ground_truth(seed, n, cam):
    """No noise, no outliers: the ground-truth pose up to the float32 rounding of the inputs (1e-7 px / 1e-7 m, which
    bounds what any solver can recover - a 1e-9 bar would measure the rounding, not the solver)."""
    sc = S.make_scene(seed, n, 0.0, cam, noise_px=0.0)
    ok, r, t, mask, info = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, False, S.ITERS, S.CONF)
    assert ok and mask.all() and info["inliers"] == n
    T = _pose(r, t)
    assert S.rot_err_rad(T[:3, :3], sc["Tcw"][:3, :3]) < 1e-6
    assert np.linalg.norm(T[:3, 3] - sc["Tcw"][:3, 3]) < 1e-6 * (1 + np.linalg.norm(sc["Tcw"][:3, 3]))


@pytest.mark.parametrize("seed,n,frac,cam", [(21, 100, 0.0, "kitti"), (22, 100, 0.3, "rand"), (23, 600, 0.3, "kitti"),
                                             (24, 150, 0.5, "rand")])
def test_noisy_meets_reference_bar_and_keeps_true_inliers(seed, n, frac, cam):
    """0.5 px noise and outliers, no guess: the reference test's bar (rotation < 2 deg, |dt| < 0.1) and >= 95 % of the
    true inliers in the mask."""
    sc = S.make_scene(seed, n, frac, cam)
    ok, r, t, mask, info = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, False, S.ITERS, S.CONF)
    assert ok
    T = _pose(r, t)
    assert S.rot_err_deg(T[:3, :3], sc["Tcw"][:3, :3]) < 2.0
    assert np.linalg.norm(T[:3, 3] - sc["Tcw"][:3, 3]) < 0.1
    assert (mask & sc["inlier"]).sum() >= 0.95 * sc["inlier"].sum()
    assert info["inliers"] == mask.sum() and 0 <= info["sample"] < info["samples"] <= S.ITERS


def test_guess_starts_the_refinement_at_the_last_sample():
    """With a guess the LM starts from the last evaluated sample (OpenCV's shared rvec / tvec), so the result may
    differ from the no-guess one while the mask, sample count and winner do not."""
    sc = S.make_scene(22, 100, 0.3, "rand")
    a = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, False, S.ITERS, S.CONF)
    b = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, True, S.ITERS, S.CONF)
    assert a[0] and b[0]
    np.testing.assert_array_equal(a[3], b[3])
    assert (a[4]["samples"], a[4]["sample"], a[4]["inliers"]) == (b[4]["samples"], b[4]["sample"], b[4]["inliers"])
    # the LM of b started where the loop's last sample left rvec / tvec: the same start gives the same result
    p3, p2 = sc["pts3d"], sc["pts2d"]
    rng = O.CvRNG()
    for _ in range(b[4]["samples"]):
        idx = []
        for _ in range(5):
            v = rng.uniform(0, len(p3))
            while v in idx:
                v = rng.uniform(0, len(p3))
            idx.append(v)
    last = O.epnp_model(p3[idx], p2[idx], sc["K"])
    r, t, _ = O.refine_lm(p3[b[3]].astype(np.float64), p2[b[3]].astype(np.float64), last[0], last[1], sc["K"])
    np.testing.assert_array_equal(r, b[1])
    np.testing.assert_array_equal(t, b[2])


def test_five_points_one_epnp_all_inliers():
    sc = S.make_scene(31, 5, 0.0, "rand")
    ok, r, t, mask, info = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, True, S.ITERS, S.CONF)
    assert ok and mask.all() and info == {"inliers": 5, "samples": 0, "sample": -1, "lm_iters": 0}
    R, tt = O.epnp(sc["pts3d"], sc["pts2d"], sc["K"])
    np.testing.assert_array_equal(r, O.rodrigues_R2r(R))
    np.testing.assert_array_equal(t, tt)
    T = _pose(r, t)
    assert S.rot_err_deg(T[:3, :3], sc["Tcw"][:3, :3]) < 2.0


def test_failure_branches():
    K = S.K_RAND
    for n in range(4):
        ok, r, t, mask, info = O.solve_pnp_ransac(np.zeros((n, 3)), np.zeros((n, 2)), K)
        assert not ok and mask.shape == (n,) and info["inliers"] == -1
    with pytest.raises(NotImplementedError):
        O.solve_pnp_ransac(np.ones((4, 3)), np.ones((4, 2)), K)
    # every point identical: no model gathers five inliers
    ok, r, t, mask, info = O.solve_pnp_ransac(np.tile([[0.5, -0.2, 4.0]], (40, 1)), np.tile([[310.0, 190.0]], (40, 1)), K,
                                               S.RANSAC_PX, False, 50, S.CONF)
    assert not ok and not mask.any() and info["inliers"] == -1 and info["samples"] == 50
    # all outliers: pixels unrelated to the points
    rng = np.random.default_rng(5)
    sc = S.make_scene(41, 60, 0.0, "rand")
    p2 = np.stack([rng.uniform(0, 640, 60), rng.uniform(0, 480, 60)], 1).astype(np.float32)
    ok, r, t, mask, info = O.solve_pnp_ransac(sc["pts3d"], p2, K, 0.01, False, 40, S.CONF)
    assert not ok and not mask.any() and info["samples"] == 40
