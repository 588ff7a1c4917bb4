"""The numpy restatement of homography RANSAC (tests/homography_ref.py) on the CPU: planted plane-induced homographies are
recovered, the orientation test throws a mirrored quadruple away, the four-match path, and a set on one line has no model.
Both variants of the small dense solvers (LAPACK, and the float64 ports of what the kernel runs) are held to the same."""
import numpy as np
import pytest

import homography_ref as HR
import homography_scenes as S
from relative_pose_scenes import MOTIONS


def _grid(n, seed):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(20, S.W - 20, n), rng.uniform(20, S.Hh - 20, n)]).astype(np.float32)


@pytest.mark.parametrize("linalg", ["lapack", "jacobi"])
@pytest.mark.parametrize("motion", list(MOTIONS))
def test_a_planted_plane_homography_is_recovered(motion, linalg):
    """H = K (R + t n^T / d) K^-1 over the motions of the relative-pose scenes, noise-free pixels rounded to float32 (half an
    ulp of 1240 is 6e-5 pixel): every match is an inlier and H comes back to 1e-5 of max |H| - the rounding over a
    lever of a few hundred pixels, far above either solver's own error."""
    R, t = MOTIONS[motion]
    nrm = np.array([0.1, 0.2, -1.0]) / np.linalg.norm([0.1, 0.2, -1.0])
    Ht = S.plane_homography(R, t, nrm, -8.0)
    p1 = _grid(200, 7)
    p2 = S.apply_h(Ht, p1.astype(np.float64)).astype(np.float32)
    H, mask, info = HR.find_homography_ransac(p1, p2, 1.5, linalg=linalg)
    assert mask.all() and info["inliers"] == 200 and info["sample"] == 0
    assert np.abs(H - Ht).max() <= 1e-5 * np.abs(Ht).max()
    # the DLT alone, and the polish from a perturbed start
    assert np.abs(HR.run_kernel(p1, p2, linalg) - Ht).max() <= 1e-5 * np.abs(Ht).max()
    Hp, its = HR.lm_polish(Ht * (1 + 1e-3 * np.arange(9).reshape(3, 3) / 9) / (1 + 1e-3 * 8 / 9), p1, p2, linalg)
    assert 1 <= its <= 10 and np.abs(Hp - Ht).max() <= 1e-5 * np.abs(Ht).max()


def test_the_orientation_test_rejects_a_mirrored_quadruple():
    src = np.float32([[100, 100], [300, 100], [300, 250], [100, 250]])
    same = src + np.float32([5, -3])
    mirrored = src.copy(); mirrored[:, 0] = 1240 - mirrored[:, 0]            # a reflection: every triple flips
    twisted = same.copy(); twisted[[2, 3]] = twisted[[3, 2]]                # two corners exchanged: some triples flip
    idx = [0, 1, 2, 3]
    assert HR.orientation_negatives(src, same) == 0 and HR.check_subset(src, same, idx)
    assert HR.orientation_negatives(src, mirrored) == 4 and HR.check_subset(src, mirrored, idx)      # 0 or 4 pass
    assert HR.orientation_negatives(src, twisted) in (1, 2, 3) and not HR.check_subset(src, twisted, idx)
    collinear = src.copy(); collinear[3] = (src[0] + src[1]) / 2
    assert not HR.check_subset(collinear, same, idx)


@pytest.mark.parametrize("linalg", ["lapack", "jacobi"])
def test_four_matches_take_one_dlt_and_no_refinement(linalg):
    p1 = _grid(4, 11)
    p2 = S.apply_h(S.PLANTED, p1.astype(np.float64)).astype(np.float32)
    H, mask, info = HR.find_homography_ransac(p1, p2, 1.5, linalg=linalg)
    assert mask.tolist() == [True] * 4 and info["iterations"] == 0 and info["lm_iterations"] == 0
    assert np.array_equal(H, HR.run_kernel(p1, p2, linalg))
    assert np.abs(S.apply_h(H, p1.astype(np.float64)) - p2).max() < 1e-6
    # runKernel returns no model: no spread along x
    p1[:, 0] = 50
    assert HR.find_homography_ransac(p1, p2, 1.5, linalg=linalg)[:2] == (None, None)


def test_points_on_one_line_have_no_model():
    s = S.all_scenes()["line_50"]
    S.assert_reaches(s)
    assert s["ref"][0] is None and s["ref_jacobi"][0] is None


def test_the_ports_solve_what_lapack_solves():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(20, 9))
    A = B.T @ B
    v = HR.jacobi_eig_smallest(A)
    w, V = np.linalg.eigh(A)
    assert min(np.abs(v - V[:, 0]).max(), np.abs(v + V[:, 0]).max()) < 1e-12
    C = A[:8, :8] + np.eye(8)
    b = rng.normal(size=8)
    assert np.abs(HR.gauss_solve(C, b) - np.linalg.solve(C, b)).max() < 1e-12
    assert np.abs(HR.gauss_inverse_diag(C) - np.diag(np.linalg.inv(C))).max() < 1e-12
    assert HR.gauss_solve(np.zeros((8, 8)), b) is None


def test_bad_arguments():
    p = _grid(10, 1)
    with pytest.raises(ValueError):
        HR.find_homography_ransac(p, p[:-1])
    with pytest.raises(ValueError):
        HR.find_homography_ransac(p[:3], p[:3])
    with pytest.raises(ValueError):
        HR.find_homography_ransac(np.zeros((16385, 2)), np.zeros((16385, 2)))
