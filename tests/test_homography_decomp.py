"""`two_view_gate.decompose_homography_mat` (`cv2.decomposeHomographyMat` in numpy) on planted plane-induced homographies
H = K (R + t n^T / d) K^-1 over the motions of tests/relative_pose_scenes.py and three planes.

Measured over those scenes on the build machine (`test_planted_decompositions` prints them on every run):
    the planted (R, t / |t|, +-n) against its nearest candidate     8.9e-14
    R + t n^T against Hn, every candidate                           6.7e-16
    R^T R - I and det R - 1, every candidate                        8.1e-15
The bar is 100 x the largest of these, 8.9e-12 - far below the 1e-9 it may never exceed.
"""
import sys

import numpy as np
import pytest

from conftest import load_pkg
from relative_pose_scenes import K, MOTIONS

BAR = 100 * 8.9e-14
assert BAR <= 1e-9

PLANES = {"frontal": ([0.0, 0.0, 1.0], 9.0), "tilted": ([0.2, -0.3, 1.0], 7.0), "ground": ([0.05, 1.0, 0.15], 1.6)}


@pytest.fixture(scope="module")
def gate():
    return load_pkg("slam.core.two_view_gate")


def _planted(motion, plane):
    R, t = MOTIONS[motion]
    n, d = PLANES[plane]
    n = np.asarray(n, float) / np.linalg.norm(n)
    return R, t, n, d, K @ (R + np.outer(t, n) / d) @ np.linalg.inv(K)


def _hn(H):
    Hn = np.linalg.inv(K) @ H @ K
    return Hn / np.linalg.svd(Hn, compute_uv=False)[1]


def test_planted_decompositions(gate):
    w_planted = w_recon = w_orth = 0.0
    for motion in MOTIONS:
        for plane in PLANES:
            R, t, n, d, H = _planted(motion, plane)
            for scale in (1.0, -2.5):                     # a homography knows no scale, nor its sign
                num, Rs, ts, ns = gate.decompose_homography_mat(scale * H, K)
                assert num == 4 and len(Rs) == len(ts) == len(ns) == 4
                Hn = _hn(H)
                Hn = Hn * np.sign(np.linalg.det(Hn))
                tu = t / np.linalg.norm(t)
                errs = []
                for Rc, tc, nc in zip(Rs, ts, ns):
                    assert Rc.shape == (3, 3) and tc.shape == (3, 1) and nc.shape == (3, 1)
                    w_orth = max(w_orth, np.abs(Rc.T @ Rc - np.eye(3)).max(), abs(np.linalg.det(Rc) - 1))
                    rec = Rc + tc @ nc.T
                    w_recon = max(w_recon, min(np.abs(rec - Hn).max(), np.abs(rec + Hn).max()))
                    tcu = tc.ravel() / np.linalg.norm(tc)
                    e_pos = max(np.abs(tcu - tu).max(), np.abs(nc.ravel() - n).max())
                    e_neg = max(np.abs(tcu + tu).max(), np.abs(nc.ravel() + n).max())
                    errs.append(max(np.abs(Rc - R).max(), min(e_pos, e_neg)))
                    assert abs(np.linalg.norm(nc) - 1) <= BAR
                w_planted = max(w_planted, min(errs))
                # the candidates come in the order (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb)
                assert np.array_equal(Rs[0], Rs[1]) and np.array_equal(ts[0], -ts[1]) and np.array_equal(ns[0], -ns[1])
                assert np.array_equal(Rs[2], Rs[3]) and np.array_equal(ts[2], -ts[3]) and np.array_equal(ns[2], -ns[3])
    print(f"planted against the nearest candidate {w_planted:.3e}, R + t n^T against Hn {w_recon:.3e}, orthonormality {w_orth:.3e} "
          f"(bar {BAR:.1e})")
    assert w_planted <= BAR and w_recon <= BAR and w_orth <= BAR


def test_a_pure_rotation_gives_exactly_one_solution(gate):
    for motion in MOTIONS:
        R = MOTIONS[motion][0]
        num, Rs, ts, ns = gate.decompose_homography_mat(3.0 * K @ R @ np.linalg.inv(K), K)
        assert num == 1 and len(Rs) == len(ts) == len(ns) == 1
        assert np.abs(Rs[0] - R).max() <= BAR and not ts[0].any() and not ns[0].any()


def test_the_gate_module_imports_without_cv2(gate):
    assert "cv2" not in sys.modules or getattr(sys.modules["cv2"], "__file__", None) is None or "cv2_stub" in str(sys.modules["cv2"])
    tvp = load_pkg("slam.core.two_view_pose")
    assert gate.TwoViewPose is tvp.TwoViewPose and gate.TwoViewDecision is tvp.TwoViewDecision and gate.InitParams is tvp.InitParams
    assert gate.compute_model_scores is tvp.compute_model_scores
