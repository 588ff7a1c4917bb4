"""The numpy restatement of the Hamming branch (tests/reproject_hamming_ref.py) against the reference's own outputs
(tests/golden/reproject_hamming.npz, written by tests/golden/make_reproject_hamming_golden.py under a cv2 stub): the
scene generator still produces the inputs the fixture was made from, no accepted decision of a golden scene is tied (so
the fixture does not depend on cKDTree's traversal order) and the restatement equals the reference bit for bit."""
import types

import numpy as np
import pytest

import reproject_hamming_ref as HR
import reproject_hamming_scenes as HS
from conftest import ROOT

G = np.load(ROOT / "tests" / "golden" / "reproject_hamming.npz")


@pytest.mark.parametrize("c", range(len(HS.CASES)))
def test_restatement_equals_reference_outputs(c):
    assert int(G["n_cases"]) == len(HS.CASES)
    sc = HS.make_case(*HS.CASES[c])
    assert sc["digest"] == float(G[f"digest{c}"])
    assert sc["des"].dtype == np.uint8 and sc["des"].shape == (len(sc["kp"]), sc["B"])
    p3, p2, kp, mp, ties, dec = HR.reproject_and_match_hamming(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"],
                                                               sc["H"], sc["radius"], sc["max_hamm"])
    assert ties == 0
    assert len(kp) > 10 and max(d for _, _, d in dec) <= sc["max_hamm"]
    np.testing.assert_array_equal(kp, G[f"kp{c}"])
    np.testing.assert_array_equal(mp, G[f"mp{c}"])
    np.testing.assert_array_equal(p3, G[f"pts3d{c}"])
    np.testing.assert_array_equal(p2, G[f"pts2d{c}"])


def test_tie_rule_and_threshold_of_the_restatement():
    """Two identical keypoint rows at the same distance from a projection: the lower index wins and the tie is counted;
    a distance equal to max_hamm is accepted, one above it is not."""
    K, T = HS.K, np.eye(4)
    X = np.array([0.0, 0.0, 10.0])
    uv = (K @ (X / X[2]))[:2]
    row = np.arange(32, dtype=np.uint8)
    obs = row.copy(); obs[0] ^= 0b111                                    # distance 3 to `row`
    wmap = types.SimpleNamespace(points={7: types.SimpleNamespace(position=X, observations=[(0, 0, obs)])})
    kp = np.float32([uv + [1, 0], uv + [0, 1], uv + [-1, 0]])
    des = np.stack([~row, row, row])
    _, _, kpi, mpi, ties, dec = HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 64)
    assert kpi == [1] and mpi == [7] and ties == 1 and dec == [(7, 1, 3)]
    assert HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 3)[2] == [1]
    assert HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 2)[2] == []
    # a last observation without descriptor skips the point; a row of another width never scores
    wmap.points[7].observations.append((1, 1, None))
    assert HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 64)[2] == []
    wmap.points[7].observations[-1] = (1, 1, np.zeros(1, np.uint8))
    assert HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 64)[2] == [1]
    wmap.points[7].observations = [(1, 1, np.zeros(1, np.uint8))]
    assert HR.reproject_and_match_hamming(wmap, K, T, kp, des, HS.W, HS.H, 5.0, 64)[2] == []
