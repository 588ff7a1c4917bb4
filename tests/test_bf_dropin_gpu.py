"""`bf_matcher.BFMatcher` in the place of `cv2.BFMatcher(norm, crossCheck=True)` on the overlay's OpenCV branch: the untouched
`feature_matcher` (slam/core/features_utils.py:173-178 of the reference: `matcher.match(des0, des1)`, sorted by `.distance`)
returns the restatement's matches in that order - python's sort is stable, so equal distances stay in query order."""
from types import SimpleNamespace

import numpy as np
import pytest

import bf_cases
from conftest import load_pkg

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in bf_cases.exact_cases()}


@pytest.mark.parametrize("name", ["ham_planted_300x280_d32", "ham_257x191_d1", "l2int_257x191_d128", "l2int_63x65_d3"])
def test_feature_matcher_returns_the_restatements_matches_sorted_by_distance(gpu_ctx, name):
    fu = load_pkg("slam.core.features_utils")
    types = load_pkg("slam.core.types")
    B = load_pkg("bf_matcher")
    c = CASES[name]
    args = SimpleNamespace(use_lightglue=False, detector="orb", matcher="bf")
    kp0 = [types.KeyPoint(float(i), 1.0, 1.0) for i in range(len(c["q"]))]
    kp1 = [types.KeyPoint(float(i), 2.0, 1.0) for i in range(len(c["t"]))]
    got = fu.feature_matcher(args, kp0, kp1, c["q"], c["t"], B.BFMatcher(c["norm"], crossCheck=True, ctx=gpu_ctx))
    ij, dist = bf_cases.expected(c, True)
    order = np.argsort(dist, kind="stable")
    assert len(got) == len(ij) > 0
    assert all(isinstance(m, types.DMatch) for m in got)
    assert [(m.queryIdx, m.trainIdx) for m in got] == [tuple(p) for p in ij[order].tolist()]
    assert [m.distance for m in got] == dist[order].astype(np.float64).tolist()
    assert all(m.imgIdx == 0 for m in got)
    ties = np.nonzero(np.diff(dist[order]) == 0)[0]
    assert len(ties) > 0 or not name.startswith("ham")                      # (Hamming: a handful of values, ties are certain)
    assert (np.diff(ij[order][:, 0])[ties] > 0).all()                       # equal distances: ascending queryIdx


def test_empty_descriptors_give_no_matches(gpu_ctx):
    fu = load_pkg("slam.core.features_utils")
    B = load_pkg("bf_matcher")
    args = SimpleNamespace(use_lightglue=False)
    des = np.zeros((3, 32), np.uint8)
    assert fu.feature_matcher(args, [], [1, 2, 3], [], des, B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=gpu_ctx)) == []
