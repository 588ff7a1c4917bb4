"""The reference's default branch (`--detector orb --matcher bf`) on the overlay with cv2 absent: `init_feature_pipeline` hands
out `orb.ORB_create(max_features)` and `bf_matcher.BFMatcher(NORM_HAMMING, crossCheck=True)`, and the untouched
`feature_extractor`, `feature_matcher` and `filter_matches_ransac` return, on a frame and its integer shift, what the
restatements (tests/orb_ref.py, tests/bf_ref.py) return through the same functions."""
from types import SimpleNamespace

import numpy as np
import pytest

import bf_ref
import orb_ref as R
import orb_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu


class RefDetector:
    """orb_ref behind `detectAndCompute`"""

    def __init__(self, KeyPoint, **kw):
        self.KeyPoint, self.kw = KeyPoint, kw

    def detectAndCompute(self, img, mask=None):
        r = R.detect(img, **self.kw)
        if len(r["xy"]) == 0:
            return [], None
        kps = [self.KeyPoint(x, y, s, a, resp, int(o), -1) for (x, y), (s, a, resp, o) in zip(r["xy"].tolist(), r["aux"].tolist())]
        return kps, r["desc"]


class RefMatcher:
    """bf_ref behind `match`"""

    def __init__(self, DMatch):
        self.DMatch = DMatch

    def match(self, q, t):
        ij, dist = bf_ref.match(q, t, bf_ref.NORM_HAMMING, True)
        return [self.DMatch(int(a), int(b), 0, float(d)) for (a, b), d in zip(ij.tolist(), dist.tolist())]


def run(fu, args, detector, matcher, frames):
    kp0, des0 = fu.feature_extractor(args, frames[0], detector)
    kp1, des1 = fu.feature_extractor(args, frames[1], detector)
    matches = fu.feature_matcher(args, kp0, kp1, des0, des1, matcher)
    kept = fu.filter_matches_ransac(kp0, kp1, matches, 1.0)
    return kp0, des0, kp1, des1, matches, kept


def same(a, b):
    kp_a0, des_a0, kp_a1, des_a1, m_a, k_a = a
    kp_b0, des_b0, kp_b1, des_b1, m_b, k_b = b
    for ka, kb in ((kp_a0, kp_b0), (kp_a1, kp_b1)):
        assert [(k.pt, k.size, k.angle, k.response, k.octave) for k in ka] == [(k.pt, k.size, k.angle, k.response, k.octave) for k in kb]
    np.testing.assert_array_equal(des_a0, des_b0)
    np.testing.assert_array_equal(des_a1, des_b1)
    for ma, mb in ((m_a, m_b), (k_a, k_b)):
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in ma] == [(m.queryIdx, m.trainIdx, m.distance) for m in mb]


def test_the_default_branch_runs_without_cv2_and_equals_the_restatements(gpu_ctx):
    fu, types, O, B = load_pkg("slam.core.features_utils"), load_pkg("slam.core.types"), load_pkg("orb"), load_pkg("bf_matcher")
    assert not types.HAVE_CV2
    args = SimpleNamespace(use_lightglue=False, detector="orb", matcher="bf", max_features=6000)
    detector, matcher = fu.init_feature_pipeline(args)
    assert isinstance(detector, O.ORB) and isinstance(matcher, B.BFMatcher)
    assert (detector.nfeatures, detector.nlevels, detector.scoreType, matcher.normType, matcher.crossCheck) == (6000, 8, 0, 6, True)
    frames = S.shifted_pair()
    got = run(fu, args, detector, matcher, frames)
    want = run(fu, args, RefDetector(types.KeyPoint, nfeatures=6000), RefMatcher(types.DMatch), frames)
    same(got, want)
    assert len(got[0]) > 100 and len(got[4]) > 50
    assert got[4] == sorted(got[4], key=lambda m: m.distance)
    detector.close()


def test_one_level_with_no_cut_binding_follows_an_integer_shift(gpu_ctx):
    fu, types, O, B = load_pkg("slam.core.features_utils"), load_pkg("slam.core.types"), load_pkg("orb"), load_pkg("bf_matcher")
    args = SimpleNamespace(use_lightglue=False, detector="orb", matcher="bf")
    kw = dict(nfeatures=6000, nlevels=1)
    detector = O.ORB_create(6000, nlevels=1, max_h=120, max_w=160, ctx=gpu_ctx)
    matcher = B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=gpu_ctx)
    frames = S.shifted_pair()
    got = run(fu, args, detector, matcher, frames)
    want = run(fu, args, RefDetector(types.KeyPoint, **kw), RefMatcher(types.DMatch), frames)
    same(got, want)
    kp0, _, kp1, _, matches, kept = got
    moved = [np.subtract(kp0[m.queryIdx].pt, kp1[m.trainIdx].pt).tolist() for m in matches if m.distance == 0]
    assert len(moved) > 20 and all(d == [7.0, 4.0] for d in moved)           # identical descriptors: the same corner, shifted
    detector.close()


def test_a_blank_frame_gives_the_extractors_empty_pair(gpu_ctx):
    fu, O = load_pkg("slam.core.features_utils"), load_pkg("orb")
    args = SimpleNamespace(use_lightglue=False)
    detector = O.ORB_create(100, max_h=120, max_w=160, ctx=gpu_ctx)
    assert fu.feature_extractor(args, S.constant(100, 120), detector) == ([], [])
    detector.close()
