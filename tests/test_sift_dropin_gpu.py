"""The substitution a maintainer makes in the reference's OpenCV branch for `--detector sift --matcher bf`:
`_get_opencv_detector` returns `sift.SIFT_create(nfeatures=max_features)` and `_get_opencv_matcher`
`bf_matcher.BFMatcher(NORM_L2, crossCheck=True)`.  The overlay's untouched `feature_extractor`, `feature_matcher` and
`filter_matches_ransac` run on those objects and return, on a frame and its integer shift, what the restatements
(tests/sift_ref.py, tests/bf_ref.py) return through the same functions."""
from types import SimpleNamespace

import numpy as np
import pytest

import bf_ref
import sift_ref as R
import sift_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu


class RefDetector:
    """sift_ref behind `detectAndCompute`"""

    def __init__(self, KeyPoint, **kw):
        self.KeyPoint, self.kw = KeyPoint, kw

    def detectAndCompute(self, img, mask=None):
        r = R.detect(img, **self.kw)
        if len(r["xy"]) == 0:
            return [], None
        kps = [self.KeyPoint(x, y, s, a, resp, o, -1) for (x, y), (s, a, resp), o in zip(r["xy"].tolist(), r["aux"].tolist(), r["octave"].tolist())]
        return kps, r["desc"]


class RefMatcher:
    """bf_ref behind `match`"""

    def __init__(self, DMatch):
        self.DMatch = DMatch

    def match(self, q, t):
        ij, dist = bf_ref.match(q, t, bf_ref.NORM_L2, True)
        return [self.DMatch(int(a), int(b), 0, float(d)) for (a, b), d in zip(ij.tolist(), dist.tolist())]


def run(fu, args, detector, matcher, frames):
    kp0, des0 = fu.feature_extractor(args, frames[0], detector)
    kp1, des1 = fu.feature_extractor(args, frames[1], detector)
    matches = fu.feature_matcher(args, kp0, kp1, des0, des1, matcher)
    kept = fu.filter_matches_ransac(kp0, kp1, matches, 1.0)
    return kp0, des0, kp1, des1, matches, kept


def test_the_sift_branch_runs_on_the_substituted_pair_and_equals_the_restatements(gpu_ctx):
    fu, types, T, B = load_pkg("slam.core.features_utils"), load_pkg("slam.core.types"), load_pkg("sift"), load_pkg("bf_matcher")
    args = SimpleNamespace(use_lightglue=False, detector="sift", matcher="bf", max_features=150)
    detector = T.SIFT_create(nfeatures=args.max_features, max_h=120, max_w=160, ctx=gpu_ctx)
    matcher = B.BFMatcher(B.NORM_L2, crossCheck=True, ctx=gpu_ctx)
    frames = S.shifted_pair()
    got = run(fu, args, detector, matcher, frames)
    want = run(fu, args, RefDetector(types.KeyPoint, nfeatures=args.max_features), RefMatcher(types.DMatch), frames)
    for ka, kb in ((got[0], want[0]), (got[2], want[2])):
        fields = lambda ks: [(k.pt, k.size, k.angle, k.response, k.octave, k.class_id) for k in ks]
        assert fields(ka) == fields(kb) and len(ka) >= args.max_features
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[3])
    for ma, mb in ((got[4], want[4]), (got[5], want[5])):
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in ma] == [(m.queryIdx, m.trainIdx, m.distance) for m in mb]
    kp0, des0, kp1, des1, matches, kept = got
    assert des0.dtype == np.float32 and des0.shape == (len(kp0), 128) and len(matches) > 50 and len(kept) > 20
    assert matches == sorted(matches, key=lambda m: m.distance)
    # the KeyPoint fields are the arrays
    xy, aux, octave, desc = detector.detect_arrays(frames[0])
    assert [k.pt for k in kp0] == [tuple(p) for p in xy.tolist()] and [k.octave for k in kp0] == octave.tolist()
    assert [(k.size, k.angle, k.response) for k in kp0] == [tuple(a) for a in aux.tolist()]
    np.testing.assert_array_equal(des0, desc)
    # matched keypoints are displaced by the shift: the close matches are the same structure seen 7 to the left and 4 up
    moved = np.array([np.subtract(kp0[m.queryIdx].pt, kp1[m.trainIdx].pt) for m in kept])
    assert (np.abs(moved - (7, 4)).max(axis=1) < 0.5).mean() > 0.8
    detector.close()


def test_a_blank_frame_gives_the_extractors_empty_pair(gpu_ctx):
    fu, T = load_pkg("slam.core.features_utils"), load_pkg("sift")
    args = SimpleNamespace(use_lightglue=False)
    detector = T.SIFT_create(100, max_h=120, max_w=160, ctx=gpu_ctx)
    assert detector.detectAndCompute(S.constant(100, 120), None) == ([], None)
    assert fu.feature_extractor(args, S.constant(100, 120), detector) == ([], [])
    assert fu.feature_extractor(args, S.constant(1, 1), detector) == ([], [])                # too small for an octave
    detector.close()
