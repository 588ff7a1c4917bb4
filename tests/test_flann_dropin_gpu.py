"""The substitution a maintainer makes in the reference's OpenCV branch for `--detector sift --matcher flann`:
`_get_opencv_detector` returns `sift.SIFT_create(nfeatures=max_features)` and `_get_opencv_matcher`
`flann_matcher.FlannBasedMatcher(index_params, search_params)`.  The overlay's untouched `feature_extractor`, `feature_matcher`
and `filter_matches_ransac` run on those objects; the stand-in's search is exact, so its `match` is the brute-force matcher's
without cross-check, its `knnMatch(k=2)` under the Python ratio idiom is `ratio_match`, and with an LSH index it matches ORB
rows by Hamming distance."""
from types import SimpleNamespace

import numpy as np
import pytest

import sift_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu


def _fields(ms):
    return [(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in ms]


def test_the_sift_flann_branch_runs_on_the_substituted_pair(gpu_ctx):
    fu, T, B, F = load_pkg("slam.core.features_utils"), load_pkg("sift"), load_pkg("bf_matcher"), load_pkg("flann_matcher")
    args = SimpleNamespace(use_lightglue=False, detector="sift", matcher="flann", max_features=150)
    detector = T.SIFT_create(nfeatures=args.max_features, max_h=120, max_w=160, ctx=gpu_ctx)
    matcher = F.FlannBasedMatcher(dict(algorithm=F.FLANN_INDEX_KDTREE, trees=5), dict(checks=50), ctx=gpu_ctx)     # the reference's parameters
    frames = S.shifted_pair()
    kp0, des0 = fu.feature_extractor(args, frames[0], detector)
    kp1, des1 = fu.feature_extractor(args, frames[1], detector)
    matches = fu.feature_matcher(args, kp0, kp1, des0, des1, matcher)
    kept = fu.filter_matches_ransac(kp0, kp1, matches, 1.0)
    detector.close()
    assert des0.dtype == np.float32 and des0.shape == (len(kp0), 128) and len(kp0) >= args.max_features
    # `match`: the exact nearest neighbour of every query row, sorted by distance by feature_matcher
    bf = B.BFMatcher(B.NORM_L2, crossCheck=False, ctx=gpu_ctx)
    assert len(matches) == len(kp0) and matches == sorted(matches, key=lambda m: m.distance)
    assert _fields(sorted(matches, key=lambda m: m.queryIdx)) == _fields(bf.match(des0, des1)) == _fields(matcher.match(des0, des1))
    assert len(kept) > 20
    moved = np.array([np.subtract(kp0[m.queryIdx].pt, kp1[m.trainIdx].pt) for m in kept])
    assert (np.abs(moved - (7, 4)).max(axis=1) < 0.5).mean() > 0.8            # the shift of the pair
    # knnMatch + the Python ratio idiom == ratio_match, and both follow the shift
    pairs = matcher.knnMatch(des0, des1, k=2)
    assert len(pairs) == len(kp0) and all(len(p) == 2 and p[0].distance <= p[1].distance for p in pairs)
    assert _fields([p[0] for p in pairs]) == _fields(bf.match(des0, des1))
    for ratio in (0.6, 0.75):
        good = [m for m, n in pairs if m.distance < ratio * n.distance]
        assert _fields(good) == _fields(matcher.ratio_match(des0, des1, ratio)) == _fields(bf.ratio_match(des0, des1, ratio))
        assert 10 < len(good) < len(kp0)
    moved = np.array([np.subtract(kp0[m.queryIdx].pt, kp1[m.trainIdx].pt) for m in good])
    assert (np.abs(moved - (7, 4)).max(axis=1) < 0.5).mean() > 0.8


def test_an_lsh_index_matches_orb_rows_by_hamming_distance(gpu_ctx):
    O, B, F = load_pkg("orb"), load_pkg("bf_matcher"), load_pkg("flann_matcher")
    detector = O.ORB_create(300, max_h=120, max_w=160, ctx=gpu_ctx)
    frames = S.shifted_pair()
    (_kp0, des0), (_kp1, des1) = detector.detectAndCompute(frames[0], None), detector.detectAndCompute(frames[1], None)
    detector.close()
    assert des0.dtype == np.uint8 and des0.shape[1] == 32 and len(des0) > 50 and len(des1) > 50
    lsh = F.FlannBasedMatcher(dict(algorithm=F.FLANN_INDEX_LSH, table_number=6, key_size=12, multi_probe_level=1), {}, ctx=gpu_ctx)
    bf = B.BFMatcher(B.NORM_HAMMING, crossCheck=False, ctx=gpu_ctx)
    assert _fields(lsh.match(des0, des1)) == _fields(bf.match(des0, des1)) and len(lsh.match(des0, des1)) == len(des0)
    assert [_fields(p) for p in lsh.knnMatch(des0, des1, 3)] == [_fields(p) for p in bf.knnMatch(des0, des1, 3)]
    assert _fields(lsh.ratio_match(des0, des1, 0.8)) == _fields(bf.ratio_match(des0, des1, 0.8))
    with pytest.raises(TypeError, match="KD-tree index refuses uint8"):
        F.FlannBasedMatcher(dict(algorithm=F.FLANN_INDEX_KDTREE, trees=5), dict(checks=50)).match(des0, des1)
