"""The ORB restatement (tests/orb_ref.py) against the definitions it restates and against the properties ORB has by
construction: FAST against a brute-force loop of the definition, strict NMS, the default pattern against cv::RNG, the quotas,
rotation and shift covariance, ties at both cuts."""
import numpy as np

import orb_ref as R
import orb_scenes as S
from oracle.ransac_ref import CvRNG


def brute_fast(patch, t):
    """the definition at the centre (3, 3) of a 7 x 7 patch: is it a corner at threshold th (9 contiguous circle pixels all
    brighter than v + th or all darker than v - th), and the largest th >= t at which it still is (0: no corner at t)"""
    v = int(patch[3, 3])
    c = [int(patch[3 + dy, 3 + dx]) for dx, dy in R.CIRCLE]

    def corner(th):
        for k in range(16):
            arc = [c[(k + j) % 16] for j in range(9)]
            if all(p > v + th for p in arc) or all(p < v - th for p in arc):
                return True
        return False
    if not corner(t):
        return 0
    th = t
    while corner(th + 1):
        th += 1
    return th


def test_fast_score_is_the_largest_threshold_of_the_definition():
    rng = np.random.default_rng(0)
    n_corner = 0
    for trial in range(60):
        img = rng.integers(0, 256, (16, 16)).astype(np.uint8)
        if trial % 3 == 0:                                   # a bright or dark blob so that corners exist
            img[5:11, 5:11] = np.clip(img[5:11, 5:11].astype(int) // 4 + (180 if trial % 2 else 0), 0, 255)
        t = int(rng.integers(1, 60))
        score = R.fast_score_map(img, t)
        assert (score[:3] == 0).all() and (score[-3:] == 0).all() and (score[:, :3] == 0).all() and (score[:, -3:] == 0).all()
        for y in range(3, 13):
            for x in range(3, 13):
                want = brute_fast(img[y - 3:y + 4, x - 3:x + 4], t)
                assert score[y, x] == want, (trial, x, y)
                n_corner += want > 0
    assert n_corner > 50


def test_fast_scores_at_exactly_t_and_t_plus_one():
    t = 20
    for delta, want in ((t, 0), (t + 1, t), (t + 2, t + 1)):
        img = np.full((7, 7), 100, np.uint8)
        for dx, dy in R.CIRCLE[:9]:
            img[3 + dy, 3 + dx] = 100 + delta                # exactly 9 contiguous brighter pixels
        assert R.fast_score_map(img, t)[3, 3] == want == brute_fast(img, t)
        img = np.full((7, 7), 100, np.uint8)
        for dx, dy in R.CIRCLE[10:] + R.CIRCLE[:3]:
            img[3 + dy, 3 + dx] = 100 - delta                # ... darker, across the wrap of the circle
        assert R.fast_score_map(img, t)[3, 3] == want == brute_fast(img, t)
    img = np.full((7, 7), 100, np.uint8)
    for dx, dy in R.CIRCLE[:8]:
        img[3 + dy, 3 + dx] = 200                            # 8 are not enough
    assert R.fast_score_map(img, t)[3, 3] == 0


def test_strict_nms_keeps_none_of_two_equal_neighbours():
    s = np.zeros((9, 9), np.int64)
    s[4, 4] = s[4, 5] = 30                                   # a plateau of two
    s[1, 1] = 25
    s[7, 7], s[6, 6] = 40, 41                                # a diagonal pair: the larger one stays
    keep = R.nms(s)
    assert not keep[4, 4] and not keep[4, 5]
    assert keep[1, 1] and keep[6, 6] and not keep[7, 7]
    assert keep.sum() == 2


def test_default_pattern_is_cv_rng_0x34985739():
    rng = CvRNG(0x34985739)
    want = [(rng.uniform(-15, 16), rng.uniform(-15, 16)) for _ in range(512)]
    p = R.default_pattern()
    assert p.dtype == np.int8 and p.shape == (512, 2)
    assert [tuple(r) for r in p.tolist()] == want
    assert p.min() == -15 and p.max() == 15
    assert p[:4].tolist() == [[13, -15], [3, 4], [10, 6], [-5, -6]]          # (recorded from this restatement)


def test_quotas_sum_to_nfeatures():
    q = R.quotas(500, 1.2, 8)
    assert sum(q) == 500 and q == sorted(q, reverse=True) and len(q) == 8
    assert R.quotas(500, 1.2, 1) == [500]
    assert R.quotas(6000, 1.2, 1) == [6000]
    assert sum(R.quotas(6000, 1.2, 8)) == 6000
    assert min(R.quotas(3, 2.0, 16)) == 0                                   # the remainder is floored at 0


def test_tables():
    assert R.umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert R.gauss_taps().tolist() == [18, 34, 49, 54, 49, 34, 18]
    assert R.border(31) == 32 and R.border(3) == 23 and R.border(50) == 51
    assert R.level_sizes(1241, 376, 1.2, 3) == [(1241, 376), (1034, 313), (862, 261)]


def test_fast_atan2_is_within_its_stated_accuracy():
    rng = np.random.default_rng(1)
    for y, x in rng.integers(-3000, 3000, (400, 2)).tolist() + [[0, 5], [5, 0], [0, -5], [-5, 0], [7, 7], [-7, 7]]:
        want = np.degrees(np.arctan2(y, x)) % 360.0
        got = float(R.fast_atan2(y, x))
        assert min(abs(got - want), 360 - abs(got - want)) < 0.3, (y, x)
    assert float(R.fast_atan2(0, 0)) == 0.0


def test_a_quarter_turn_of_the_image_turns_every_level_0_angle_by_90_degrees():
    img = S.mosaic(96, 96, seed=2)
    kw = dict(nfeatures=5000, nlevels=1, edgeThreshold=31)
    a, b = R.detect(img, **kw), R.detect(np.ascontiguousarray(np.rot90(img, -1)), **kw)      # clockwise: (x, y) -> (95 - y, x)
    assert len(a["xy"]) == len(b["xy"]) > 10
    moved = {(95 - y, x): ang for (x, y), ang in zip(a["xy"].astype(int).tolist(), a["aux"][:, 1].tolist())}
    for (x, y), ang in zip(b["xy"].astype(int).tolist(), b["aux"][:, 1].tolist()):
        d = (ang - moved[(x, y)] - 90.0) % 360.0
        assert min(d, 360.0 - d) < 0.3, (x, y)                                   # the polynomial's stated 0.3 degrees


def test_an_integer_shift_moves_the_keypoints_and_keeps_their_descriptors():
    img0, img1 = S.shifted_pair()
    kw = dict(nfeatures=5000, nlevels=1)
    a, b = R.detect(img0, **kw), R.detect(img1, **kw)
    assert all(np.isneginf(r["levels"][0]["cut2"]) and r["levels"][0]["cut1"] == 0 for r in (a, b))      # no cut binds
    h, w = img0.shape
    e = 31
    da = {(x, y): i for i, (x, y) in enumerate(a["xy"].astype(int).tolist())}
    db = {(x, y): i for i, (x, y) in enumerate(b["xy"].astype(int).tolist())}
    common = 0
    for (x, y), i in da.items():
        if e <= x - 7 < w - e and e <= y - 4 < h - e:                            # inside both frames' border filter
            j = db[(x - 7, y - 4)]
            assert a["aux"][i].tobytes() == b["aux"][j].tobytes()
            np.testing.assert_array_equal(a["desc"][i], b["desc"][j])
            common += 1
    assert common > 50
    assert sum(1 for (x, y) in db if (x + 7, y + 4) in da) == common


def test_ties_at_either_cut_are_all_kept():
    for score_type in (R.HARRIS_SCORE, R.FAST_SCORE):
        r = R.detect(S.image("tiles"), nfeatures=4, nlevels=1, scoreType=score_type)
        lv = r["levels"][0]
        assert lv["cut1"] > 0 and len(lv["cand"]) == 15
        assert len(set(lv["cand"][:, 2].tolist())) == 1 and lv["live"].all()     # 15 equal scores, first cut to 8 (4): all stay
        assert len(set(lv["resp"].tolist())) == 1 and lv["keep"].all()           # 15 equal responses, second cut to 4: all stay
        assert len(r["xy"]) == 15 > 4
        key = list(zip(r["xy"][:, 1].tolist(), r["xy"][:, 0].tolist()))
        assert key == sorted(key)                                                # equal responses: by y, then x
    # a cut between different values drops what is below it and nothing else
    r = R.detect(S.image("mosaic"), nfeatures=12, nlevels=3)
    for lv, q in zip(r["levels"], r["quotas"]):
        kept = lv["resp"][lv["keep"]]
        assert len(kept) >= min(q, lv["live"].sum())
        assert (lv["resp"][lv["live"] & ~lv["keep"]] < kept.min()).all()
        assert (np.sort(kept)[::-1][q - 1:] == kept.min()).all()                 # beyond the quota: only ties of the cut


def test_refused_parameters():
    assert R.check_params() is None
    for kw, word in ((dict(nfeatures=0), "nfeatures"), (dict(scaleFactor=1.0), "scaleFactor"), (dict(scaleFactor=2.01), "scaleFactor"),
                     (dict(nlevels=0), "nlevels"), (dict(nlevels=17), "nlevels"), (dict(edgeThreshold=2), "edgeThreshold"),
                     (dict(firstLevel=1), "firstLevel"), (dict(WTA_K=3), "WTA_K"), (dict(scoreType=2), "scoreType"),
                     (dict(patchSize=21), "patchSize"), (dict(fastThreshold=0), "fastThreshold"), (dict(fastThreshold=255), "fastThreshold")):
        assert R.check_params(**kw) == word
