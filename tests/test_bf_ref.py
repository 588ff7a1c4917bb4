"""The restatement of cv2.BFMatcher.match (tests/bf_ref.py) against itself: the plain double loop and the vectorised form agree,
the cross-checked result is symmetric, planted pairs are found, and the inputs of the GPU tests have the properties those
tests rely on.  No GPU."""
import numpy as np
import pytest

import bf_cases
import bf_ref

CASES = {c["name"]: c for c in bf_cases.exact_cases() + [bf_cases.l2_unit_case()]}


def test_the_unconfirmed_points_are_listed():
    assert len(bf_ref.UNCONFIRMED) == 6 and "PARITY UNPINNED" in bf_ref.__doc__


@pytest.mark.parametrize("name", list(CASES))
def test_loop_and_vectorised_forms_agree(name):
    c = CASES[name]
    nearest = bf_ref.nearest_loop(c["q"], c["t"], c["norm"])
    for cc in (False, True):
        ij, dist = bf_cases.expected(c, cc)
        ij_l, dist_l = bf_ref.match_loop(c["q"], c["t"], c["norm"], cc, nearest=nearest)
        np.testing.assert_array_equal(ij_l, ij)
        np.testing.assert_array_equal(dist_l, dist)
        assert dist.dtype == np.float32 and ij.dtype == np.int32 and ij.shape == (len(dist), 2)
        assert (np.diff(ij[:, 0]) > 0).all()                               # query order, a query at most once
        if not cc and name != "l2_nonfinite_40x50_d16":
            assert len(ij) == len(c["q"])                                  # every query row has a nearest train row
        if cc:
            assert len(set(ij[:, 1].tolist())) == len(ij)                  # mutual: a train row at most once


@pytest.mark.parametrize("name", list(CASES))
def test_cross_check_is_symmetric(name):
    c = CASES[name]
    ij, dist = bf_cases.expected(c, True)
    ji, dist_r = bf_ref.match(c["t"], c["q"], c["norm"], True)
    a = {(int(i), int(j)): float(d) for (i, j), d in zip(ij, dist)}
    b = {(int(i), int(j)): float(d) for (j, i), d in zip(ji, dist_r)}
    assert a == b


def test_d1_hamming_is_all_ties_and_the_lowest_index_wins():
    c = CASES["ham_257x191_d1"]
    ij, dist = bf_cases.expected(c, False)
    d = bf_ref.distances(c["q"], c["t"], c["norm"])
    assert ((d == d.min(1, keepdims=True)).sum(1) > 1).mean() > 0.25       # nine values of d: a tied minimum is common
    for (i, j), v in zip(ij, dist):
        assert v == d[i].min() and j == np.nonzero(d[i] == v)[0][0]


def test_exact_l2_sums_are_exact_in_any_order_and_tie():
    """Integer-valued rows: every sum is an integer below 2^24, so any order of accumulation gives the same float32, and a row's
    two smallest sums are often EQUAL - real ties for the lowest index to win.  (A tie that only the root makes - two
    different sums with one float32 root - needs sums above 2^22, where neighbouring roots are closer than an ulp; these
    rows stay below 512 * 16^2 = 2^17, so none occurs here: the comparison after the root is the kernel's by construction,
    its key holds the root's bits.)"""
    tied = 0
    for c in bf_cases.l2_exact_cases():
        d = bf_ref.distances(c["q"], c["t"], c["norm"])
        sq = ((c["q"].astype(np.float64)[:, None] - c["t"].astype(np.float64)[None]) ** 2).sum(-1)
        assert sq.max() <= 2 ** 17
        assert np.array_equal(d, np.sqrt(sq.astype(np.float32)))           # exact sums: any order gives these bits
        if len(c["t"]) >= 2:
            tied += int((bf_ref.gaps(sq) == 0).sum())
            roots = np.sqrt(np.unique(sq).astype(np.float32))
            assert len(np.unique(roots)) == len(roots)                     # different sums, different roots
    assert tied > 100


def test_every_planted_pair_is_found_and_mutual():
    c = CASES["ham_planted_300x280_d32"]
    assert len(c["planted"]) == 200
    for cc in (False, True):
        ij, dist = bf_cases.expected(c, cc)
        got = {(int(i), int(j)): float(d) for (i, j), d in zip(ij, dist)}
        for i, j in c["planted"]:
            assert 1 <= got[(int(i), int(j))] <= 3


def test_non_finite_rows_never_match():
    c = CASES["l2_nonfinite_40x50_d16"]
    for cc in (False, True):
        ij, dist = bf_cases.expected(c, cc)
        assert bf_cases.NONFINITE_QUERY not in ij[:, 0] and bf_cases.NONFINITE_TRAIN not in ij[:, 1]
        assert np.isfinite(dist).all()
    assert len(bf_cases.expected(c, False)[0]) == 39


@pytest.mark.parametrize("seed", [0, 2])
def test_unit_rows_leave_float32_no_choice(seed):
    """The float32 chain errs by at most (D + 2) 2^-24 S on a squared distance S (D = 128, S <= 2.9 with seed 0: 2.2e-5; no
    two unit rows are further apart than S = 4: 3.1e-5), so a gap of 1e-4 between the best and the second-best squared
    distance, over rows and over columns, makes the float64 argmin the only legal answer - for every row, nothing left out.
    (Seed 1 fails this.)"""
    c = bf_cases.l2_unit_case(seed)
    sq = bf_ref.distances(c["q"], c["t"], c["norm"], "f64") ** 2
    assert sq.max() <= (2.9 if seed == 0 else 4.0)
    assert bf_ref.gaps(sq).min() >= 1e-4 and bf_ref.gaps(sq.T).min() >= 1e-4
    ij64, d64 = bf_ref.match(c["q"], c["t"], c["norm"], True, "f64")
    ij32, d32 = bf_ref.match(c["q"], c["t"], c["norm"], True)
    np.testing.assert_array_equal(ij32, ij64)
    assert (np.abs(d32 - d64) <= 1e-5 * d64).all()
    if seed == 0:
        assert len(ij64) == 114
        assert 2.3e-4 < bf_ref.gaps(sq).min() < 2.5e-4 and 2.6e-4 < bf_ref.gaps(sq.T).min() < 2.8e-4


def test_empty_sides_give_no_match():
    q = np.zeros((0, 32), np.uint8)
    t = np.zeros((5, 32), np.uint8)
    for a, b in ((q, t), (t, q), (q, q)):
        ij, dist = bf_ref.match(a, b, bf_ref.NORM_HAMMING, True)
        assert ij.shape == (0, 2) and dist.shape == (0,)
