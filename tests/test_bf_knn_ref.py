"""The restatement of knnMatch and of the ratio test (tests/bf_knn_ref.py) against itself on the CPU: the vectorised form
against a plain double loop, k = 1 against `bf_ref.match` without cross-check, the padding for N < k, the ratio test on the
planted case, and the figures the GPU tests rely on (ties at the k-th place, the ratio margins, the gaps of the unit rows)."""
import numpy as np
import pytest

import bf_cases
import bf_knn_ref as R
import bf_ref

EXACT = {c["name"]: c for c in bf_cases.exact_cases()}
SMALL = ["ham_1x1_d1", "ham_1x300_d32", "ham_63x65_d1", "ham_63x65_d61", "l2int_1x300_d3", "l2int_63x65_d1", "l2int_63x65_d129",
         "l2_nonfinite_40x50_d16"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "dist", "cnt")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        np.testing.assert_array_equal(_bits(g) if name == "dist" else g, _bits(w) if name == "dist" else w, err_msg=f"{what} {name}")


def test_unconfirmed_is_listed():
    print("\n".join(R.UNCONFIRMED))
    assert len(R.UNCONFIRMED) >= 5 and any("crossCheck" in u for u in R.UNCONFIRMED) and any("lower train index" in u for u in R.UNCONFIRMED)


@pytest.mark.parametrize("name", SMALL)
def test_vectorised_form_equals_the_double_loop(name):
    c = EXACT[name]
    for k in (1, 2, 3, 8):
        _same(R.knn_of_distances(R.case_distances(c), k), R.knn_loop(c["q"], c["t"], c["norm"], k), f"{name} k={k}")


@pytest.mark.parametrize("name", list(EXACT))
def test_k1_is_match_without_cross_check(name):
    c = EXACT[name]
    idx, dist, cnt = R.knn_of_distances(R.case_distances(c), 1)
    ij, d = bf_cases.expected(c, False)
    rows = np.nonzero(cnt)[0]
    np.testing.assert_array_equal(np.stack([rows, idx[rows, 0]], 1), ij)
    np.testing.assert_array_equal(_bits(dist[rows, 0]), _bits(d))
    assert (idx[cnt == 0] == -1).all() and np.isinf(dist[cnt == 0]).all()


def test_fewer_train_rows_than_k_and_the_non_finite_rows():
    c = EXACT["ham_63x65_d32"]
    for N in (1, 2, 3):
        for k in (2, 3, 8):
            idx, dist, cnt = R.knn(c["q"], c["t"][:N], c["norm"], k)
            assert (cnt == min(k, N)).all() and (idx[:, min(k, N):] == -1).all() and np.isinf(dist[:, min(k, N):]).all()
            assert (np.sort(idx[:, :min(k, N)], 1) == np.arange(min(k, N))).all() if N <= k else True
            assert (np.diff(dist[:, :min(k, N)].astype(np.float64), axis=1) >= 0).all()
    c = EXACT["l2_nonfinite_40x50_d16"]
    idx, dist, cnt = R.knn(c["q"], c["t"], c["norm"], 8)
    assert cnt[bf_cases.NONFINITE_QUERY] == 0 and (idx[bf_cases.NONFINITE_QUERY] == -1).all()
    assert bf_cases.NONFINITE_TRAIN not in idx and (np.delete(cnt, bf_cases.NONFINITE_QUERY) == 8).all()
    idx, dist, cnt = R.knn(c["q"], c["t"][:0], c["norm"], 2)
    assert idx.shape == (40, 2) and (cnt == 0).all()


def test_the_exact_cases_hold_ties_at_the_kth_place():
    """what makes the tie rule a tested rule: rows whose k-th and (k+1)-th neighbours are equally far"""
    ham = [R.tied_rows(R.case_distances(EXACT["ham_257x191_d1"]), k) for k in range(1, 9)]
    l2 = [R.tied_rows(R.case_distances(EXACT["l2int_257x191_d3"]), k) for k in range(1, 9)]
    print("tied rows of 257, k = 1..8: ham_257x191_d1", ham, "l2int_257x191_d3", l2)
    assert min(ham) >= 143 and min(l2) >= 50                                # of 257 rows, for every k


@pytest.mark.parametrize("ratio", [0.7, 0.75, 0.8])
def test_ratio_restatement_keeps_the_planted_pairs(ratio):
    c = bf_cases.planted_hamming()
    idx, dist, cnt = R.knn_of_distances(R.case_distances(c), 2)
    ij, d = R.ratio_of_knn(idx, dist, cnt, ratio)
    np.testing.assert_array_equal(ij, c["planted"])
    margin = np.abs(dist[:, 0].astype(np.float64) - ratio * dist[:, 1].astype(np.float64)).min()
    print(f"ratio {ratio}: {len(ij)} kept, smallest |d1 - ratio d2| = {margin}")
    assert margin > 10.7                                                    # (10.8 up to the rounding of 0.8 * d2: far from a boundary)
    # the Python idiom on DMatch floats
    want = [(i, int(idx[i, 0])) for i in range(len(idx)) if cnt[i] >= 2 and float(dist[i, 0]) < ratio * float(dist[i, 1])]
    assert want == [tuple(p) for p in ij.tolist()]


def test_ratio_equalities_are_dropped_and_exist():
    """integer-valued L2 rows at ratio 0.75: d1 == 0.75 d2 happens (two train rows equal to the query row: 0 == 0.75 * 0) and
    such a row is not kept"""
    n_eq = 0
    for name in ("l2int_257x191_d1", "l2int_257x191_d3", "l2int_63x65_d1"):
        c = EXACT[name]
        idx, dist, cnt = R.knn_of_distances(R.case_distances(c), 2)
        ij, _ = R.ratio_of_knn(idx, dist, cnt, 0.75)
        eq = (cnt >= 2) & (dist[:, 0].astype(np.float64) == 0.75 * dist[:, 1].astype(np.float64))
        n_eq += int(eq.sum())
        assert not set(np.nonzero(eq)[0].tolist()) & set(ij[:, 0].tolist())
    print("rows with d1 == 0.75 d2:", n_eq)
    assert n_eq > 0


def test_unit_rows_leave_float32_no_choice_up_to_k4():
    """the gaps between the first k + 1 sorted squared float64 distances of l2_unit_case(5): >= 6.2e-5, twice the float32
    chain's bound of 3.1e-5 (tests/test_bf_gpu.py), for every row up to k = 4; at k = 8 a few rows fall below"""
    c = bf_cases.l2_unit_case(seed=5)
    sq = np.sort(R.case_distances(c, "f64") ** 2, axis=1)
    gap = {k: np.diff(sq[:, :k + 1], axis=1).min(axis=1) for k in (2, 3, 4, 8)}
    print({k: float(g.min()) for k, g in gap.items()}, "rows below 6.2e-5 at k = 8:", int((gap[8] < 6.2e-5).sum()))
    for k in (2, 3, 4):
        assert gap[k].min() >= 6.2e-5
    assert (gap[8] < 6.2e-5).sum() <= 8
