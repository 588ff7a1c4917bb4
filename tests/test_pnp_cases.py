"""The cases of tests/pnp_cases.py on the restatement alone (oracle/pnp_ref.py): each one reaches the branch it is named
for.  A case that does not is a failure here, before any kernel is compared."""
import math

import numpy as np
import pytest

import pnp_cases as C
import pnp_scenes as S
from oracle import pnp_ref as O
from oracle.ransac_ref import update_num_iters


# ---- the trace changes nothing ---------------------------------------------------------------------------------------------
def test_trace_leaves_every_result_bit_identical():
    sc = S.make_scene(22, 100, 0.3, "rand")
    for guess in (False, True):
        a = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, guess, 40, S.CONF)
        tr = {}
        b = O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, guess, 40, S.CONF, trace=tr)
        assert a[0] and b[0] and a[4] == b[4]
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and np.array_equal(a[3], b[3])
        assert len(tr["samples"]) == a[4]["samples"] and tr["lm"]["exit"] in ("cap", "small_step")
        assert tr["samples"][a[4]["sample"]]["good"] == a[4]["inliers"]


def test_guess_run_reuses_the_sample_loop_bit_for_bit():
    """pnp_cases.restated(name, True) refines from the traced last sample; the same as the restatement's own guess run."""
    for name in ("budget_9", "lm_step_guess_2011"):
        c, r = C.case(name), C.restated(name, True)
        ok, rv, tv, mask, info = O.solve_pnp_ransac(c["pts3d"], c["pts2d"], c["K"], c["px"], True, c["iters"], C.CONF)
        assert ok and info == r.info and np.array_equal(mask, r.mask)
        assert rv.tobytes() == r.rvec.tobytes() and tv.tobytes() == r.tvec.tobytes()


# ---- A: every sample's EPnP ------------------------------------------------------------------------------------------------
def test_families_reach_every_epnp_branch():
    """Over the union of the families: each beta approximation wins at least 5 times; solve_for_sign's flip, det < 0, a
    dropped control axis, a singular least-squares solve, a singular Gauss-Newton solve and a NaN model each occur.
    Counted here: beta sets 43 / 89 / 70; flip on 108 subsets, det < 0 on 98, dropped axis / singular solves / NaN on 17."""
    beta = [0, 0, 0]
    seen = dict(flip=0, det_neg=0, dropped_axes=0, ls_singular=0, gn_singular=0, nan_model=0)
    for name in C.FAMILIES:
        for _, _, tr in C.family_restated(name):
            if not tr["nan_model"]:
                beta[tr["beta"]] += 1
            seen["flip"] += any(tr["flip"])
            seen["det_neg"] += any(tr["det_neg"])
            for k in ("dropped_axes", "ls_singular", "gn_singular", "nan_model"):
                seen[k] += bool(tr[k])
    print(beta, seen)
    assert min(beta) >= 5, beta
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", list(C.FAMILIES))
def test_family_sizes_and_models(name):
    """At most 64 subsets; the degenerate families give a NaN model on every subset but the two general-direction lines,
    the others a finite one; at most 2 subsets per family lie beyond the rotation angle the comparison leaves out."""
    rs = C.family_restated(name)
    assert 1 <= len(rs) <= 64
    nan = [tr["nan_model"] for _, _, tr in rs]
    if name in C.NAN_FAMILIES:
        assert sum(nan) >= len(rs) - 2 and all(nan[:6])
    else:
        assert not any(nan)
    for r, t, tr in rs:
        assert tr["nan_model"] == (not np.isfinite(r).all())
    assert sum(C.beyond_angle_bar(r) for r, _, _ in rs) <= 2


def test_duplicate_family_holds_one_point_twice():
    for p3, p2 in C.family("duplicate")[0]:
        assert len(np.unique(p3, axis=0)) == 4 and len(np.unique(p2, axis=0)) == 4


# ---- B: the sample loop at its chunk bounds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.LOOP_CASES))
def test_loop_case_reaches_its_branch(name):
    c, r = C.case(name), C.restated(name)
    assert 6 <= len(c["pts3d"]) <= 60
    exp = c["expect"]
    assert r.ok == exp.get("ok", True)
    for k in ("sample", "samples", "inliers"):
        if k in exp:
            assert r.info[k] == exp[k], (k, r.info)
    if r.ok:
        assert r.info["inliers"] == int(r.mask.sum()) and C.restated(name, True).ok


@pytest.mark.parametrize("h", C.PLANT_H)
def test_planted_winner_is_the_first_clean_sample(h):
    """Sample h lies in the 12 inliers, no earlier one does, and the budget (2840 at 12 of 40) never cuts the loop."""
    full, last = C.restated(f"planted_h{h}_full"), C.restated(f"planted_h{h}_last")
    inl = set(np.flatnonzero(full.mask))
    subs = C.subsets(40, h + 1)
    assert set(subs[h]) <= inl and not any(set(s) <= inl for s in subs[:h])
    assert full.info["sample"] == last.info["sample"] == h and last.info["samples"] == h + 1
    assert full.trace["budgets"] == [C.case(f"planted_h{h}_full")["iters"]]
    assert update_num_iters(C.CONF, 28 / 40, 5, 100000) > 300


@pytest.mark.parametrize("m", C.MAX_ITERS)
def test_max_iters_is_the_sample_count(m):
    assert C.restated(f"max_iters_{m}").info["samples"] == max(m, 1)


@pytest.mark.parametrize("b", list(C.BUDGETS))
def test_budget_lands_on_the_bound(b):
    n, good = C.BUDGETS[b]
    assert update_num_iters(C.CONF, (n - good) / n, 5, S.ITERS) == b
    r = C.restated(f"budget_{b}")
    assert len(C.case(f"budget_{b}")["pts3d"]) == n
    assert r.info["inliers"] == good and r.info["sample"] < 7 and r.info["samples"] == b and r.trace["budgets"][-1] == b


def test_four_inliers_and_five_inlier_winner():
    r = C.restated("four_inliers")
    assert not r.ok and max(s["good"] for s in r.trace["samples"]) <= 4
    r = C.restated("five_inlier_winner")
    assert r.ok and r.info["inliers"] == 5 and r.info["samples"] == 12
    assert len(C.case("six_points")["pts3d"]) == 6 and C.restated("six_points").ok


# ---- C: sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_size_case(n):
    c, r = C.case(f"n{n}"), C.restated(f"n{n}")
    assert len(c["pts3d"]) == n and r.info["samples"] <= 100
    assert r.ok == (n > 6)
    if n in C.LONE_LANE_SIZES:
        assert r.mask[n - 1]                           # the lone lane of the last turn decides a mask entry that is set


@pytest.mark.parametrize("q,pattern", C.DEV_CASES)
def test_association_patterns(q, pattern):
    kop, xyz, kp, sc = C.association(q, pattern)
    m = int((kop >= 0).sum())
    assert len(kop) == q and m == len(sc["pts3d"]) and m == {"all": q, "every_other": q // 2, "past_1024": q - 1024,
                                                             "four": 4, "five": 5}[pattern]
    if pattern == "past_1024":
        assert m >= 6 and not (kop[:1024] >= 0).any()
    assert np.array_equal(kp[kop[kop >= 0]], sc["pts2d"])


# ---- D: the LM ---------------------------------------------------------------------------------------------------------------------
def test_degenerate_last_sample_gives_nan_only_with_a_guess():
    c = C.case("degenerate_last")
    a, b = C.restated("degenerate_last", False), C.restated("degenerate_last", True)
    last = a.trace["samples"][-1]
    assert a.info["samples"] == C.DEGENERATE_H + 1 and last["nan_model"] and last["dropped_axes"] == 1
    assert a.ok and np.isfinite(a.rvec).all() and np.isfinite(a.tvec).all() and a.info["sample"] < C.DEGENERATE_H
    assert b.ok and np.isnan(b.rvec).all() and np.isnan(b.tvec).all() and b.info["lm_iters"] == 20
    assert np.array_equal(a.mask, b.mask) and len(c["pts3d"]) == 60


@pytest.mark.parametrize("name", list(C.LM_PINNED))
def test_lm_pinned_case(name):
    """Every accept / reject decision and every stop test of the trajectory has a relative margin >= 1e-9, steps are
    rejected on the way, and the exit is the one the case is named for."""
    _, _, _, guess, exit_ = C.LM_PINNED[name]
    r = C.restated(name, guess)
    lm = r.trace["lm"]
    assert r.ok and lm["exit"] == exit_ and lm["rejected"] > 0
    assert min(lm["min_margin"], lm["stop_margin"]) >= C.LM_MARGIN
    assert (r.info["lm_iters"] == 20) == (exit_ == "cap")


def test_lm_pinned_cases_cover_both_exits_with_and_without_guess():
    kinds = {(g, e) for _, _, _, g, e in C.LM_PINNED.values()}
    assert kinds == {(False, "cap"), (True, "cap"), (False, "small_step"), (True, "small_step")}
    assert all(sum(1 for v in C.LM_PINNED.values() if v[4] == e) >= 2 for e in ("cap", "small_step"))


def test_lm_k_reaches_its_cap():
    for name, (_, _, noise, guess, _) in C.LM_K_CAP.items():
        assert noise == 0.0 and C.restated(name, guess).trace["lm"]["k_max"] >= 16


# ---- E: the threshold is closed ------------------------------------------------------------------------------------------------------
def test_threshold_case():
    i = C.THRESHOLD_POINT
    base, at, below = (C.restated(n) for n in ("threshold_base", "threshold_at", "threshold_below"))
    px32, lo = C.threshold_px()
    assert np.float32(float(px32) ** 2) == base.err[i] and lo < px32
    assert at.ok and below.ok and at.info["sample"] == below.info["sample"] == base.info["sample"]
    assert at.err[i] == base.err[i] == np.float32(float(px32) ** 2)
    assert at.mask[i] and not below.mask[i]
    assert math.isclose(float(px32) ** 2, float(base.err[i]), rel_tol=1e-6)
