"""The AKAZE restatement (tests/akaze_ref.py) on properties that need no cv2: the FED cycles, what one diffusion step conserves,
kcontrast on images whose gradient distribution is known, the M-LDB bit layout, quarter turns, and every case of
akaze_scenes.CASES bound to what it is named for."""
import math

import numpy as np

import akaze_ref as R
import akaze_scenes as S

U = 2.0 ** -24                     # the unit roundoff of float32


def test_fed_cycles_sum_to_their_time_and_are_a_permutation_of_the_unordered_cycle():
    counts = []
    for noct, nol in ((4, 4), (8, 1), (3, 5)):
        lv = R.levels(16384, 16384, noct, nol)
        for a, b in zip(lv, lv[1:]):
            T = b["etime"] - a["etime"]
            steps, raw = R.fed_steps(T), R.fed_unordered(T)
            assert sorted(steps.tolist()) == sorted(raw.tolist()) and len(steps) >= 1
            # n float32 roundings of values that sum to T, and the cycle's own closed form (exact in real arithmetic)
            assert abs(float(steps.astype(np.float64).sum()) - T) <= len(steps) * U * T + 1e-12 * T
            assert (steps > 0).all()
            if (noct, nol) == (4, 4):
                counts.append(len(steps))
    assert counts == [3, 3, 4, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 29] and sum(counts) == 166
    assert len(set(R.fed_steps(100.0).tolist())) == len(R.fed_steps(100.0)) and not np.array_equal(R.fed_steps(100.0), R.fed_unordered(100.0))


def _step_bound(npix, tau, lmax):
    # per pixel: 4 products of at most 2 * 2 lmax, 3 sums of at most 16 lmax, the scaling by 0.5 tau, the final sum: < 40 roundings
    # of magnitudes within 16 lmax max(1, tau)
    return npix * 40 * U * 16 * lmax * max(1.0, tau)


def test_one_step_with_unit_conductivity_on_an_impulse_conserves_the_sum_and_spreads_by_two_tau_per_axis():
    h, w, tau = 21, 25, np.float32(0.2)
    L = np.zeros((h, w), np.float32)
    L[10, 12] = 1
    out = R.nld_step(L, np.ones((h, w), np.float32), tau)
    bound = _step_bound(h * w, float(tau), 1.0)
    o = out.astype(np.float64)
    assert abs(o.sum() - 1.0) <= bound
    yy, xx = np.mgrid[0:h, 0:w]
    for axis, c in ((xx, 12), (yy, 10)):
        assert abs((o * (axis - c) ** 2).sum() - 2 * float(tau)) <= bound * 4          # (offsets of at most 1, squared)
    assert abs(float(out[10, 12]) - (1 - 4 * float(tau))) <= 8 * U and np.count_nonzero(out) == 5


def test_any_conductivity_conserves_the_sum_over_the_whole_plane_borders_included():
    rng = np.random.default_rng(3)
    for h, w in ((37, 53), (2, 9), (1, 1), (5, 1)):
        L = rng.uniform(0, 1, (h, w)).astype(np.float32)
        c = rng.uniform(0.01, 1, (h, w)).astype(np.float32)
        for tau in (0.05, 0.25, 1.7):
            out = R.nld_step(L, c, np.float32(tau))
            assert abs(out.astype(np.float64).sum() - L.astype(np.float64).sum()) <= _step_bound(h * w, tau, 1.0)
            assert not np.array_equal(out, L) or h * w == 1


def test_kcontrast_of_ramps_with_a_known_gradient_distribution():
    # a ramp of one grey level per pixel: away from the replicated left and right borders the blurred image is the ramp and the
    # Scharr magnitude is 32 / 255 everywhere, so nearly every counted pixel falls into the last bin and k = hmax (300 / 300)
    ramp = np.tile(np.arange(255, dtype=np.float32) / np.float32(255), (20, 1))
    k, hmax, npoints = R.kcontrast(ramp)
    assert abs(float(hmax) - 32 / 255) < 1e-5 and k == hmax and npoints == 18 * 253
    # flat columns beside the ramp have a zero gradient and are NOT counted: counted, they would put the percentile into bin 0
    wide = np.concatenate([ramp, np.full((20, 600), ramp[0, -1], np.float32)], axis=1)
    k2, hmax2, npoints2 = R.kcontrast(wide)
    assert k2 == hmax2 and abs(float(hmax2) - 32 / 255) < 1e-5 and npoints2 < 18 * 260
    # two slopes: a sixth of the columns at 3 grey levels per pixel, the rest (83 %) at 1: the 70th percentile lies among the gentle
    # ones, whose bin is floor(300 / 3) = 100 (or 99 by a rounding of the ratio); k is that bin's upper edge
    x = np.concatenate([np.arange(500), 499 + 3 * np.arange(1, 101)]).astype(np.float32)
    two = np.tile(x / np.float32(1000), (12, 1))
    k3, hmax3, _ = R.kcontrast(two)
    assert abs(float(hmax3) - 96 / 1000) < 1e-5
    assert float(k3) in (float(hmax3 * (np.float32(b) / np.float32(300))) for b in (100, 101))
    assert R.kcontrast(np.full((9, 9), 0.3, np.float32))[0] == np.float32(0.03)      # no gradient at all: the fallback


def test_the_mldb_bit_layout():
    layout = R.bit_layout()
    assert len(layout) == R.DESC_BITS == 486 and R.DESC_BYTES * 8 - R.DESC_BITS == 2
    for g, pairs in enumerate((6, 36, 120)):
        for ch in range(3):
            got = [(i, j) for gg, cc, i, j in layout if (gg, cc) == (g, ch)]
            n = (g + 2) ** 2
            assert len(got) == pairs and got == [(i, j) for i in range(n) for j in range(i + 1, n)]
    assert [layout.index(next(e for e in layout if e[0] == g)) for g in range(3)] == [0, 18, 126]
    rng = np.random.default_rng(0)
    ones = R.mldb_bits([np.tile(-np.arange(n * n, dtype=np.float32)[:, None], (1, 3)) for n in (2, 3, 4)])    # every v_i > v_j
    assert ones[:60].tolist() == [255] * 60 and ones[60] == 0x3F
    for _ in range(4):
        d = R.mldb_bits([rng.normal(size=(n * n, 3)).astype(np.float32) for n in (2, 3, 4)])
        assert d.shape == (61,) and d.dtype == np.uint8 and not d[60] & 0xC0
    assert not R.mldb_bits([np.zeros((n * n, 3), np.float32) for n in (2, 3, 4)]).any()       # strictly greater


def _level(lt, lx, ly):
    h, w = lt.shape
    lv = [dict(octave=0, w=w, h=h)]
    return lv, [dict(Lt=lt, Lx=lx, Ly=ly)]


def test_a_quarter_turn_of_the_gradient_field_turns_the_angle_by_90_degrees():
    h = w = 81
    for phi in (10.0, 33.0, 100.0, 200.0, 281.0):
        angles = []
        for turn in (0, 90):
            a = math.radians(phi + turn)
            lv, planes = _level(np.zeros((h, w), np.float32), np.full((h, w), math.cos(a), np.float32), np.full((h, w), math.sin(a), np.float32))
            angles.append(float(R.orientation(lv, planes, dict(level=0, x=np.float32(40), y=np.float32(40), size=np.float32(4.8)))))
        # every sample has the field's direction, so every window that holds it sums the same vector; fastAtan2 is within 0.3
        # degrees of atan2 (its stated accuracy), twice
        assert abs((angles[1] - angles[0]) % 360 - 90) <= 0.6 and abs(angles[0] - phi) <= 0.3


def test_a_quarter_turn_and_the_intensity_bits_of_the_2x2_grid():
    """sample (k, l) lies at x = xf + (k co - l si) s, y = yf + (l co + k si) s and belongs to cell (k // step) cells + l // step.
    Turning the ANGLE by 90 degrees (co 0, si 1) puts cell (a, b) over the image's quadrant (x half 1 - b, y half a), where the
    angle 0 has cell (b', a') = quadrant (x half a', y half b'): the values are permuted by v'[2 a + b] = v[2 (1 - b) + a], up to
    the column the half-open range [-10, 10) shifts.  Turning the IMAGE with the angle brings every sample back onto the same
    pixel: the bits are those of the unturned patch."""
    h = w = 81
    yc = xc = 40
    yy, xx = np.mgrid[0:h, 0:w]
    quad = np.array([[1.0, 0.7], [0.4, 0.1]], np.float32)[(xx >= xc).astype(int), (yy >= yc).astype(int)]      # [x half][y half]
    zero = np.zeros((h, w), np.float32)
    key = dict(level=0, x=np.float32(xc), y=np.float32(yc), size=np.float32(4.8))
    lv, planes = _level(quad, zero, zero)
    v0 = R.mldb_values(lv, planes, dict(key, angle=np.float32(0)))[0][:, 0]
    v90 = R.mldb_values(lv, planes, dict(key, angle=np.float32(90)))[0][:, 0]
    assert v0.tolist() == [np.float32(1.0), np.float32(0.7), np.float32(0.4), np.float32(0.1)]
    want = np.array([v0[2 * (1 - b) + a] for a in range(2) for b in range(2)])
    assert np.abs(v90 - want).max() <= 0.9 / 10 + 1e-6                  # one of a cell's ten columns comes from the neighbouring quadrant
    assert [bool(v90[i] > v90[j]) for i in range(4) for j in range(i + 1, 4)] == [bool(want[i] > want[j]) for i in range(4) for j in range(i + 1, 4)]
    turned = np.zeros_like(quad)
    dy, dx = yy - yc, xx - xc
    turned[yc + dx, xc - dy] = quad                                      # the content at (dx, dy) moves to (-dy, dx)
    lv2, planes2 = _level(turned, zero, zero)
    for g, (a, b) in enumerate(zip(R.mldb_values(lv, planes, dict(key, angle=np.float32(0))), R.mldb_values(lv2, planes2, dict(key, angle=np.float32(90))))):
        np.testing.assert_array_equal(a[:, 0], b[:, 0], err_msg=f"grid {g}")
    d0 = R.mldb_bits(R.mldb_values(lv, planes, dict(key, angle=np.float32(0))))
    d90 = R.mldb_bits(R.mldb_values(lv2, planes2, dict(key, angle=np.float32(90))))
    assert d0[0] & 0x3F == d90[0] & 0x3F == 0x3F


def _ref(name):
    scene, h, w, kw = S.CASES[name]
    return S.reference(scene, h, w, **kw)


def test_every_case_is_bound_to_what_it_is_named_for():
    octaves = {name: (len(_ref(name)["levels"]), _ref(name)["levels"][-1]["octave"] + 1) for name in S.CASES}
    assert octaves["one_octave"] == (4, 1) and octaves["two_octaves"] == (8, 2) and octaves["three_octaves"] == (12, 3)
    assert octaves["four_octaves_defaults"] == (16, 4) and octaves["octaves_1"] == (4, 1) and octaves["layers_1"] == (2, 2) and octaves["layers_5"] == (5, 1)
    assert (octaves["cut_159x80"], octaves["cut_160x79"], octaves["cut_160x80"]) == ((4, 1), (4, 1), (8, 2))
    lv = _ref("two_octaves")["levels"]
    assert (lv[4]["w"], lv[4]["h"]) == (81, 41) and (163 // 2 // 2 < 80)
    four = _ref("four_octaves_defaults")
    assert [L["sigma_size"] for L in four["levels"]] == [2, 3, 3, 4] * 4
    assert {int(i > 0 and L["w"] * L["h"] <= R.WG_PIXELS) for i, L in enumerate(four["levels"])} == {0, 1}
    assert sum(len(R.fed_steps(b["etime"] - a["etime"])) for a, b in zip(four["levels"], four["levels"][1:])) == 166
    # suppression across and within levels, a rejected refinement, where the scan decides otherwise, samples outside the level
    three = _ref("three_octaves")
    assert (three["kind"] == 1).sum() >= 1 and (three["kind"] == 2).sum() >= 1
    assert int(three["survives"].sum()) - three["n_refined"] >= 1
    assert three["scan_differs"] >= 1 and three["outside"] >= 1
    assert (four["kind"] == 1).sum() >= 1 and (four["kind"] == 2).sum() >= 1
    for name in S.CASES:
        r = _ref(name)
        assert len(r["xy"]) == len(r["desc"]) == len(r["lvl"]) and r["desc"].dtype == np.uint8
        order = [(k["class_id"], k["r"], k["c"]) for k in r["kept"]]
        assert order == sorted(order) and len(set(order)) == len(order)
    # the thresholds, the cut, the tie at the cut
    base = _ref("one_octave")
    assert len(_ref("threshold_rejects_most")["cand"]) < len(base["cand"]) // 10 and len(_ref("threshold_rejects_most")["xy"]) >= 1
    assert len(_ref("threshold_rejects_none")["cand"]) > len(base["cand"])
    cut = _ref("max_points_cuts")
    assert len(cut["xy"]) == 10 < cut["n_refined"] and sorted(cut["aux"][:, 2].tolist()) == sorted(k["response"] for k in base["kept"])[-10:]
    tie = _ref("max_points_cuts_on_a_tie")
    resp = sorted(tie["aux"][:, 2].tolist(), reverse=True)
    assert 3 < len(tie["xy"]) < tie["n_refined"] and resp[2] == resp[-1]              # the third largest is shared down to the last kept row
    tiles = _ref("tiles")
    assert len(set(tiles["aux"][:, 2].tolist())) < len(tiles["xy"]) // 2               # repeated structure: equal responses
    assert len(_ref("three_channels")["xy"]) > 10 and not np.array_equal(_ref("three_channels")["xy"], base["xy"])
    const = _ref("constant")
    assert len(const["xy"]) == 0 and const["kcontrast"][0] == np.float32(0.03) and len(const["planes"]) == 4
    thin = _ref("thin_10")
    assert len(thin["xy"]) == 0 and thin["planes"] == [] and thin["levels"][0]["border"] == 5
    assert len(R.UNCONFIRMED) >= 10
