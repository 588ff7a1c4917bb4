"""The SIFT restatement (tests/sift_ref.py) on its own, without a GPU: properties that do not depend on what it restates - a
shifted scene moves its keypoints with it, a descriptor is invariant under a 90-degree rotation of the image up to the
permutation of its bins, the float64 form of the pyramid agrees with the defined float32 form within a bound derived from the
tap counts - and that every case of tests/sift_scenes.py binds what it is named for.  What was restated from memory is
printed: parity with cv2 is unpinned."""
from collections import Counter

import numpy as np

import sift_ref as R
import sift_scenes as S


def test_what_is_unconfirmed_is_listed():
    assert len(R.UNCONFIRMED) >= 15 and all(isinstance(u, str) and len(u) > 20 for u in R.UNCONFIRMED)
    print("\nsift_ref restates OpenCV from memory; unconfirmed against cv2:")
    for i, u in enumerate(R.UNCONFIRMED, 1):
        print(f" {i:2d}. {u}")


def test_a_shift_of_the_scene_moves_the_keypoints_with_it():
    f0, f1 = S.shifted_pair()                                              # f1 is f0 moved by (7, 4)
    a, b = R.detect(f0), R.detect(f1)
    assert len(a["xy"]) > 100 and len(b["xy"]) > 100
    # the fine octaves away from the frame's edge, where the reflected border does not reach
    fine = ((a["octave"] & 255) >= 255) | ((a["octave"] & 255) == 0)
    inside = (a["xy"][:, 0] > 30) & (a["xy"][:, 0] < 130) & (a["xy"][:, 1] > 30) & (a["xy"][:, 1] < 90)
    pts = a["xy"][fine & inside].astype(np.float64) - (7, 4)
    assert len(pts) > 20
    d = np.abs(pts[:, None, :] - b["xy"][None].astype(np.float64)).max(axis=2).min(axis=1)
    assert (d < 0.01).mean() > 0.9, d


def test_a_descriptor_is_invariant_under_a_quarter_turn_up_to_the_bin_permutation():
    G, _ = R.pyramid(S.image("mosaic", 64, 64))
    P = G[0][2]                                                            # 128 x 128
    w = P.shape[1]
    Q = np.ascontiguousarray(np.rot90(P))                                  # (r, c) -> (w - 1 - c, r)
    for x, y, ori, scl in ((60.3, 70.8, 33.0, 2.0), (31.0, 90.0, 271.5, 1.3), (100.6, 40.2, 0.0, 3.1)):
        x, y, ori, scl = R.F32(x), R.F32(y), R.F32(ori), R.F32(scl)
        d0 = R.descriptor(P, x, y, ori, scl)
        assert d0.shape == (128,) and d0.max() > 50 and np.all(d0 == np.rint(d0))
        x2, y2 = y, R.F32(w - 1) - x
        # the orientation turned with the image: the same vector
        d1 = R.descriptor(Q, x2, y2, R.F32((float(ori) + 90) % 360), scl)
        assert np.abs(d0 - d1).max() <= 1
        # the orientation kept: the 4 x 4 cells turn and the 8 orientation bins move by two
        d2 = R.descriptor(Q, x2, y2, ori, scl)
        want = np.roll(np.rot90(d0.reshape(4, 4, 8), 1, (0, 1)), 2, axis=2).reshape(128)
        assert np.abs(d2 - want).max() <= 1
        assert np.abs(d2 - d0).max() > 20                                  # (and it is not the identity)


def test_the_float64_pyramid_agrees_with_the_defined_float32_form_within_the_derived_bound():
    """A blur pass of n taps on values of magnitude <= 256 makes n products and n sums, each rounded with relative error
    u = 2^-24 of a value <= 256 (the taps are positive and sum to 1 within n u, so every partial sum is bounded by the largest
    input): at most 2 n u 256 per pass, on top of the error of its input, which a pass (a convex combination within n u)
    carries through with gain <= 1 + n u.  The doubling is exact, the decimation copies, float64's own rounding (2^-53) is
    nothing beside it.  A DoG plane adds the errors of its two layers and one rounding of a value <= 256."""
    u = 2.0 ** -24
    for nol, sigma in ((3, 1.6), (2, 2.4)):
        g = S.image("mosaic", S.HS, S.WS)
        g32, d32 = R.pyramid(g, nol, sigma, np.float32)
        g64, d64 = R.pyramid(g, nol, sigma, np.float64)
        n = [len(R.gauss_taps(s)) for s in R.sigmas(sigma, nol)]
        step = lambda e, k: (e * (1 + k * u) + 2 * k * u * 256) * (1 + k * u) + 2 * k * u * 256      # row pass, column pass
        base = step(0.0, n[0])
        worst = 0.0
        for o in range(len(g32)):
            e = [base]
            for i in range(1, nol + 3):
                e.append(step(e[-1], n[i]))
            for i in range(nol + 3):
                err = np.abs(g32[o][i].astype(np.float64) - g64[o][i]).max()
                assert err <= e[i], (o, i, err, e[i])
                worst = max(worst, err / e[i])
            for i in range(nol + 2):
                assert np.abs(d32[o][i].astype(np.float64) - d64[o][i]).max() <= e[i] + e[i + 1] + u * 256
            base = e[nol]
        assert 0 < worst < 1 and e[-1] < 0.1                                # the bound is not vacuous: below a tenth of a grey level


def test_the_cases_bind_what_they_are_named_for():
    def ref(name):
        scene, h, w, kw = S.CASES[name]
        return S.reference(scene, h, w, **kw), kw
    r, _ = ref("defaults")
    why = Counter(r["rejects"].values())
    assert len(r["sizes"]) == 7 and r["sizes"][0] == (262, 194) and r["sizes"][-1] == (4, 3)
    assert [len(c) for c in r["cand"]][:3] == [169, 74, 8] and sum(len(c) for c in r["cand"][3:]) == 0
    assert why["contrast"] == 3 and why["edge"] == 9 and why["steps"] > 0 and why["left"] > 0
    assert len(r["refined"]) - len(r["rejects"]) == 179
    moved = [k for key, k in r["refined"].items() if k is not None and (k["layer"], k["r"], k["c"]) != key[1:]]
    assert len(moved) > 5                                                  # a refinement that moves the sample point
    # a keypoint with two orientations: two rows that share pt, size and response
    npk = Counter(len(R.orientation_peaks(h)) for h in r["hists"].values())
    assert npk[2] > 10 and npk[3] > 0 and r["n_raw"] == sum(k * v for k, v in npk.items()) == 239
    # two extrema that refine to the same keypoint: only the finer mosaic has them, there removeDuplicatedSorted binds
    assert all((ref(name)[0]["n_raw"] > ref(name)[0]["n_unique"]) == (name == "duplicates") for name in S.CASES)
    r, _ = ref("duplicates")
    assert r["n_raw"] - r["n_unique"] == 5 and len(r["xy"]) == r["n_unique"]
    r, _ = ref("defaults")
    r, _ = ref("small")
    assert r["sizes"] == [(82, 66), (41, 33), (20, 16), (10, 8), (5, 4)] and len(r["xy"]) == 20
    assert len(R.gauss_taps(R.sigmas(1.6, 3)[5])) // 2 > 10               # the coarse octaves are smaller than a blur radius
    r, kw = ref("layers_1")
    assert r["gauss"][0].shape[0] == 4 and r["threshold"] == 5 and len(r["xy"]) > 100
    r, kw = ref("layers_5")
    assert r["gauss"][0].shape[0] == 8 and {k[1] for k in r["refined"]} >= {1, 5}
    r, _ = ref("contrast_rejects_most")
    why = Counter(r["rejects"].values())
    assert why["contrast"] > 100 and why["contrast"] > 5 * (len(r["refined"]) - len(r["rejects"])) and len(r["xy"]) > 5
    r, _ = ref("contrast_rejects_none")
    assert r["threshold"] == 0 and "contrast" not in r["rejects"].values() and len(r["xy"]) > 10
    r, _ = ref("edge_2")
    assert Counter(r["rejects"].values())["edge"] > 50
    r, _ = ref("sigma_1_2")
    assert len(R.gauss_taps(R.sigmas(1.2, 3)[0])) < len(R.gauss_taps(R.sigmas(1.6, 3)[0])) and len(r["xy"]) > 100
    r, kw = ref("quota_cuts")
    assert r["n_unique"] > len(r["xy"]) == kw["nfeatures"]
    r, kw = ref("quota_cuts_on_a_tie")
    assert r["n_unique"] > len(r["xy"]) == kw["nfeatures"] + 1
    r, _ = ref("tiles")
    assert len(r["xy"]) > 50
    r, _ = ref("stripes_tie")
    tied = 0
    for o, cand in enumerate(r["cand"]):
        D = r["dog"][o]
        for l, y, x in cand.tolist():
            nb = D[l - 1:l + 2, y - 1:y + 2, x - 1:x + 2]
            tied += (nb == D[l, y, x]).sum() > 1
    # extrema that equal a neighbour are all candidates (whole columns); det = 0 along a stripe, so none becomes a keypoint
    assert tied > 20 and tied == sum(len(c) for c in r["cand"]) and set(r["rejects"].values()) <= {"edge", "left", "steps"} and len(r["xy"]) == 0
    r, _ = ref("thin_12")
    assert r["sizes"][0] == (262, 24) and len(r["cand"][0]) > 0 and len(r["xy"]) > 0
    assert all(5 <= y < 19 for _, y, _ in r["cand"][0].tolist())             # the 14 usable rows of octave 0
    r, _ = ref("no_interior_5x40")
    assert r["sizes"] == [(80, 10), (40, 5)] and len(r["xy"]) == 0
    r, _ = ref("constant")
    assert len(r["sizes"]) == 5 and sum(len(c) for c in r["cand"]) == 0
    assert R.octave_sizes(1, 1) == [] and R.octave_sizes(2, 2) == [(4, 4)]
