"""The stereo restatement (tests/stereo_ref.py) against itself on the CPU: the vectorised aggregation against a scalar per-pixel
loop, the median against np.median, the normalisation rules, the INVALID columns, and two scenes with a planted disparity."""
import numpy as np
import pytest

import stereo_ref as R
import stereo_scenes as SC


def _scalar_aggregate(C, P1, P2):
    """the path recurrence one pixel and one disparity at a time, as the definition reads"""
    H, W1, D = C.shape
    total = np.zeros((H, W1, D), np.int64)
    for dy, dx in R.DIRECTIONS:
        L = np.zeros((H, W1, D), np.int64)
        ys = range(H)
        xs = range(W1) if dx >= 0 else range(W1 - 1, -1, -1)
        for y in ys:
            for x in xs:
                qy, qx = y - dy, x - dx
                inside = 0 <= qy < H and 0 <= qx < W1
                Lq = L[qy, qx] if inside else np.zeros(D, np.int64)
                m = int(Lq.min())
                for d in range(D):
                    lo = int(Lq[d - 1]) + P1 if d > 0 else 32767 + P1
                    hi = int(Lq[d + 1]) + P1 if d < D - 1 else 32767 + P1
                    L[y, x, d] = int(C[y, x, d]) + min(int(Lq[d]), lo, hi, m + P2) - m
        total += L
    return np.minimum(total, 32767).astype(np.int16)


def test_vectorised_aggregation_equals_the_scalar_loop():
    rng = np.random.default_rng(0)
    C = rng.integers(0, 400, (7, 12, 16)).astype(np.int16)
    for P1, P2 in ((2, 5), (40, 160), (300, 301)):
        assert np.array_equal(R.aggregate(C, P1, P2), _scalar_aggregate(C, P1, P2))
    big = rng.integers(9000, 11374, (3, 4, 16)).astype(np.int16)          # the sum of five paths saturates
    S = R.aggregate(big, 800, 3200)
    assert np.array_equal(S, _scalar_aggregate(big, 800, 3200)) and S.max() == 32767


def test_median_equals_np_median():
    rng = np.random.default_rng(1)
    for H, W in ((1, 1), (1, 7), (6, 1), (5, 9), (12, 13)):
        img = rng.integers(-16, 500, (H, W)).astype(np.int16)
        pad = np.pad(img, 1, mode="edge")
        want = np.array([[np.median(pad[y:y + 3, x:x + 3]) for x in range(W)] for y in range(H)]).astype(np.int16)
        assert np.array_equal(R.median3(img), want)


def test_normalisation_rules():
    p = R.Params()
    assert (p.P1, p.P2, p.d12, p.uniq, p.ftzero, p.maxD, p.invalid) == (2, 5, 1, 0, 15, 16, -16)
    p = R.Params(minDisparity=5, numDisparities=32, P1=10, P2=4, disp12MaxDiff=-1, preFilterCap=20, uniquenessRatio=-3)
    assert (p.P1, p.P2, p.d12, p.uniq, p.ftzero, p.maxD, p.invalid) == (10, 11, 1, 10, 21, 37, 64)
    assert R.Params(P1=7, P2=0).P2 == 8 and R.Params(P1=0, P2=3).P2 == 3 and R.Params(P1=0, P2=2).P2 == 3
    assert R.Params(preFilterCap=63).ftzero == 63 and R.Params(preFilterCap=16).ftzero == 17 and R.Params(disp12MaxDiff=3).d12 == 3
    assert R.Params(preFilterCap=63, blockSize=11).max_block_cost() == 121 * 94
    assert R.check_create(100, 50, blockSize=11, preFilterCap=63, P2=32767 - 121 * 94) is None
    assert "largest block cost 11374" in R.check_create(100, 50, blockSize=11, preFilterCap=63, P2=32768 - 121 * 94)
    assert len(R.UNCONFIRMED) >= 5 and any("disp12MaxDiff" in u for u in R.UNCONFIRMED)


def test_every_pixel_lies_on_one_path_per_direction():
    for H, W1 in ((1, 1), (1, 9), (9, 1), (5, 8), (8, 5), (7, 7)):
        for k, (dy, dx) in enumerate(R.DIRECTIONS):
            seen = np.zeros((H, W1), np.int32)
            for pth in range(R.path_count(k, H, W1)):
                y, x, n = R.path_start(k, pth, H, W1)
                assert n >= 1
                for i in range(n):
                    seen[y + i * dy, x + i * dx] += 1
                assert not (0 <= y - dy < H and 0 <= x - dx < W1)       # it starts at the border
            assert (seen == 1).all(), (H, W1, k)


def test_narrow_images_and_leading_columns_are_invalid():
    rng = np.random.default_rng(2)
    for W in (1, 15, 16):
        l, r = rng.integers(0, 256, (2, 5, W), dtype=np.uint8)
        out = R.compute(l, r, R.Params(numDisparities=16, blockSize=3))
        assert out.shape == (5, W) and (out == -16).all()
    l, r = SC.planted_pair(40, 8, 16, 3)
    p = R.Params(minDisparity=2, numDisparities=16, blockSize=3, P1=72, P2=288)
    st = R.compute_stages(l, r, p)
    for k in ("raw", "checked"):
        assert (st[k][:, :18] == 16).all() and st[k].shape == (8, 40)
    assert st["C"].shape == (8, 22, 16) and st["S"].shape == (8, 22, 16)
    assert (st["pf_left"][:, [0, -1]] == p.ftzero).all()


@pytest.mark.parametrize("W,H,D,bs,d0", SC.PLANTED)
def test_planted_constant_disparity_is_found_within_half_a_pixel(W, H, D, bs, d0):
    """The true cost is 0, so the sub-pixel offset lies in -7 .. 8: every computed pixel is valid and within 8 of 16 d0."""
    l, r = SC.planted_pair(W, H, D, d0)
    p = R.Params(**SC.planted_params(D, bs))
    out = R.compute(l, r, p)[:, p.maxD:].astype(np.int32)
    assert (out != p.invalid).all()
    print("worst error", np.abs(out - 16 * d0).max())
    assert np.abs(out - 16 * d0).max() <= 8


def test_two_plane_scene():
    """Measured with this restatement: valid fraction 0.8333 (the 16 columns the nearer block occludes are removed by the left-right
    check: 80 of 96 computed columns stay), share of valid pixels within 16 of the truth 0.9988; the thresholds are those minus 0.02."""
    l, r, truth = SC.two_plane_pair()
    p = R.Params(**SC.planted_params(32, 5))
    out = R.compute(l, r, p)[:, p.maxD:].astype(np.int32)
    valid = out != p.invalid
    good = np.abs(out - 16 * truth[:, p.maxD:])[valid] <= 16
    print("valid", valid.mean(), "within 16", good.mean())
    assert valid.mean() >= 0.8333 - 0.02
    assert good.mean() >= 0.9988 - 0.02


def test_grey_conversion_and_lift_restatement():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)
    g = R.bgr_to_grey(img)
    assert g.dtype == np.uint8 and abs(int(g[0, 0]) - (0.114 * img[0, 0, 0] + 0.587 * img[0, 0, 1] + 0.299 * img[0, 0, 2])) <= 1
    f, B = 700.0, 0.54
    Pl = np.array([[f, 0, 600, 0], [0, f, 180, 0], [0, 0, 1, 0]], float)
    Pr = Pl.copy(); Pr[0, 3] = -f * B
    disp = np.full((20, 30), 16 * 10, np.int16)
    disp[0, 0] = -16
    xy = np.float32([[5.7, 3.2], [0.4, 0.9], [30.0, 3.0], [-0.5, 2.0], [np.nan, 1.0]])
    d, mask, xr, X = R.lift(xy, disp, Pl, Pr, 0.0, 100.0)
    assert mask.tolist() == [True, False, False, True, False] and d[0] == 10 and d[1] == -1
    assert abs(X[0, 2] - f * B / 10) < 1e-6 and np.isnan(X[1]).all()
    assert np.array_equal(xr[0], np.float32([5.7 - 10, 3.2]))
