"""The stage helper of the ALIKED GPU tests (tests/aliked_stages.py) checked on the CPU: it reproduces the float64 oracle stage
by stage, the quadratic form of the aggregation equals the direct norm where a level is one pixel thin, and the bars of
tests/test_aliked_stages_gpu.py see the faults they are there for (a mutated float64 reference is at least 100 bars away from
the true one, on the same input)."""
import numpy as np
import pytest
import torch

import aliked_stages as S
import frames
from conftest import load_pkg

M_FP32, M_SPLIT = 4, 16                  # the margins of the GPU stage tests (their docstring)
TEETH = 100.0
_CHAINS = {}


def _chain(h, w, seed, max_kpts=1024):
    """Every stage value of one frame, float64, each from the previous stage's float64 output (cached)."""
    key = (h, w, seed)
    if key in _CHAINS:
        return _CHAINS[key]
    sd = load_pkg("weights").random_aliked_state_dict(seed)
    image = frames.noise_frame(seed, h=h, w=w)
    d = S.dims(h, w)
    c = dict(sd=sd, image=image, d=d)
    c["img"] = S.padded_image(image)
    c["x0"] = c["img"]
    for i in (1, 2, 3, 4):
        c["x%d" % i] = S.block(sd, i, c["x%d" % (i - 1)])
        c["g%d" % i] = S.gate(sd, i, c["x%d" % i])
    g = [c["g%d" % i] for i in (1, 2, 3, 4)]
    c["s8"], c["rnorm"] = S.aggregate(sd, *g)
    c["score"] = S.score_tail(sd, c["s8"], d)
    c["fmap"] = S.feature_map(*g, c["rnorm"], d)
    c["kp"], c["ks"], c["idx"] = S.refine(c["score"], max_kpts)
    c["pos"], c["decided"] = S.positions(sd, c["fmap"], c["kp"])
    c["desc"] = S.descriptors(sd, c["fmap"], c["pos"])
    _CHAINS[key] = c
    return c


@pytest.mark.parametrize("h,w,seed", [(16, 2048, 0), (100, 1000, 1)])
def test_helper_chain_reproduces_the_float64_oracle(h, w, seed):
    """One thin frame (8 x 1024 network, a 1/32 level one pixel high) and one noise frame with several row blocks."""
    c = _chain(h, w, seed)
    d, dbg = c["d"], None
    out = S.extract(c["sd"], c["image"], 1024)
    dbg = out["debug"]
    crop = lambda a: a[..., d["pt"]:d["pt"] + d["h"], d["pl"]:d["pl"] + d["w"]]                 # noqa: E731
    pairs = [("img", crop(c["img"]), dbg["img"][0]), ("score_map", c["score"], dbg["score_map"][0, 0]),
             ("feature_map", c["fmap"], dbg["feature_map"][0]), ("kp_norm", c["kp"], dbg["kp_norm"]),
             ("scores", c["ks"], out["scores"]), ("descriptors", c["desc"], out["descriptors"])]
    pairs += [(k, c[k], dbg[k][0]) for k in ("x1", "x2", "x3", "x4", "g1", "g2", "g3", "g4")]
    wh = np.array([d["w"] - 1, d["h"] - 1], np.float64)
    kwh = (c["kp"] / 2 + 0.5) * wh
    pairs.append(("offsets", c["pos"] - kwh[:, None, :], dbg["offsets"]))
    assert len(c["kp"]) > 100
    np.testing.assert_array_equal(c["idx"], out["indices"])
    for name, got, want in pairs:
        want = want.numpy() if isinstance(want, torch.Tensor) else want
        assert got.dtype == np.float64 and got.shape == want.shape, name
        # offsets are a difference of positions up to ~1300: 1e-12 of the POSITIONS' maximum
        scale = np.abs(c["pos"]).max() / np.abs(want).max() if name == "offsets" else 1.0
        assert S.err(got, want) <= 1e-12 * scale, (name, S.err(got, want))


@pytest.mark.parametrize("h,w", [(16, 2048), (2048, 16)])
def test_quadratic_form_of_the_planes_is_the_direct_norm(h, w):
    """sum_c up(g_c)^2 from planes 8..12 against the upsampled level squared, at every pixel: the 1/32 level here is one pixel
    high (or wide), so x1 == x0 (y1 == y0) on every tap and the clamped H / D1 / D2 planes carry the whole cross term."""
    c = _chain(h, w, 0)
    d = c["d"]
    assert 1 in c["g4"].shape[1:]
    for i, s in ((2, 2), (3, 8), (4, 32)):
        g = c["g%d" % i]
        pre = S.pre_planes(c["sd"], i, g)
        assert pre.shape == (13,) + g.shape[1:]
        up = torch.nn.functional.interpolate(torch.from_numpy(g)[None], scale_factor=s, mode="bilinear", align_corners=True)[0]
        direct = (up * up).sum(0).numpy()
        assert S.err(S.norm2_from_planes(pre, d["Hp"], d["Wp"]), direct) <= 1e-12, i
        # ... and planes 0..7 upsampled are the level's share of the first score-head layer
        ws0 = torch.from_numpy(np.asarray(c["sd"]["score_head.0.weight"], np.float64)[:, 32 * (i - 1):32 * i])
        share = torch.nn.functional.conv2d(up[None], ws0)[0].numpy()
        proj = torch.nn.functional.interpolate(torch.from_numpy(pre[:8])[None], scale_factor=s, mode="bilinear", align_corners=True)[0]
        assert S.err(proj.numpy(), share) <= 1e-12, i


# --------------------------------------------------------------------------- #
#  the bars have teeth
# --------------------------------------------------------------------------- #
def _teeth(true64, ref32, mutated, m):
    """deviation of the mutated float64 reference / the stage's bar, both relative to max |true|."""
    bar = S.bar(m, S.err(ref32, true64))
    return S.err(mutated, true64) / bar


def _rnorm_without_d2(c, level):
    d = c["d"]
    n2 = (c["g1"] ** 2).sum(0)
    for i in (2, 3, 4):
        n2 = n2 + S.norm2_from_planes(S.pre_planes(c["sd"], i, c["g%d" % i]), d["Hp"], d["Wp"], drop_d2=(i == level))
    return 1.0 / np.sqrt(n2)


@pytest.mark.parametrize("h,w,level", [(16, 2048, 2), (16, 2048, 3), (640, 24, 2), (640, 24, 3), (640, 24, 4), (100, 1000, 4)])
def test_bar_sees_the_d2_term_dropped_from_one_level(h, w, level):
    """The r06 fault: n2 without the D2 term of one level's quadratic form.  (Not level 4 of the 8-row network: a level one
    pixel high has ly = 0 on every tap, so its D2 coefficient hy lx * ly hx is zero and the term cannot be missed there; the
    2-pixel level of 640 x 24 and the 4 x 32 one of 100 x 1000 stand in.)"""
    c = _chain(h, w, 0)
    g = [c["g%d" % i] for i in (1, 2, 3, 4)]
    assert S.err(_rnorm_without_d2(c, 0), c["rnorm"]) <= 1e-12                    # the form itself, nothing dropped
    r32 = S.aggregate(c["sd"], *g, dtype=np.float32)[1]
    assert _teeth(c["rnorm"], r32, _rnorm_without_d2(c, level), M_FP32) >= TEETH


@pytest.mark.parametrize("h,w", [(16, 2048), (640, 24)])
def test_bar_sees_align_corners_false(h, w):
    c = _chain(h, w, 0)
    g = [c["g%d" % i] for i in (1, 2, 3, 4)]
    ref32 = S.aggregate(c["sd"], *g, dtype=np.float32)
    mut = S.aggregate(c["sd"], *g, align_corners=False)
    for true, r32, mu in zip((c["s8"], c["rnorm"]), ref32, mut):
        assert _teeth(true, r32, mu, M_FP32) >= TEETH


DCN_RULE = "(py <= -1) | (py >= H) | (px <= -1) | (px >= W)"


@pytest.mark.parametrize("h,w", [(16, 2048), (640, 24)])
@pytest.mark.parametrize("i", [3, 4])
def test_bar_sees_a_weakened_deformable_border_rule(h, w, i):
    """torchvision's rule: a sample at or beyond -1 (or H) contributes nothing.  Weakened by one pixel (`<= -2`) the corner
    masks alone decide, and a sample in (-2, -1) picks up row / column 0 through the un-masked upper corner.

    The weakening `<= -1` -> `< -1` is NOT a fault: a sample AT -1 has weight ly = 0 on row 0, the only row its corners could
    read, so both rules give bit-identical maps on every input.  That is asserted here instead of a deviation, so that a
    change of the oracle's corner masks that makes the boundary case matter is noticed."""
    c = _chain(h, w, 0)
    x = c["x%d" % (i - 1)]
    true = c["x%d" % i]
    same = S.block(c["sd"], i, x, M=S.oracle(np.float64, [(DCN_RULE, "(py < -1) | (py >= H) | (px < -1) | (px >= W)")]))
    np.testing.assert_array_equal(same, true)
    mut = S.block(c["sd"], i, x, M=S.oracle(np.float64, [(DCN_RULE, "(py <= -2) | (py >= H) | (px <= -2) | (px >= W)")]))
    assert _teeth(true, S.block(c["sd"], i, x, dtype=np.float32), mut, M_SPLIT) >= TEETH


@pytest.mark.parametrize("h,w", [(24, 640), (640, 24), (100, 1000)])
def test_bar_sees_reflect_padding(h, w):
    c = _chain(h, w, 0)
    assert c["d"]["pt"] + c["d"]["pl"] > 0
    mut = S.padded_image(c["image"], pad_mode="reflect")
    assert _teeth(c["img"], S.padded_image(c["image"], np.float32), mut, M_FP32) >= TEETH


@pytest.mark.parametrize("h,w,edit", [(16, 2048, ("corner[:, 1].clamp(min=0", "corner[:, 1].clamp(min=1")),
                                      (16, 2048, ("max=h - 1 - ps", "max=h - 2 - ps")),
                                      (2048, 16, ("corner[:, 0].clamp(min=0", "corner[:, 0].clamp(min=1")),
                                      (2048, 16, ("max=w - 1 - ps", "max=w - 2 - ps"))])
def test_bar_sees_a_patch_clamp_off_by_one(h, w, edit):
    """Each clamp of `get_patches` moved by one towards the inside, across the 8-pixel side of the map, where keypoints sit two
    pixels from the border and the clamps act on many of them.  (Moved OUTWARD the upper clamps act on no keypoint of these
    frames: `long(long(kwh) - 0.5)` reaches `h - 1 - ps + 1` only for a keypoint refined by a whole pixel towards the border.)"""
    c = _chain(h, w, 0)
    dec = c["decided"]
    assert dec.mean() > 0.98
    p32, _ = S.positions(c["sd"], c["fmap"], c["kp"], dtype=np.float32)
    mut, _ = S.positions(c["sd"], c["fmap"], c["kp"], M=S.oracle(np.float64, [edit]))
    assert _teeth(c["pos"][dec], p32[dec], mut[dec], M_FP32) >= TEETH
