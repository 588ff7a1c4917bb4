"""The fused gate + pre-aggregation kernels (al_level2_kernel, al_level_small_kernel) and the aggregation behind them, stage by
stage against float64 on level shapes that the seven frames of tests/test_aliked_stages_gpu.py do not reach.

The network's long side is always 1024 (oracle/aliked_ref.py::resize_plan), so a level is never small in both directions: a
network of 96 x 160 or of 32 x 32 does not exist.  What can be reached is a SHORT side that is no whole number of tiles, with
the long side supplying many tiles the other way.  The kernels' tiles are 32 x 8 pixels of the 1/2 level (whole 4 x 4 pooling
cells; its height is always a multiple of 16) and 16 x 4 pixels of the 1/8 and 1/32 levels:

    1024 x 150  network 1024 x 150 in 1024 x 160, pl = 5: level 2 is 80 wide (2.5 tiles, 64 tile rows), level 3 is 20 wide
                (1.25 tiles), level 4 is 5 x 32 - columns 80, 20 and 5 take the clamped right halo inside a partial tile
    150 x 1024  the transpose, 160 x 1024, pt = 5: level 3 is 20 rows (5 tile rows), level 4 is 5 rows (1.25 tiles): the lower
                halo clamps inside a partial tile; 16 x 10 tiles of level 2, a multiple of 8 (the banded placement)
    1024 x 30   network in 1024 x 32: level 4 is ONE pixel wide, every right neighbour clamps (H = S, D1 = D2 = V); level 2 is
                half a tile wide, level 3 a quarter

Stages: g2..g4, pre2..pre4 (projections and S, H, V, D1, D2 apart), g1, s8, rnorm, and x3 - block3 reads the pooled map the
level-2 kernel writes, so a wrong pool shows there.  Helpers, margins (M_FP32 = 4, M_SPLIT = 16) and the rule
err_gpu <= max(m * err_ref, 1e-6) are those of tests/test_aliked_stages_gpu.py.

Measured on the MI355X: err_gpu / err_ref per stage and frame, the largest err_gpu of the stage and the largest err_gpu / bar.

    stage           1024x150 150x1024  1024x30   max err_gpu   max err_gpu / bar
    g2                 1.00     1.00     1.00    4.0e-07       0.25
    g3                 0.64     0.81     0.57    3.0e-07       0.20
    g4                 0.80     0.66     0.69    3.2e-07       0.20
    pre2 proj          1.00     1.01     0.80    2.5e-07       0.25
    pre2 S..D2         1.00     0.98     1.04    2.1e-07       0.21
    pre3 proj          0.80     0.90     0.96    3.0e-07       0.24
    pre3 S..D2         0.97     1.00     1.00    4.1e-07       0.25
    pre4 proj          1.28     1.00     1.00    2.7e-07       0.25
    pre4 S..D2         1.14     0.96     0.91    3.0e-07       0.29
    g1                 1.00     1.00     1.00    2.6e-07       0.25
    s8                 0.09     0.19     0.13    6.1e-07       0.05
    rnorm              0.22     0.24     0.12    2.2e-07       0.06
    x3                 0.80     1.29     0.96    2.8e-06       0.08

Then two properties of the frame stride and of the batch: three different frames through one launch sequence give the three
single-frame extractions bit for bit (outputs, and buffers 10..18 of frame 0), and two instances of different capacities
(another workspace stride) give identical stage buffers for the same frame."""
import numpy as np
import pytest

import aliked_stages as S
import frames
import test_aliked_stages_gpu as T
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAX_KPTS = 512
FRAMES = [(1024, 150), (150, 1024), (1024, 30)]
STAGES = ["g2", "g3", "g4", "pre2", "pre3", "pre4", "g1", "s8", "rnorm", "x3"]
# debug_read buffers 10..18: (which, channels or 0 for a plain map, level divisor, channel-last)
BUFFERS = [(10, 32, 1, True), (11, 0, 1, False), (12, 32, 2, False), (13, 32, 8, False), (14, 32, 32, False),
           (15, 13, 2, False), (16, 13, 8, False), (17, 13, 32, False), (18, 8, 1, False)]

_RUN = {}


@pytest.fixture(scope="module", autouse=True)
def _forget_runs():
    yield
    _RUN.clear()


def _stage_buffers(al, Hp, Wp):
    out = {}
    for which, ch, div, cl in BUFFERS:
        h, w = Hp // div, Wp // div
        out[which] = al.debug_read(which, (h, w, ch) if cl else ((ch, h, w) if ch else (h, w)))
    return out


def _run(h, w):
    """One extraction (seed 0) and the stage buffers the tests below read; the latest frame only is kept."""
    if (h, w) in _RUN:
        return _RUN[(h, w)]
    _RUN.clear()
    sd = load_pkg("weights").random_aliked_state_dict(0)
    al = load_pkg("aliked").AlikedHIP(sd, max_num_keypoints=MAX_KPTS, max_h=h, max_w=w)
    image = frames.noise_frame(0, h=h, w=w)
    xy, desc = al.extract(image, MAX_KPTS)
    d = T._dims(al)
    want = S.dims(h, w)
    assert all(d[k] == want[k] for k in ("h", "w", "Hp", "Wp", "pl", "pt")), (d, want)
    Hp, Wp = d["Hp"], d["Wp"]
    assert len(xy) > 50
    r = dict(sd=sd, d=d)
    for which, name, div, ch in ((3, "x1", 1, 16), (4, "x2", 2, 32), (5, "x3", 8, 64), (6, "x4", 32, 128),
                                 (12, "g2", 2, 32), (13, "g3", 8, 32), (14, "g4", 32, 32),
                                 (15, "pre2", 2, 13), (16, "pre3", 8, 13), (17, "pre4", 32, 13), (18, "s8", 1, 8)):
        r[name] = al.debug_read(which, (ch, Hp // div, Wp // div))
    r["g1"] = np.ascontiguousarray(al.debug_read(10, (Hp, Wp, 32)).transpose(2, 0, 1))
    r["rnorm"] = al.debug_read(11, (Hp, Wp))
    al.close()
    for k, v in r.items():
        if isinstance(v, np.ndarray):
            assert np.isfinite(v).all(), k
    _RUN[(h, w)] = r
    return r


def test_the_frames_reach_partial_tiles():
    """The shapes the docstring promises, from the oracle's own size rule."""
    lv = lambda h, w: [(S.dims(h, w)["Hp"] // s, S.dims(h, w)["Wp"] // s) for s in (2, 8, 32)]           # noqa: E731
    assert lv(1024, 150) == [(512, 80), (128, 20), (32, 5)]
    assert lv(150, 1024) == [(80, 512), (20, 128), (5, 32)]
    assert lv(1024, 30) == [(512, 16), (128, 4), (32, 1)]
    assert 80 % 32 and 80 > 32 and 20 % 16 and 20 > 16 and 5 % 4 and 5 > 4


CASES = [(h, w, st) for (h, w) in FRAMES for st in STAGES]


@pytest.mark.parametrize("h,w,stage", CASES, ids=["%dx%d-%s" % c for c in CASES])
def test_stage_against_float64(h, w, stage):
    r = _run(h, w)
    label = "%dx%d %s" % (h, w, stage)
    ref64, got, m = T._stage(r, stage, np.float64)
    ref32 = T._stage(r, stage, np.float32)[0]
    assert got.shape == ref64.shape and ref32.dtype == np.float32 and ref64.dtype == np.float64
    assert m == (T.M_SPLIT if stage == "x3" else T.M_FP32)
    if stage.startswith("pre"):
        T._judge(label + " proj", got[:8], ref64[:8], ref32[:8], m)
        T._judge(label + " S,H,V,D1,D2", got[8:], ref64[8:], ref32[8:], m)
        return
    T._judge(label, got, ref64, ref32, m)


def test_one_pixel_wide_level_clamps_every_right_neighbour():
    """1024 x 30: level 4 is one pixel wide, so g(x + 1) IS g(x): H = S and D1 = D2 = V, exactly."""
    pre4 = _run(1024, 30)["pre4"]
    assert pre4.shape == (13, 32, 1)
    np.testing.assert_array_equal(pre4[9], pre4[8])
    np.testing.assert_array_equal(pre4[11], pre4[10])
    np.testing.assert_array_equal(pre4[12], pre4[10])


def test_batch_of_three_frames_equals_the_single_frame_entry(gpu_ctx):
    """Three DIFFERENT frames of 1024 x 150 through one launch sequence: keypoints, descriptors, scores and counts of every frame,
    and frame 0's buffers 10..18, are the single-frame entry's bit for bit."""
    h, w, K = 1024, 150, MAX_KPTS
    sd = load_pkg("weights").random_aliked_state_dict(0)
    AL = load_pkg("aliked").AlikedHIP
    imgs = [frames.noise_frame(20 + i, h=h, w=w) for i in range(3)]
    Hp, Wp = S.dims(h, w)["Hp"], S.dims(h, w)["Wp"]
    single = AL(sd, max_num_keypoints=K, max_h=h, max_w=w, ctx=gpu_ctx)
    want = [single.extract(im, K, return_scores=True) for im in reversed(imgs)][::-1]          # (frame 0 last: its buffers stay)
    want_buf = _stage_buffers(single, Hp, Wp)
    single.close()
    al = AL(sd, max_num_keypoints=K, max_h=h, max_w=w, ctx=gpu_ctx, max_frames=3)
    dev = [gpu_ctx.upload(im) for im in imgs]
    xy = [gpu_ctx.malloc(K * 8) for _ in imgs]; de = [gpu_ctx.malloc(K * 512) for _ in imgs]
    sc = [gpu_ctx.malloc(K * 4) for _ in imgs]; nn = [gpu_ctx.malloc(16) for _ in imgs]
    al.extract_batch_dev(dev, h, w, 3, xy, de, sc, nn, K)
    gpu_ctx.sync()
    for i in range(3):
        n = np.empty(1, np.int32); gpu_ctx.d2h(n, nn[i])
        k = int(n[0])
        assert k == len(want[i][0]) > 50, (i, k, len(want[i][0]))
        a = np.empty((K, 2), np.float32); d = np.empty((K, 128), np.float32); s = np.empty(K, np.float32)
        gpu_ctx.d2h(a, xy[i]); gpu_ctx.d2h(d, de[i]); gpu_ctx.d2h(s, sc[i])
        np.testing.assert_array_equal(a[:k], want[i][0])
        np.testing.assert_array_equal(d[:k], want[i][1])
        np.testing.assert_array_equal(s[:k], want[i][2])
    got_buf = _stage_buffers(al, Hp, Wp)
    for which in want_buf:
        np.testing.assert_array_equal(got_buf[which], want_buf[which], err_msg="buffer %d" % which)
    for p in dev + xy + de + sc + nn:
        gpu_ctx.free(p)
    al.close()


def test_two_capacities_give_identical_stage_buffers(gpu_ctx):
    """The workspace stride between frames follows the instance's capacity, the stage buffers' contents must not: the same
    150 x 1024 frame on an instance made for it and on one made for 600 x 1300 images."""
    h, w, K = 150, 1024, MAX_KPTS
    sd = load_pkg("weights").random_aliked_state_dict(0)
    AL = load_pkg("aliked").AlikedHIP
    image = frames.noise_frame(30, h=h, w=w)
    Hp, Wp = S.dims(h, w)["Hp"], S.dims(h, w)["Wp"]
    got = []
    for mh, mw, mf in ((h, w, 1), (600, 1300, 2)):
        al = AL(sd, max_num_keypoints=K, max_h=mh, max_w=mw, ctx=gpu_ctx, max_frames=mf)
        out = al.extract(image, K, return_scores=True)
        got.append((out, _stage_buffers(al, Hp, Wp)))
        al.close()
    for x, y in zip(got[0][0], got[1][0]):
        np.testing.assert_array_equal(x, y)
    for which in got[0][1]:
        np.testing.assert_array_equal(got[0][1][which], got[1][1][which], err_msg="buffer %d" % which)
