"""HIP ALIKED stage by stage against float64, at the thinnest legal frames.

Every stage of csrc/aliked_kernels.hip is compared with the float64 evaluation of THAT stage on the stage's own input as read
back from the GPU (tests/aliked_stages.py), so errors do not compound and a failure names the kernel.  Frames (noise, so that
score ties decide nothing) and what they reach:

    16 x 2048   network 8 x 1024 in 32 x 1024, pt = 12: the smallest legal height, 24 rows of padding, a 1/32 level one pixel
                high, 4 score rows inside the NMS border, fewer candidates than max_kpts (raster branch)
    20 x 640    32 x 1024, no padding: sy32 = 0
    24 x 640    38 x 1024 in 64 x 1024, pt = 13: a 2-row 1/32 level, odd padding
    100 x 1000  102 x 1024 in 128 x 1024: several row blocks per strip
    2048 x 16, 640 x 20, 640 x 24   the transposes, Wp = 32 or 64: a second 30-pixel strip of 2 pixels, 32-pixel deformable
                tiles with 1, 2 or 4 live pixels, 32 live lanes in the aggregate kernel, one NMS tile column

The bar.  With err(a) = max |a - float64| / max |float64| over the stage's output, err_gpu <= max(m * err_ref, 1e-6), where
err_ref is the error of the SAME helper function run in float32 on the same input (the reference's own rounding noise, not the
code under test) and
    m = 4   for the stages that are fp32 throughout (preprocess, gates, pre-aggregation, aggregation, score tail, DKD refine,
            patch gather, sample positions): other summation order, fmaf contraction, an expm1 of their own - a few roundings;
    m = 16  for the split-precision stages (block1..block4, descriptors): operands travel as fp16 (hi, lo) planes of ~22
            significant bits, up to 4 x the fp32 operand error on each of two operands;
the 1e-6 floor covers stages whose float32 reference happens to be exact.  The pre-aggregation planes are held to the bar in
two groups of their own scale (projections 0..7, inner products 8..12), which asks more than one bar over all 13.

Measured on the MI355X: err_gpu / err_ref per stage and frame (the larger of the two seeds), the largest err_gpu of the stage
and the largest err_gpu / bar.  No stage is over its margin; the aggregation (s8, rnorm) and the sample positions are MORE
accurate than the float32 reference, the split-precision blocks about as accurate, the descriptors 1.0 - 1.5 x its error.

    stage      16x2048  20x640  24x640 100x1000 2048x16  640x20  640x24   max err_gpu   max err_gpu / bar
    img           1.00    1.00    1.00    1.02    1.00    1.12    1.00    3.8e-06       0.25
    x1            0.68    0.64    0.60    0.63    0.70    0.65    0.62    4.9e-07       0.04
    x2            0.52    0.56    0.66    0.63    0.61    0.51    0.50    5.0e-07       0.04
    x3            1.23    1.00    0.96    1.01    1.00    0.89    0.94    2.5e-06       0.08
    x4            0.88    0.66    0.74    0.90    0.66    1.02    0.66    1.5e-06       0.06
    g1            1.00    1.00    1.00    1.00    1.00    1.00    1.00    3.1e-07       0.25
    g2            1.00    1.00    1.00    1.00    1.00    1.00    1.00    3.9e-07       0.25
    g3            0.82    0.67    0.81    0.78    0.84    0.78    0.92    3.2e-07       0.23
    g4            0.78    0.54    0.70    0.71    0.91    0.80    1.03    4.1e-07       0.26
    pre2 proj     1.19    0.97    1.13    0.94    0.97    0.99    0.95    3.2e-07       0.30
    pre2 S..D2    0.84    1.00    1.00    1.06    0.98    1.01    1.00    2.4e-07       0.23
    pre3 proj     0.98    1.22    1.04    1.00    1.00    1.10    1.00    3.1e-07       0.30
    pre3 S..D2    0.94    1.00    1.14    1.09    1.00    1.13    0.99    3.4e-07       0.25
    pre4 proj     1.00    1.13    1.21    0.87    1.13    1.33    1.00    3.1e-07       0.26
    pre4 S..D2    0.81    0.95    1.00    1.00    0.73    1.12    1.40    2.6e-07       0.23
    s8            0.24    0.21    0.16    0.17    0.11    0.12    0.08    1.2e-06       0.06
    rnorm         0.35    0.24    0.15    0.19    0.16    0.15    0.16    3.1e-07       0.09
    score         1.06    0.99    0.95    0.81    1.26    1.30    0.88    3.5e-07       0.27
    kp_norm       1.00    1.00    1.00    1.00    1.00    1.00    1.00    1.6e-07       0.16
    kp_score      1.00    1.00    1.00    1.00    1.00    1.00    1.00    7.7e-06       0.25
    patch         0.67    0.33    0.28    0.21    0.80    0.35    0.55    3.2e-06       0.20
    pos           0.53    0.51    0.52    0.52    0.52    0.51    0.52    3.3e-08       0.03
    desc          1.46    1.32    1.39    1.53    1.17    1.30    1.01    9.4e-06       0.10

The 3 x 3 patch of the descriptor head sits at a truncated coordinate; keypoints whose coordinate lies within 2^-11 of an
integer (where float32 and float64 may truncate differently, tests/aliked_stages.py) are left out of the patch / position
comparison and must be fewer than 2 %."""
import numpy as np
import pytest
import torch

import aliked_stages as S
import frames
from conftest import load_pkg
from oracle import aliked_ref as R

pytestmark = pytest.mark.gpu

MAX_KPTS = 1024
FRAMES = [(16, 2048), (20, 640), (24, 640), (100, 1000), (2048, 16), (640, 20), (640, 24)]
SEEDS = (0, 1)
M_FP32, M_SPLIT = 4, 16
STAGES = ["img", "x1", "x2", "x3", "x4", "g1", "g2", "g3", "g4", "pre2", "pre3", "pre4", "s8", "rnorm", "score", "dkd",
          "patch", "pos", "desc"]

_INST = {}
_RUN = {}


@pytest.fixture(scope="module", autouse=True)
def _release_instances():
    yield
    for al, _ in _INST.values():
        al.close()
    _INST.clear()
    _RUN.clear()


def _instance(h, w, seed):
    """One instance per orientation and weight set, kept for the module (wide: the 100-row frame has to fit too)."""
    wide = w >= h
    key = (wide, seed)
    if key not in _INST:
        sd = load_pkg("weights").random_aliked_state_dict(seed)
        mh, mw = (128, 2048) if wide else (2048, 32)
        _INST[key] = (load_pkg("aliked").AlikedHIP(sd, max_num_keypoints=MAX_KPTS, max_h=mh, max_w=mw), sd)
    return _INST[key]


def _dims(al):
    d = al.debug_read(2, (8,), np.int32)
    return dict(h=int(d[0]), w=int(d[1]), Hp=int(d[2]), Wp=int(d[3]), pl=int(d[4]), pt=int(d[5]), n_cand=int(d[6]), n_kp=int(d[7]))


def _run(h, w, seed):
    """One extraction and every stage buffer of it (the latest frame only is kept: the tests come frame by frame)."""
    key = (h, w, seed)
    if key in _RUN:
        return _RUN[key]
    _RUN.clear()
    al, sd = _instance(h, w, seed)
    image = frames.noise_frame(seed, h=h, w=w)
    xy, desc, sc = al.extract(image, MAX_KPTS, return_scores=True)
    d = _dims(al)
    want = S.dims(h, w)
    assert all(d[k] == want[k] for k in ("h", "w", "Hp", "Wp", "pl", "pt")), (d, want)
    Hp, Wp, n = d["Hp"], d["Wp"], len(xy)
    assert n == d["n_kp"] and n > 50
    r = dict(al=al, sd=sd, image=image, d=d, xy=xy, desc=desc, sc=sc, n=n)
    r["img"] = al.debug_read(7, (3, Hp, Wp))
    for which, name, div, ch in ((3, "x1", 1, 16), (4, "x2", 2, 32), (5, "x3", 8, 64), (6, "x4", 32, 128),
                                 (12, "g2", 2, 32), (13, "g3", 8, 32), (14, "g4", 32, 32),
                                 (15, "pre2", 2, 13), (16, "pre3", 8, 13), (17, "pre4", 32, 13), (18, "s8", 1, 8)):
        r[name] = al.debug_read(which, (ch, Hp // div, Wp // div))
    r["g1"] = np.ascontiguousarray(al.debug_read(10, (Hp, Wp, 32)).transpose(2, 0, 1))
    r["rnorm"] = al.debug_read(11, (Hp, Wp))
    r["score"] = al.debug_read(0, (d["h"], d["w"]))
    r["nms"] = al.debug_read(8, (d["h"], d["w"]))
    r["idx"] = al.debug_read(1, (n,), np.int32)
    r["kp"] = al.debug_read(9, (n, 2))
    r["pos"] = al.debug_read(19, (n, 16, 2))
    r["patch"] = al.debug_read(20, (n, 1152))
    r["x0"] = r["img"]
    for k, v in r.items():
        if isinstance(v, np.ndarray) and v.dtype == np.float32:
            assert np.isfinite(v).all(), k
    _RUN[key] = r
    return r


def _fmap(r, dtype):
    """The normalised un-padded map from the GPU's gated levels and the GPU's 1 / |F| (cached per run and dtype)."""
    k = ("fmap", dtype)
    if k not in r:
        r[k] = S.feature_map(r["g1"], r["g2"], r["g3"], r["g4"], r["rnorm"], r["d"], dtype)
    return r[k]


def _positions(r, dtype):
    k = ("pos", dtype)
    if k not in r:
        r[k] = S.positions(r["sd"], _fmap(r, dtype), r["kp"], dtype)
    return r[k]


def _patches(r, dtype):
    x = torch.from_numpy(_fmap(r, dtype))
    h, w = x.shape[1:]
    kwh = (torch.from_numpy(r["kp"].astype(dtype)) / 2 + 0.5) * torch.tensor([[w - 1, h - 1]], dtype=x.dtype)
    return S.oracle(dtype).get_patches(x, kwh.long(), 3).reshape(r["n"], 1152).numpy()                  # [n][c][y][x]


def _stage(r, name, dtype):
    """(reference output of stage `name` in `dtype` from the GPU's input of that stage, the GPU's output, margin)"""
    sd, d = r["sd"], r["d"]
    if name == "img":
        return S.padded_image(r["image"], dtype), r["img"], M_FP32
    if name in ("x1", "x2", "x3", "x4"):
        i = int(name[1])
        return S.block(sd, i, r["x%d" % (i - 1)], dtype), r[name], M_SPLIT
    if name in ("g1", "g2", "g3", "g4"):
        i = int(name[1])
        return S.gate(sd, i, r["x%d" % i], dtype), r[name], M_FP32
    if name in ("s8", "rnorm"):
        k = ("agg", dtype)
        if k not in r:
            r[k] = S.aggregate(sd, r["g1"], r["g2"], r["g3"], r["g4"], dtype)
        return r[k][name == "rnorm"], r[name], M_FP32
    if name.startswith("pre"):
        i = int(name[3])
        return S.pre_planes(sd, i, r["g%d" % i], dtype), r[name], M_FP32
    if name == "score":
        return S.score_tail(sd, r["s8"], d, dtype), r["score"], M_FP32
    dec = _positions(r, np.float64)[1]
    if name == "patch":
        return _patches(r, dtype)[dec], r["patch"][dec], M_FP32
    if name == "pos":
        return _positions(r, dtype)[0][dec], r["pos"][dec], M_FP32
    if name == "desc":
        return S.descriptors(sd, _fmap(r, dtype), r["pos"], dtype), r["desc"], M_SPLIT
    raise KeyError(name)


def _judge(label, got, ref64, ref32, m):
    e_gpu, e_ref = S.err(got, ref64), S.err(ref32, ref64)
    print("STAGE %-24s err_gpu %.3e err_ref %.3e ratio %7.2f bar %.3e" % (label, e_gpu, e_ref, e_gpu / max(e_ref, 1e-300), S.bar(m, e_ref)))
    assert e_gpu <= S.bar(m, e_ref), (label, e_gpu, e_ref, m)


CASES = [(h, w, seed, st) for (h, w) in FRAMES for seed in SEEDS for st in STAGES]


@pytest.mark.parametrize("h,w,seed,stage", CASES, ids=["%dx%d-s%d-%s" % c for c in CASES])
def test_stage_against_float64(h, w, seed, stage):
    r = _run(h, w, seed)
    label = "%dx%d s%d %s" % (h, w, seed, stage)
    if stage == "dkd":
        # the detector on the GPU's own score map: every discontinuous decision exactly (the stage-exact check of
        # tests/test_aliked_gpu.py::_check), the refined coordinates and scores to the bar
        sg = torch.from_numpy(r["score"].copy())[None, None]
        nms_o = R.simple_nms(sg, 2)[0, 0].numpy().copy()
        nms_o[:2] = 0; nms_o[-2:] = 0; nms_o[:, :2] = 0; nms_o[:, -2:] = 0
        np.testing.assert_array_equal(r["nms"], nms_o)
        kp_o, ks_o, idx_o = R.dkd(sg, MAX_KPTS)
        np.testing.assert_array_equal(r["idx"], idx_o.numpy())
        np.testing.assert_allclose(r["kp"], kp_o.numpy(), atol=2e-6)
        np.testing.assert_allclose(r["sc"], ks_o.numpy(), atol=1e-5)
        kp64, ks64, idx64 = S.refine(r["score"], MAX_KPTS)
        np.testing.assert_array_equal(idx64, idx_o.numpy())
        _judge(label + " kp_norm", r["kp"], kp64, kp_o.numpy(), M_FP32)
        _judge(label + " kp_score", r["sc"], ks64, ks_o.numpy(), M_FP32)
        return
    ref64, got, m = _stage(r, stage, np.float64)
    ref32 = _stage(r, stage, np.float32)[0]
    assert got.shape == ref64.shape and ref32.dtype == np.float32 and ref64.dtype == np.float64
    if stage in ("patch", "pos"):
        assert _positions(r, np.float64)[1].mean() > 0.98
    if stage.startswith("pre"):
        _judge(label + " proj", got[:8], ref64[:8], ref32[:8], m)
        _judge(label + " S,H,V,D1,D2", got[8:], ref64[8:], ref32[8:], m)
        return
    _judge(label, got, ref64, ref32, m)


def test_thinnest_frame_takes_the_raster_branch():
    """16 x 2048: fewer candidates than max_kpts, all kept in raster order; the outputs stay inside the image."""
    r = _run(16, 2048, 0)
    assert 0 < r["d"]["n_cand"] == r["n"] < MAX_KPTS
    assert np.all(np.diff(r["idx"]) > 0)
    ys = r["idx"] // r["d"]["w"]
    assert ys.min() >= 2 and ys.max() <= r["d"]["h"] - 3                          # 4 score rows inside the NMS border
    np.testing.assert_allclose(np.linalg.norm(r["desc"], axis=1), 1.0, atol=1e-5)
    assert r["xy"][:, 1].min() >= -0.5 and r["xy"][:, 1].max() <= 15.5


def test_refusal_just_past_the_smallest_height(native):
    """16 x 2064 resizes to 7 x 1024: refused before anything is launched (the workspace keeps the previous frame's score map and
    control block bit for bit), and the instance then extracts the 16 x 2048 frame with the same bits as before."""
    sd = load_pkg("weights").random_aliked_state_dict(0)
    al = load_pkg("aliked").AlikedHIP(sd, max_num_keypoints=MAX_KPTS, max_h=32, max_w=2112)
    img = frames.noise_frame(0, h=16, w=2048)
    a = al.extract(img, MAX_KPTS, return_scores=True)
    assert S.dims(16, 2064)["h"] == 7 and S.dims(16, 2048)["h"] == 8
    before = (al.debug_read(0, (7, 1024)), _dims(al)["n_kp"], _dims(al)["n_cand"], al.debug_read(9, (len(a[0]), 2)))
    with pytest.raises(native.NativeError, match="network size"):
        al.extract(frames.noise_frame(1, h=16, w=2064), MAX_KPTS)
    d = _dims(al)
    assert (d["h"], d["w"]) == (7, 1024)                                          # the refused frame's bookkeeping ...
    np.testing.assert_array_equal(al.debug_read(0, (7, 1024)), before[0])         # ... and nothing of it on the device
    assert (d["n_kp"], d["n_cand"]) == before[1:3]
    np.testing.assert_array_equal(al.debug_read(9, (len(a[0]), 2)), before[3])
    b = al.extract(img, MAX_KPTS, return_scores=True)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    al.close()


@pytest.mark.parametrize("h,w", [(20, 640), (640, 20)])
def test_batch_of_five_thin_frames_equals_the_single_frame_entry(gpu_ctx, h, w):
    """The row-block split of block1 / block2 and the descriptor GEMM's tile depend on the batch size F: five frames through
    one launch sequence give the single-frame entry's keypoints, descriptors, scores and counts bit for bit."""
    sd = load_pkg("weights").random_aliked_state_dict(0)
    AL = load_pkg("aliked").AlikedHIP
    K = MAX_KPTS
    imgs = [frames.noise_frame(10 + i, h=h, w=w) for i in range(5)]
    single = AL(sd, max_num_keypoints=K, max_h=h, max_w=w, ctx=gpu_ctx)
    want = [single.extract(im, K, return_scores=True) for im in imgs]
    single.close()
    al = AL(sd, max_num_keypoints=K, max_h=h, max_w=w, ctx=gpu_ctx, max_frames=5)
    dev = [gpu_ctx.upload(im) for im in imgs]
    xy = [gpu_ctx.malloc(K * 8) for _ in imgs]; de = [gpu_ctx.malloc(K * 512) for _ in imgs]
    sc = [gpu_ctx.malloc(K * 4) for _ in imgs]; nn = [gpu_ctx.malloc(16) for _ in imgs]
    al.extract_batch_dev(dev, h, w, 3, xy, de, sc, nn, K)
    gpu_ctx.sync()
    for i in range(5):
        n = np.empty(1, np.int32); gpu_ctx.d2h(n, nn[i])
        k = int(n[0])
        assert k == len(want[i][0]) > 50, (i, k, len(want[i][0]))
        a = np.empty((K, 2), np.float32); d = np.empty((K, 128), np.float32); s = np.empty(K, np.float32)
        gpu_ctx.d2h(a, xy[i]); gpu_ctx.d2h(d, de[i]); gpu_ctx.d2h(s, sc[i])
        np.testing.assert_array_equal(a[:k], want[i][0])
        np.testing.assert_array_equal(d[:k], want[i][1])
        np.testing.assert_array_equal(s[:k], want[i][2])
    for p in dev + xy + de + sc + nn:
        gpu_ctx.free(p)
    al.close()


def test_refused_frame_in_front_of_a_graph_capture(gpu_ctx, native):
    """With use_graphs on, a call that is not cached yet captures its launch sequence: the 16 x 2064 frame (network 7 x 1024) must
    be refused BEFORE that capture begins.  The instance then captures the 16 x 2048 frame and gives the keypoints, descriptors
    and scores of plain launches on a fresh instance bit for bit, and the second call - a replay - gives them again."""
    sd = load_pkg("weights").random_aliked_state_dict(0)
    AL = load_pkg("aliked").AlikedHIP
    K = MAX_KPTS
    dev = gpu_ctx.upload(frames.noise_frame(0, h=16, w=2048))
    bad = gpu_ctx.upload(frames.noise_frame(1, h=16, w=2064))
    xy, de, sc, nn = gpu_ctx.malloc(K * 8), gpu_ctx.malloc(K * 512), gpu_ctx.malloc(K * 4), gpu_ctx.malloc(16)

    def call(al, ptr, w):
        for p, nbytes in ((xy, K * 8), (de, K * 512), (sc, K * 4), (nn, 16)):
            gpu_ctx.memset_async(p, 0xff, nbytes)
        al.extract_dev(ptr, 16, w, 3, xy, de, sc, nn, K)
        gpu_ctx.sync()
        n = np.empty(1, np.int32); gpu_ctx.d2h(n, nn)
        a = np.empty((K, 2), np.float32); d = np.empty((K, 128), np.float32); s = np.empty(K, np.float32)
        gpu_ctx.d2h(a, xy); gpu_ctx.d2h(d, de); gpu_ctx.d2h(s, sc)
        k = int(n[0])
        return a[:k], d[:k], s[:k]

    plain = AL(sd, max_num_keypoints=K, max_h=16, max_w=2064, ctx=gpu_ctx)
    want = call(plain, dev, 2048)
    plain.close()
    assert 50 < len(want[0]) < K
    al = AL(sd, max_num_keypoints=K, max_h=16, max_w=2064, ctx=gpu_ctx)
    al.use_graphs(True)
    with pytest.raises(native.NativeError, match="network size 32x1024 outside"):
        call(al, bad, 2064)
    assert (_dims(al)["h"], _dims(al)["w"]) == (7, 1024)
    for _ in range(2):                                   # capture + launch, then a replay
        for x, y in zip(call(al, dev, 2048), want):
            np.testing.assert_array_equal(x, y)
    al.close()
    for p in (dev, bad, xy, de, sc, nn):
        gpu_ctx.free(p)
