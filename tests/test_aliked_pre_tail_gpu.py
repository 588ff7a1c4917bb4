"""The tiled pre-processing kernel and the register-blocked score tail of csrc/aliked_kernels.hip (al_preprocess_kernel,
al_score_tail_kernel) at the smallest frames at which their tiling can go wrong.  The padded image (debug_read 7) is compared
with the oracle's pre-processing + replicate pad at 1e-5 and the score map (debug_read 0) with the oracle's dense map at 1e-3,
the tolerances tests/test_aliked_gpu.py uses for the two stages.

What each frame is there for (network size h x w; pre-processing tiles are `pre_tw x pre_th` of al_plan.hpp's ladder, the
score tail's 32 x 8):
  16 x 2048        8 rows: the thinnest legal frame; downscale 2, three taps; pt = 12, the tail's tiles are mostly padding
  2048 x 16        8 columns: the same, the other way round (pl = 12)
  257 x 1024       no resize, no blur; 257 rows = 32 tiles + 1; pt = 15; the map is as wide as the padded one, so the tail's
                   zero padding at the padded-map border is what its left and right columns see
  1024 x 257 gray  C = 1; 257 columns = 8 tail tiles + 1 and 4.5 pre-processing tiles (a partial tile); pl = 15; zero padding at
                   the top and bottom rows
  300 x 1100 BGRA  C = 4; downscale 1.074: blur with three taps; pt = 4; source rows start at any byte offset mod 4 (W C = 4400
                   does, W C = 3072 and 257 do not)
  5120 x 80        downscale 5: nine taps, reflect border on both sides of a 16-pixel-wide map, i.e. narrower than twice the
                   radius plus a tile; the ladder picks 16 x 4 tiles here
  1080 x 1920      the largest frame the issue names (downscale 1.875), odd row length 5760 + the 64 x 8 tile at its widest span
  3072 x 96, 8192 x 128
                   downscales 3 and 8 (5 and 15 taps; 8192 is the longest side an instance takes): the ladder's 32 x 8 and 8 x 2
                   tiles, the last with fewer pixels than threads
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_pkg
from oracle import aliked_ref as R

pytestmark = pytest.mark.gpu

CASES = {
    "8_rows": (16, 2048, 3),
    "8_columns": (2048, 16, 3),
    "no_resize_257_rows": (257, 1024, 3),
    "gray_257_columns": (1024, 257, 1),
    "bgra_three_taps": (300, 1100, 4),
    "nine_taps_narrow": (5120, 80, 3),
    "full_hd": (1080, 1920, 3),
    "five_taps_32x8_tiles": (3072, 96, 3),
    "fifteen_taps_8x2_tiles": (8192, 128, 3),
}
EXPECT = {          # (h, w, pl, pt, blur, ky, kx): the case is what the docstring says it is
    "8_rows": (8, 1024, 0, 12, True, 3, 3),
    "8_columns": (1024, 8, 12, 0, True, 3, 3),
    "no_resize_257_rows": (257, 1024, 0, 15, False, 3, 3),
    "gray_257_columns": (1024, 257, 15, 0, False, 3, 3),
    "bgra_three_taps": (279, 1024, 0, 4, True, 3, 3),
    "nine_taps_narrow": (1024, 16, 8, 0, True, 9, 9),
    "full_hd": (576, 1024, 0, 0, True, 3, 3),
    "five_taps_32x8_tiles": (1024, 32, 0, 0, True, 5, 5),
    "fifteen_taps_8x2_tiles": (1024, 16, 8, 0, True, 15, 15),
}


@pytest.fixture(scope="module")
def W():
    return load_pkg("weights")


@pytest.fixture(scope="module")
def AL():
    return load_pkg("aliked").AlikedHIP


def _image(name):
    H, Wd, C = CASES[name]
    rng = np.random.default_rng(list(CASES).index(name))
    # smooth structure + noise: blur and resize have something to average, and every byte value occurs
    yy, xx = np.mgrid[0:H, 0:Wd].astype(np.float32)
    base = 127.0 + 90.0 * np.sin(xx / 7.0 + yy / 11.0)
    img = base[:, :, None] + rng.normal(0.0, 35.0, (H, Wd, max(C, 1)))
    img = np.clip(img, 0, 255).astype(np.uint8)
    if C == 4:
        img[:, :, 3] = rng.integers(0, 256, (H, Wd), dtype=np.uint8)      # alpha must not leak into a channel
    return np.ascontiguousarray(img[:, :, 0] if C == 1 else img)


def _oracle(sd, img):
    x, _ = R.preprocess(R.bgr_to_tensor(img))
    h, w = x.shape[-2:]
    pl, pr, pt, pb = R.pad_amounts(h, w)
    padded = F.pad(x, (pl, pr, pt, pb), mode="replicate")[0].numpy()
    sdt = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in sd.items()}
    with torch.no_grad():
        _, score = R.extract_dense_map(sdt, x)
    return padded, score[0, 0].numpy(), (h, w, pl, pt)


@pytest.mark.parametrize("name", list(CASES))
def test_padded_image_and_score_map_against_the_oracle(W, AL, name):
    H, Wd, C = CASES[name]
    sd = W.random_aliked_state_dict(0)
    img = _image(name)
    plan = R.resize_plan(H, Wd)
    padded, score, (h, w, pl, pt) = _oracle(sd, img)
    assert (h, w, pl, pt, plan["blur"], plan["ky"], plan["kx"]) == EXPECT[name]
    al = AL(sd, max_num_keypoints=256, max_h=H, max_w=Wd)
    al.extract(img, 256)
    d = al.debug_read(2, (8,), np.int32)
    assert tuple(int(v) for v in d[:6]) == (h, w) + padded.shape[1:] + (pl, pt)
    img_g = al.debug_read(7, padded.shape)
    score_g = al.debug_read(0, (h, w))
    al.close()
    err_i, err_s = np.abs(img_g - padded).max(), np.abs(score_g - score).max()
    print(f"{name}: padded image max |err| {err_i:.3g}, score map max |err| {err_s:.3g}")
    np.testing.assert_allclose(img_g, padded, atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(score_g, score, atol=1e-3, rtol=1e-3)


def test_a_frame_alone_equals_the_frame_inside_a_batch_of_three(W, AL, gpu_ctx):
    """F = 1 against the same frame inside an F = 3 batch, bit for bit: the stage buffers of the batch's frame 0 (the debug hook
    reads that frame) and the outputs of every slot - the frame also sits in slot 2, behind another frame."""
    H, Wd, K = 300, 1100, 512
    sd = W.random_aliked_state_dict(0)
    a, b = _image("bgra_three_taps")[:, :, :3].copy(), _image("bgra_three_taps")[::-1, ::-1, :3].copy()
    single = AL(sd, max_num_keypoints=K, max_h=H, max_w=Wd, ctx=gpu_ctx)
    want_b = single.extract(b, K, return_scores=True)
    want_a = single.extract(a, K, return_scores=True)
    d = single.debug_read(2, (8,), np.int32)
    h, w, Hp, Wp = (int(v) for v in d[:4])
    img_1, score_1 = single.debug_read(7, (3, Hp, Wp)), single.debug_read(0, (h, w))
    single.close()
    al = AL(sd, max_num_keypoints=K, max_h=H, max_w=Wd, ctx=gpu_ctx, max_frames=3)
    dev = [gpu_ctx.upload(a), gpu_ctx.upload(b)]
    xy = [gpu_ctx.malloc(K * 8) for _ in range(3)]; de = [gpu_ctx.malloc(K * 512) for _ in range(3)]
    sc = [gpu_ctx.malloc(K * 4) for _ in range(3)]; nn = [gpu_ctx.malloc(16) for _ in range(3)]
    al.extract_batch_dev([dev[0], dev[1], dev[0]], H, Wd, 3, xy, de, sc, nn, K)
    gpu_ctx.sync()
    np.testing.assert_array_equal(al.debug_read(7, (3, Hp, Wp)), img_1)
    np.testing.assert_array_equal(al.debug_read(0, (h, w)), score_1)
    for slot, want in enumerate((want_a, want_b, want_a)):
        n = np.empty(1, np.int32); gpu_ctx.d2h(n, nn[slot])
        k = int(n[0])
        assert k == len(want[0]) > 0
        o_xy = np.empty((K, 2), np.float32); o_de = np.empty((K, 128), np.float32); o_sc = np.empty(K, np.float32)
        gpu_ctx.d2h(o_xy, xy[slot]); gpu_ctx.d2h(o_de, de[slot]); gpu_ctx.d2h(o_sc, sc[slot])
        np.testing.assert_array_equal(o_xy[:k], want[0])
        np.testing.assert_array_equal(o_de[:k], want[1])
        np.testing.assert_array_equal(o_sc[:k], want[2])
    for p in dev + xy + de + sc + nn:
        gpu_ctx.free(p)
    al.close()
