"""ALIKED stage by stage: every stage of the extractor as a function of that stage's INPUT, in float64 or float32.  CPU only.

The float64 side is `oracle/aliked_ref.py` itself, its source evaluated with float32 -> float64 (`oracle(np.float64)`); the
float32 side is the module as it stands.  A stage function takes the stage's input as an array (what `debug_read` returned
from the GPU, or the previous stage's output) and returns the output of that ONE stage, so that errors do not compound and a
failure names the kernel.  Where the oracle has a function for the stage (`conv_block`, `res_block`, `dkd`, `sddh`,
`preprocess`) that function is called; the gates, the aggregation, the score tail and the descriptor half of `sddh` are lines
inside `extract_dense_map` / `sddh` there and are restated here - tests/test_aliked_stages.py chains these functions from the
oracle's own image and requires the oracle's own stage values to 1e-12, so a restatement cannot drift.

`err(got, want)` is max |got - want| / max |want|; `bar(m, err_ref)` is the acceptance rule of the stage tests:
err_gpu <= max(m * err_ref, 1e-6) with err_ref the float32 evaluation of the same function on the same input."""
import contextlib
import inspect
import types

import numpy as np
import torch

from oracle import aliked_ref as A32

_SRC = inspect.getsource(A32)
_TD = {np.float32: torch.float32, np.float64: torch.float64}
_MODS = {}


@contextlib.contextmanager
def default_dtype(dtype):
    """The oracle creates some tensors (`torch.linspace`, `.float()` free arithmetic) in torch's default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(_TD[dtype])
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def oracle(dtype=np.float64, edits=()):
    """The oracle module in `dtype`.  `edits`: (old, new) source replacements (the mutation tests); each must apply."""
    key = (dtype, tuple(edits))
    if key not in _MODS:
        src = _SRC
        for old, new in edits:
            assert src.count(old) >= 1, old
            src = src.replace(old, new)
        if dtype is np.float64:
            src = src.replace("torch.float32", "torch.float64").replace("np.float32", "np.float64")
        elif not edits:
            _MODS[key] = A32
            return A32
        mod = types.ModuleType("aliked_%s_%d" % (np.dtype(dtype).name, len(_MODS)))
        with default_dtype(dtype):
            exec(compile(src, mod.__name__, "exec"), mod.__dict__)
        _MODS[key] = mod
    return _MODS[key]


def extract(sd, image_u8, max_kpts, dtype=np.float64):
    """The whole oracle in `dtype` (return_debug=True)."""
    with default_dtype(dtype):
        return oracle(dtype).aliked_extract({k: np.asarray(v, dtype) for k, v in sd.items()}, image_u8, max_kpts, return_debug=True)


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype)))


def _sd(sd, dtype):
    return {k: _t(v, dtype) for k, v in sd.items()}


def err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


FLOOR = 1e-6


def bar(m, err_ref):
    return max(m * err_ref, FLOOR)


# --------------------------------------------------------------------------- #
#  geometry
# --------------------------------------------------------------------------- #
def dims(H, W):
    """Network size of an H x W image: dict(h, w, Hp, Wp, pl, pt, pr, pb)."""
    p = A32.resize_plan(H, W, A32.CFG["resize"])
    h, w = p["new_h"], p["new_w"]
    pl, pr, pt, pb = A32.pad_amounts(h, w)
    return dict(h=h, w=w, Hp=h + pt + pb, Wp=w + pl + pr, pl=pl, pt=pt, pr=pr, pb=pb)


# --------------------------------------------------------------------------- #
#  dense stages
# --------------------------------------------------------------------------- #
@torch.no_grad()
def padded_image(image_u8, dtype=np.float64, pad_mode="replicate"):
    """uint8 image -> the whole padded network input [3][Hp][Wp]."""
    M = oracle(dtype)
    with default_dtype(dtype):
        img, _ = M.preprocess(M.bgr_to_tensor(image_u8), M.CFG["resize"])
        pl, pr, pt, pb = M.pad_amounts(*img.shape[-2:])
        return M.F.pad(img, (pl, pr, pt, pb), mode=pad_mode)[0].numpy()


@torch.no_grad()
def block(sd, i, x, dtype=np.float64, M=None):
    """Block i (1..4) of its input map: img -> x1, x1 -> x2, x2 -> x3, x3 -> x4 (pooling included)."""
    M = M or oracle(dtype)
    s, x = _sd(sd, dtype), _t(x, dtype)[None]
    with default_dtype(dtype):
        if i == 1:
            return M.conv_block(s, "block1", x)[0].numpy()
        k = 2 if i == 2 else 4
        return M.res_block(s, "block%d" % i, M.F.avg_pool2d(x, k, k), i >= 3)[0].numpy()


@torch.no_grad()
def gate(sd, i, x, dtype=np.float64):
    """g_i = selu(conv1x1(x_i)), planar [32][H_i][W_i]."""
    M = oracle(dtype)
    return M.F.selu(M.F.conv2d(_t(x, dtype)[None], _t(sd["conv%d.weight" % i], dtype)))[0].numpy()


def pre_planes(sd, i, g, dtype=np.float64):
    """The 13 pre-aggregation planes of gated level i (2..4), [13][ih][iw]: proj[o] = sum_c Ws0[c][o] g_c (Ws0 = the level's 32
    rows of score_head.0.weight), then S = <g, g>, H = <g, g(x+1)>, V = <g, g(y+1)>, D1 = <g, g(x+1, y+1)>,
    D2 = <g(x+1), g(y+1)>, the right / lower neighbour clamped at the border."""
    g = np.asarray(g, dtype)
    ws0 = np.asarray(sd["score_head.0.weight"], dtype)[:, 32 * (i - 1):32 * i, 0, 0]            # [8][32]
    ih, iw = g.shape[1:]
    yd, xr = np.minimum(np.arange(ih) + 1, ih - 1), np.minimum(np.arange(iw) + 1, iw - 1)
    gr, gd, gdr = g[:, :, xr], g[:, yd, :], g[:, yd, :][:, :, xr]
    dot = lambda a, b: (a * b).sum(0, dtype=dtype)                                             # noqa: E731
    return np.concatenate([np.einsum("oc,cyx->oyx", ws0, g).astype(dtype),
                           np.stack([dot(g, g), dot(g, gr), dot(g, gd), dot(g, gdr), dot(gr, gd)])])


def norm2_from_planes(pre, Hp, Wp, drop_d2=False):
    """sum_c up(g_c)^2 at every pixel of the Hp x Wp map as the quadratic form in planes 8..12 (align_corners=True taps).
    `drop_d2`: without the D2 term - what the aggregate kernel once computed on 16 lanes."""
    pre = np.asarray(pre, np.float64)
    ih, iw = pre.shape[1:]
    fy, fx = np.arange(Hp) * ((ih - 1) / (Hp - 1)), np.arange(Wp) * ((iw - 1) / (Wp - 1))
    y0, x0 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    y1, x1 = np.minimum(y0 + 1, ih - 1), np.minimum(x0 + 1, iw - 1)
    ly, lx = (fy - y0)[:, None], (fx - x0)[None, :]
    w00, w01, w10, w11 = (1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx
    at = lambda p, yy, xx: pre[p][yy[:, None], xx[None, :]]                                     # noqa: E731
    S, Hh, V, D1, D2 = 8, 9, 10, 11, 12
    sq = w00 ** 2 * at(S, y0, x0) + w01 ** 2 * at(S, y0, x1) + w10 ** 2 * at(S, y1, x0) + w11 ** 2 * at(S, y1, x1)
    cr = w00 * w01 * at(Hh, y0, x0) + w10 * w11 * at(Hh, y1, x0) + w00 * w10 * at(V, y0, x0) + w01 * w11 * at(V, y0, x1) \
        + w00 * w11 * at(D1, y0, x0)
    if not drop_d2:
        cr = cr + w01 * w10 * at(D2, y0, x0)
    return sq + 2 * cr


@torch.no_grad()
def upsampled(g1, g2, g3, g4, dtype=np.float64, align_corners=True):
    """x1234 = cat(g1, up(g2, 2), up(g3, 8), up(g4, 32)), [128][Hp][Wp] (torch)."""
    M = oracle(dtype)
    up = lambda t, s: M.F.interpolate(_t(t, dtype)[None], scale_factor=s, mode="bilinear", align_corners=align_corners)  # noqa: E731
    return torch.cat([_t(g1, dtype)[None], up(g2, 2), up(g3, 8), up(g4, 32)], dim=1)


@torch.no_grad()
def aggregate(sd, g1, g2, g3, g4, dtype=np.float64, align_corners=True):
    """The gated levels (planar) -> (s8 [8][Hp][Wp] = selu(conv1x1(x1234, score_head.0)), rnorm [Hp][Wp] = 1 / max(|x1234|, 1e-12))."""
    M = oracle(dtype)
    x = upsampled(g1, g2, g3, g4, dtype, align_corners)
    s8 = M.F.selu(M.F.conv2d(x, _t(sd["score_head.0.weight"], dtype)))[0].numpy()
    rnorm = (1.0 / x.norm(p=2, dim=1).clamp_min(1e-12))[0].numpy()
    return s8, rnorm


@torch.no_grad()
def score_tail(sd, s8, d, dtype=np.float64):
    """s8 (whole padded map) -> score map [h][w]: the three 3 x 3 convs zero padded at the padded map's border, sigmoid, crop."""
    M = oracle(dtype)
    s = _t(s8, dtype)[None]
    s = M.F.selu(M.F.conv2d(s, _t(sd["score_head.2.weight"], dtype), padding=1))
    s = M.F.selu(M.F.conv2d(s, _t(sd["score_head.4.weight"], dtype), padding=1))
    s = torch.sigmoid(M.F.conv2d(s, _t(sd["score_head.6.weight"], dtype), padding=1))
    return s[0, 0, d["pt"]:d["pt"] + d["h"], d["pl"]:d["pl"] + d["w"]].numpy()


@torch.no_grad()
def feature_map(g1, g2, g3, g4, rnorm, d, dtype=np.float64):
    """The normalised, un-padded descriptor map [128][h][w] from the gated levels and a given 1 / |x1234| map."""
    x = upsampled(g1, g2, g3, g4, dtype)[0] * _t(rnorm, dtype)[None]
    return x[:, d["pt"]:d["pt"] + d["h"], d["pl"]:d["pl"] + d["w"]].numpy()


# --------------------------------------------------------------------------- #
#  sparse stages
# --------------------------------------------------------------------------- #
@torch.no_grad()
def refine(score, max_kpts, dtype=np.float64):
    """DKD on a given score map [h][w]: (kp_norm [n][2], keypoint scores [n], pixel indices [n])."""
    M = oracle(dtype)
    with default_dtype(dtype):
        kp, ks, idx = M.dkd(_t(score, dtype)[None, None].clone(), max_kpts)
    return kp.numpy(), ks.numpy(), idx.numpy()


PATCH_GUARD = 2.0 ** -11


@torch.no_grad()
def positions(sd, fmap, kp_norm, dtype=np.float64, M=None):
    """`sddh` up to the sample positions: (pos [n][16][2] in un-padded pixels, (x, y) of sample p; decided [n] bool).

    The 3 x 3 patch sits at `long(kwh)`, kwh = (kp / 2 + 0.5) * (w - 1, h - 1): a truncation.  Where kwh lies within
    PATCH_GUARD of an integer, which patch is read depends on the rounding of kwh itself (two float32 roundings at a
    magnitude up to 1024: 1.2e-4 < PATCH_GUARD) and no precision-independent answer exists; `decided` is False there."""
    M = M or oracle(dtype)
    f, kp = _t(fmap, dtype)[None], _t(kp_norm, dtype)
    with default_dtype(dtype):
        _, off = M.sddh(_sd(sd, dtype), f, kp, M.CFG["K"], M.CFG["M"])
    h, w = f.shape[-2:]
    kwh = (np.asarray(kp_norm, np.float64) / 2 + 0.5) * np.array([w - 1, h - 1], np.float64)
    decided = (np.abs(kwh - np.round(kwh)) > PATCH_GUARD).all(1)
    kwh_t = (kp / 2 + 0.5) * torch.tensor([[w - 1, h - 1]], dtype=_TD[dtype])
    return (kwh_t.unsqueeze(1) + off).numpy(), decided


@torch.no_grad()
def descriptors(sd, fmap, pos, dtype=np.float64):
    """Sample positions [n][16][2] (pixels) -> the returned descriptors [n][128]: grid_sample(align_corners=True, zeros),
    sf_conv, SELU, agg_weights, L2 normalise, then rows / (|row| + 1e-8) (what the drop-in returns)."""
    M = oracle(dtype)
    s, x, pos = _sd(sd, dtype), _t(fmap, dtype), _t(pos, dtype)
    c, h, w = x.shape
    n, m = pos.shape[:2]
    wh = torch.tensor([w - 1, h - 1], dtype=_TD[dtype])
    grid = (2.0 * pos / wh - 1).reshape(1, n * m, 1, 2)
    feats = M.F.grid_sample(x[None], grid, mode="bilinear", align_corners=True)
    feats = feats.reshape(c, n, m, 1).permute(1, 0, 2, 3)
    feats = M.F.selu(M.F.conv2d(feats, s["desc_head.sf_conv.weight"])).squeeze(-1)
    des = M.F.normalize(torch.einsum("ncp,pcd->nd", feats, s["desc_head.agg_weights"]), p=2.0, dim=1).numpy()
    return des / (np.linalg.norm(des, axis=1, keepdims=True) + 1e-8).astype(dtype)
