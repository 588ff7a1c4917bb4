"""ORB on the GPU (csrc/orb_kernels.hip through orb.py) against the restatement tests/orb_ref.py: every stage through
sslam_orb_stage_read and the outputs end to end, identical - integers, float32 bits and descriptor bytes - and in the defined
order.  Shapes are small: what can go wrong is at edges (odd sides, strides that are no multiple of 4, frames thinner than a
tile, levels too small for a keypoint, an edge threshold that reads the stored border), not at size."""
import ctypes as C

import numpy as np
import pytest

import orb_ref as R
import orb_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAXH, MAXW = 128, 160


def make(gpu_ctx, max_h=MAXH, max_w=MAXW, **kw):
    O = load_pkg("orb")
    names = dict(nfeatures=500, scaleFactor=1.2, nlevels=8, edgeThreshold=31, scoreType=0, fastThreshold=20)
    names.update(kw)
    pattern = names.pop("pattern", None)
    return O.ORB_create(names["nfeatures"], names["scaleFactor"], names["nlevels"], names["edgeThreshold"], 0, 2, names["scoreType"],
                        31, names["fastThreshold"], pattern=pattern, max_h=max_h, max_w=max_w, ctx=gpu_ctx)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_output(got, ref):
    xy, aux, desc = got
    assert len(xy) == len(ref["xy"]), (len(xy), len(ref["xy"]))
    assert xy.dtype == np.float32 and aux.dtype == np.float32 and desc.dtype == np.uint8
    assert xy.shape == (len(xy), 2) and aux.shape == (len(xy), 4) and desc.shape == (len(xy), 32)
    np.testing.assert_array_equal(bits(xy), bits(ref["xy"]))
    np.testing.assert_array_equal(bits(aux), bits(ref["aux"]))
    np.testing.assert_array_equal(desc, ref["desc"])


def assert_defined_order(aux, xy):
    """level ascending, then response descending, then y, then x"""
    key = list(zip(aux[:, 3].tolist(), (-aux[:, 2].astype(np.float64)).tolist(), xy[:, 1].tolist(), xy[:, 0].tolist()))
    assert key == sorted(key)


def test_every_stage_of_every_level_equals_the_restatement(gpu_ctx):
    kw = dict(nfeatures=12, nlevels=3)
    ref = S.reference("mosaic", **kw)
    o = make(gpu_ctx, **kw)
    o.detect_arrays(S.image("mosaic"))
    assert ref["sizes"][0] == (S.W, S.H) and (S.W + 2 * ref["border"]) % 4 != 0
    for lv, want in enumerate(ref["levels"]):
        info = o.level_info(lv)
        assert (info["w"], info["h"], info["border"], info["quota"]) == (want["w"], want["h"], ref["border"], ref["quotas"][lv])
        got = o.stage_read(lv)
        np.testing.assert_array_equal(got["img"], want["img"], err_msg=f"level {lv} with its border")
        np.testing.assert_array_equal(got["blur"], want["blur"], err_msg=f"blurred level {lv} with its border")
        assert len(got["cand"]) == len(want["cand"]) <= info["cand_cap"]
        g = {(x, y): (s, r) for (x, y, s), r in zip(got["cand"].tolist(), got["resp"].view(np.uint32).tolist())}
        assert len(g) == len(got["cand"])                                    # no candidate twice
        for (x, y, s), live, r in zip(want["cand"].tolist(), want["live"], bits(want["resp"]).tolist()):
            assert (x, y) in g and g[(x, y)][0] == s, (lv, x, y)
            if live:
                assert g[(x, y)][1] == r, (lv, x, y)
            else:
                assert np.isnan(np.uint32(g[(x, y)][1]).view(np.float32))     # dropped by the first cut
        assert got["cut1"] == want["cut1"]
        assert bits(got["cut2"]) == bits(want["cut2"])
    o.close()


CASES = {
    "no_cut_binds": ("mosaic", dict(nfeatures=5000, nlevels=3)),
    "both_cuts_bind": ("mosaic", dict(nfeatures=12, nlevels=3)),
    "ties_exceed_nfeatures": ("tiles", dict(nfeatures=12, nlevels=3)),
    "ties_one_level": ("tiles", dict(nfeatures=4, nlevels=1)),
    "fast_score": ("mosaic", dict(nfeatures=12, nlevels=3, scoreType=1)),
    "fast_score_ties": ("tiles", dict(nfeatures=12, nlevels=3, scoreType=1)),
    "fast_score_no_cut": ("mosaic", dict(nfeatures=5000, nlevels=3, scoreType=1)),
    "threshold_5": ("mosaic", dict(nfeatures=60, nlevels=3, fastThreshold=5)),
    "threshold_60": ("mosaic", dict(nfeatures=5000, nlevels=3, fastThreshold=60)),
    "edge_3_reads_the_border": ("mosaic", dict(nfeatures=5000, nlevels=3, edgeThreshold=3, fastThreshold=30)),
    "edge_3_cuts": ("mosaic", dict(nfeatures=100, nlevels=4, edgeThreshold=3)),
    "scale_2": ("mosaic", dict(nfeatures=5000, nlevels=2, scaleFactor=2.0, edgeThreshold=10)),
    "scale_1_05": ("mosaic", dict(nfeatures=200, nlevels=6, scaleFactor=1.05)),
}


def test_the_cases_bind_the_cuts_they_are_named_for():
    def levels(name):
        scene, kw = CASES[name]
        return [lv for lv in S.reference(scene, **kw)["levels"] if lv is not None], S.reference(scene, **kw), kw
    lv, ref, kw = levels("no_cut_binds")
    assert all(l["cut1"] == 0 and np.isneginf(l["cut2"]) for l in lv) and len(ref["xy"]) > 100
    lv, ref, kw = levels("both_cuts_bind")
    assert all(l["cut1"] > 0 and l["live"].sum() < len(l["cand"]) for l in lv[:2])
    assert all(np.isfinite(l["cut2"]) and l["keep"].sum() < l["live"].sum() for l in lv)
    lv, ref, kw = levels("ties_exceed_nfeatures")
    assert len(ref["xy"]) > kw["nfeatures"]
    lv, ref, kw = levels("ties_one_level")
    assert lv[0]["cut1"] > 0 and np.isfinite(lv[0]["cut2"]) and len(ref["xy"]) > kw["nfeatures"]
    lv, ref, kw = levels("edge_3_reads_the_border")
    assert min(ref["xy"][:, 0].min(), ref["xy"][:, 1].min()) < 15             # a disc and taps that leave the interior


@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end_equals_the_restatement_in_the_defined_order(gpu_ctx, name):
    scene, kw = CASES[name]
    o = make(gpu_ctx, **kw)
    got = o.detect_arrays(S.image(scene))
    assert_same_output(got, S.reference(scene, **kw))
    assert len(got[0]) > 0
    assert_defined_order(got[1], got[0])
    assert len(got[0]) <= o.capacity
    o.close()


@pytest.mark.parametrize("kw", [dict(nfeatures=5000, nlevels=3), dict(nfeatures=12, nlevels=3)], ids=["no_cut", "cuts"])
def test_three_channel_input_goes_through_the_fixed_point_grey(gpu_ctx, kw):
    o = make(gpu_ctx, **kw)
    ref = S.reference("mosaic3", **kw)
    assert_same_output(o.detect_arrays(S.image("mosaic3")), ref)
    # BGRA: the fourth channel is ignored, whatever it holds
    alpha = np.random.default_rng(4).integers(0, 256, S.image("mosaic3").shape[:2] + (1,), dtype=np.uint8)
    assert_same_output(o.detect_arrays(np.concatenate([S.image("mosaic3"), alpha], axis=2)), ref)
    assert not np.array_equal(R.gray(S.image("mosaic3")), S.image("mosaic3")[..., 1])
    o.close()


def test_levels_too_small_for_a_keypoint_give_nothing_and_change_nothing(gpu_ctx):
    """80 x 100 with 8 levels and edgeThreshold 31: levels 0 and 1 only have both sides >= 63"""
    kw8 = dict(nfeatures=300, nlevels=8)
    ref = S.reference("mosaic", 80, 100, **kw8)
    stored = [lv is not None for lv in ref["levels"]]
    assert stored == [True, True] + [False] * 6
    o = make(gpu_ctx, **kw8)
    got = o.detect_arrays(S.image("mosaic", 80, 100))
    assert_same_output(got, ref)
    assert len(got[0]) > 0 and set(got[1][:, 3].tolist()) <= {0.0, 1.0}
    assert [o.level_info(lv)["stored"] for lv in range(8)] == [1, 1, 0, 0, 0, 0, 0, 0]
    # the stored levels are what they are without the empty ones behind them
    for lv in (0, 1):
        np.testing.assert_array_equal(o.stage_read(lv)["img"], ref["levels"][lv]["img"])
    # an image with no level that can hold a keypoint: nothing, and no error
    assert len(o.detect_arrays(S.image("mosaic", 40, 50))[0]) == 0
    o.close()


@pytest.mark.parametrize("h,w,levels", [(64, 400, 4), (400, 64, 4), (23, 300, 2), (300, 23, 2)])
def test_a_frame_thinner_than_a_tile_in_one_direction(gpu_ctx, h, w, levels):
    """64: two tile columns and a level chain that ends below one; 23: thinner than the 32-pixel tile from level 0 on"""
    kw = dict(nfeatures=150, nlevels=4, edgeThreshold=8)
    o = make(gpu_ctx, max_h=400, max_w=400, **kw)
    got = o.detect_arrays(S.image("mosaic", h, w))
    assert_same_output(got, S.reference("mosaic", h, w, **kw))
    assert len(set(got[1][:, 3].tolist())) == levels
    o.close()


def test_a_constant_image_gives_nothing(gpu_ctx):
    o = make(gpu_ctx, nlevels=3)
    xy, aux, desc = o.detect_arrays(S.image("constant"))
    assert (len(xy), len(aux), len(desc)) == (0, 0, 0)
    assert o.detectAndCompute(S.image("constant"), None) == ([], None)
    o.close()


def test_detect_and_compute_returns_keypoints_with_every_field(gpu_ctx):
    types = load_pkg("slam.core.types")
    kw = dict(nfeatures=12, nlevels=3)
    o = make(gpu_ctx, **kw)
    ref = S.reference("mosaic", **kw)
    kps, desc = o.detectAndCompute(S.image("mosaic"))
    assert len(kps) == len(ref["xy"]) and all(isinstance(k, types.KeyPoint) for k in kps)
    np.testing.assert_array_equal(desc, ref["desc"])
    for k, (x, y), (size, angle, resp, octave) in zip(kps, ref["xy"].tolist(), ref["aux"].tolist()):
        assert (k.pt, k.size, k.angle, k.response, k.octave, k.class_id) == ((x, y), size, angle, resp, int(octave), -1)
    o.close()


def test_a_user_pattern_is_honoured(gpu_ctx):
    rng = np.random.default_rng(3)
    pattern = rng.integers(-15, 16, (512, 2)).astype(np.int8)
    kw = dict(nfeatures=40, nlevels=2)
    o = make(gpu_ctx, pattern=pattern, **kw)
    xy, aux, desc = o.detect_arrays(S.image("mosaic"))
    ref_user, ref_default = R.detect(S.image("mosaic"), pattern=pattern, **kw), S.reference("mosaic", **kw)
    assert_same_output((xy, aux, desc), ref_user)
    np.testing.assert_array_equal(bits(xy), bits(ref_default["xy"]))         # the same keypoints ...
    assert (desc != ref_default["desc"]).any(axis=1).all()                   # ... and other descriptors, every one
    np.testing.assert_array_equal(load_pkg("orb").default_pattern(), R.default_pattern())
    o.close()


def test_one_instance_keeps_no_residue_and_repeats_itself(gpu_ctx):
    kw = dict(nfeatures=60, nlevels=3)
    o = make(gpu_ctx, **kw)
    a1 = o.detect_arrays(S.image("mosaic"))
    b = o.detect_arrays(S.image("tiles"))                                    # another image, fewer keypoints
    c = o.detect_arrays(S.image("mosaic", 80, 100))                          # another size, fewer levels
    a2 = o.detect_arrays(S.image("mosaic"))
    assert_same_output(a1, S.reference("mosaic", **kw))
    assert_same_output(b, S.reference("tiles", **kw))
    assert_same_output(c, S.reference("mosaic", 80, 100, **kw))
    for x, y in zip(a1, a2):
        assert x.tobytes() == y.tobytes()
    o.close()


def test_two_instances_of_different_capacity_alternate_on_one_context(gpu_ctx):
    """An instance lays its memory out from its own capacities.  Two of them (another frame bound, nfeatures and level count:
    every piece of the two differs in size) alive on one context and called in turn return, each, bit for bit what it returns
    alone on a fresh context - which is the restatement's.  A pointer left from the measuring pass, a piece sized in another
    unit than its pointer's, or two pieces that overlap would show here."""
    native = load_pkg("_native")
    specs = [(dict(max_h=MAXH, max_w=MAXW), dict(nfeatures=60, nlevels=3), ()),          # (the frame at its default size)
             (dict(max_h=80, max_w=100), dict(nfeatures=300, nlevels=8), (80, 100))]    # two stored levels of eight
    alone = []
    for cap, kw, size in specs:
        ctx = native.Context(0)
        o = make(ctx, **cap, **kw)
        alone.append(o.detect_arrays(S.image("mosaic", *size)))
        o.close(); ctx.close()
        assert_same_output(alone[-1], S.reference("mosaic", *size, **kw))
        assert len(set(alone[-1][1][:, 3].tolist())) > 1                     # keypoints on more than one level
    both = [make(gpu_ctx, **cap, **kw) for cap, kw, _ in specs]
    for _ in range(2):                                                       # (the first call creates the native instance)
        for o, (_, _, size), want in zip(both, specs, alone):
            for x, y in zip(o.detect_arrays(S.image("mosaic", *size)), want):
                assert x.tobytes() == y.tobytes()
    assert both[0].capacity != both[1].capacity
    for o in both:
        o.close()


def test_the_device_entry_and_the_chain_into_the_matcher_and_the_f_filter(gpu_ctx):
    """ORB -> sslam_bf_match_dev (device counts) -> sslam_fmat_ransac_dev on a shifted pair, nothing read back in between,
    equals the same chain fed from host arrays."""
    B, E, native = load_pkg("bf_matcher"), load_pkg("epipolar"), load_pkg("_native")
    img0, img1 = S.shifted_pair()
    kw = dict(nfeatures=5000, nlevels=1, edgeThreshold=16)
    o = make(gpu_ctx, max_h=376, max_w=1241, **kw)                         # the benchmark's frame size as the instance's bound
    host = [o.detect_arrays(im) for im in (img0, img1)]
    cap, rows = o.capacity, o.chain_rows
    assert min(len(host[0][0]), len(host[1][0])) >= 30 and cap > 65536 == rows == B.MAX_ROWS
    ctx = gpu_ctx
    dev = []
    for im in (img0, img1):
        d = dict(img=ctx.upload(im), xy=ctx.malloc(cap * 8), aux=ctx.malloc(cap * 16), desc=ctx.malloc(cap * 32), n=ctx.malloc(4))
        o.detect_dev(d["img"], im.shape[0], im.shape[1], 1, d["xy"], d["aux"], d["desc"], d["n"])
        dev.append(d)
    m = B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=ctx)
    ij_dev, dist_dev, info_dev = ctx.malloc(cap * 8), ctx.malloc(cap * 4), ctx.malloc(16)
    # the ORB arrays hold `capacity` rows; the matcher and the filter are given min(capacity, 65 536) of them as their bound
    m.match_dev(ctx, 32, dev[0]["desc"], rows, dev[1]["desc"], rows, ij_dev, dist_dev, info_dev, m_dev=dev[0]["n"], n_dev=dev[1]["n"])
    kept_dev, finfo_dev, mask_dev = ctx.malloc(cap * 8), ctx.malloc(16), ctx.malloc(cap)
    E.filter_matches_dev(ctx, rows, info_dev, dev[0]["xy"], dev[1]["xy"], ij_dev, kept_dev, finfo_dev, thresh=1.0, mask_out_dev=mask_dev)
    ctx.sync()
    # the device entry's outputs and count are the host entry's
    for d, (xy, aux, desc) in zip(dev, host):
        n = np.zeros(1, np.int32); ctx.d2h(n, d["n"])
        assert n[0] == len(xy)
        for name, want in (("xy", xy), ("aux", aux), ("desc", desc)):
            got = np.empty_like(want); ctx.d2h(got, d[name])
            assert got.tobytes() == want.tobytes(), name
    # the chain from host arrays
    ij, dist = m.match_arrays(host[0][2], host[1][2])
    info = np.zeros(4, np.int32); ctx.d2h(info, info_dev)
    assert info.tolist() == [len(ij), len(host[0][0]), len(host[1][0]), 0] and len(ij) >= 20
    got_ij = np.empty_like(ij); ctx.d2h(got_ij, ij_dev)
    np.testing.assert_array_equal(got_ij, ij)
    # most mutual pairs are the shift (7, 4): identical descriptors inside the common region
    d = host[0][0][ij[:, 0]] - host[1][0][ij[:, 1]]
    assert (np.abs(d - np.array([7, 4], np.float32)).max(axis=1) == 0).mean() > 0.8
    finfo = np.zeros(4, np.int32); ctx.d2h(finfo, finfo_dev)
    ctx2 = native.Context(0)                                               # (the host chain on a context of its own)
    ij_pad = np.zeros((rows, 2), np.int32); ij_pad[:len(ij)] = ij
    ij_h = ctx2.upload(ij_pad); n_h = ctx2.upload(np.array([len(ij)], np.int32)); xy0_h = ctx2.upload(host[0][0]); xy1_h = ctx2.upload(host[1][0])
    kept_h, finfo_h, mask_h = ctx2.malloc(cap * 8), ctx2.malloc(16), ctx2.malloc(cap)
    E.filter_matches_dev(ctx2, rows, n_h, xy0_h, xy1_h, ij_h, kept_h, finfo_h, thresh=1.0, mask_out_dev=mask_h)
    ctx2.sync()
    finfo2 = np.zeros(4, np.int32); ctx2.d2h(finfo2, finfo_h)
    assert finfo.tolist() == finfo2.tolist()
    kept = max(int(finfo[0]), 0)
    a, b = np.empty((kept, 2), np.int32), np.empty((kept, 2), np.int32)
    if kept:
        ctx.d2h(a, kept_dev); ctx2.d2h(b, kept_h)
    np.testing.assert_array_equal(a, b)
    ctx2.close()
    o.close()


def test_the_c_entries_refuse_with_a_status_and_a_message_and_launch_nothing(gpu_ctx):
    native = load_pkg("_native")
    lib = native.lib()
    h = C.c_void_p()

    def create(**kw):
        a = dict(max_w=64, max_h=64, nfeatures=10, sf=1.2, nlevels=2, edge=8, score=0, fast=20, pattern=None)
        a.update(kw)
        return lib.sslam_orb_create(gpu_ctx.handle, a["max_w"], a["max_h"], a["nfeatures"], a["sf"], a["nlevels"], a["edge"], a["score"],
                                    a["fast"], native.ptr(a["pattern"]), C.byref(h))
    bad = np.zeros((512, 2), np.int8); bad[100, 1] = 16
    for kw, word in ((dict(nfeatures=0), "nfeatures"), (dict(sf=1.0), "scaleFactor"), (dict(sf=2.5), "scaleFactor"), (dict(nlevels=0), "nlevels"),
                     (dict(nlevels=17), "nlevels"), (dict(edge=2), "edgeThreshold"), (dict(score=2), "scoreType"), (dict(fast=0), "fastThreshold"),
                     (dict(fast=255), "fastThreshold"), (dict(max_w=0), "frame size"), (dict(pattern=bad), "pattern point 100")):
        assert create(**kw) != 0 and h.value is None
        assert word in lib.sslam_last_error().decode(), (kw, lib.sslam_last_error())
    assert create() == 0
    img = np.zeros((65, 64), np.uint8)
    out = [np.full((64, 2), 7, np.float32), np.full((64, 4), 7, np.float32), np.full((64, 32), 7, np.uint8)]
    n = C.c_int32(-7)
    P = native.ptr
    assert lib.sslam_orb_detect_host(h, P(img), 65, 64, 1, P(out[0]), P(out[1]), P(out[2]), C.byref(n)) != 0
    assert "larger than the instance's 64x64" in lib.sslam_last_error().decode()
    assert lib.sslam_orb_detect_host(h, P(img), 64, 64, 2, P(out[0]), P(out[1]), P(out[2]), C.byref(n)) != 0
    assert "2 channels" in lib.sslam_last_error().decode()
    assert lib.sslam_orb_detect_dev(h, P(img), 64, 65, 1, P(out[0]), P(out[1]), P(out[2]), C.byref(n)) != 0
    assert n.value == -7 and all((o == 7).all() for o in out)               # nothing was written
    assert lib.sslam_orb_level_info(h, 0, P(np.zeros(8, np.int32))) != 0    # ... and no frame was planned
    assert lib.sslam_orb_destroy(h) == 0
