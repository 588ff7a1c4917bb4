"""AKAZE on the GPU (csrc/akaze_kernels.hip through akaze.py) against the restatement tests/akaze_ref.py: every level's Lt, Lflow,
Lx, Ly and Ldet, kcontrast per octave, the candidate and survivor sets, the refined records with their angles through
sslam_akaze_stage_read, and the outputs end to end - identical integers, float32 bits and descriptor bytes, in the defined
order; no tolerance anywhere.  Shapes are the smallest at which each structure exists (tests/akaze_scenes.py): levels above
and below the one-workgroup bound, odd sides, the octave cut on either side."""
import numpy as np
import pytest

import akaze_ref as R
import akaze_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAXH, MAXW = 330, 650


def make(gpu_ctx, max_h=MAXH, max_w=MAXW, **kw):
    return load_pkg("akaze").AKAZE_create(max_h=max_h, max_w=max_w, ctx=gpu_ctx, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_output(got, ref):
    xy, aux, lvl, desc = got
    n = len(ref["xy"])
    assert len(xy) == n, (len(xy), n)
    assert xy.dtype == np.float32 and aux.dtype == np.float32 and lvl.dtype == np.int32 and desc.dtype == np.uint8
    assert xy.shape == (n, 2) and aux.shape == (n, 3) and lvl.shape == (n, 2) and desc.shape == (n, 61)
    np.testing.assert_array_equal(lvl, ref["lvl"])
    np.testing.assert_array_equal(bits(xy), bits(ref["xy"]))
    np.testing.assert_array_equal(bits(aux), bits(ref["aux"]))
    np.testing.assert_array_equal(desc, ref["desc"])


STAGES = ["one_octave", "two_octaves", "cut_160x80", "three_octaves", "four_octaves_defaults", "layers_5", "tiles", "three_channels"]


@pytest.mark.parametrize("name", STAGES)
def test_every_stage_of_every_level_equals_the_restatement(gpu_ctx, name):
    scene, h, w, kw = S.CASES[name]
    ref = S.reference(scene, h, w, **kw)
    o = make(gpu_ctx, **kw)
    o.detect_arrays(S.image(scene, h, w))
    lv = ref["levels"]
    got, forms = None, set()
    for i, (L, P) in enumerate(zip(lv, ref["planes"])):
        info = o.level_info(i)
        assert (info["w"], info["h"], info["levels"], info["octave"], info["sigma_size"], info["border"]) == \
            (L["w"], L["h"], len(lv), L["octave"], L["sigma_size"], L["border"])
        assert info["one_workgroup"] == int(i > 0 and L["w"] * L["h"] <= R.WG_PIXELS)
        forms.add((info["one_workgroup"], i > 0))
        got = o.stage_read(i)
        if i == 0:
            np.testing.assert_array_equal(bits(got["kcontrast"]), bits(ref["kcontrast"]))
        for plane in ("Lflow", "Lt", "Lx", "Ly", "Ldet"):
            if P[plane] is None:
                assert got[plane] is None
                continue
            np.testing.assert_array_equal(bits(got[plane]), bits(P[plane]), err_msg=f"{plane} of level {i}")
    assert o.level_info(len(lv))["w"] == 0
    if name == "four_octaves_defaults":
        assert len(lv) == 16 and forms == {(0, False), (0, True), (1, True)}     # one launch per step AND the in-LDS form
    # the candidates of the whole frame as a set, no candidate twice; the survivors; the refined records
    cand = [tuple(c) for c in got["cand"].tolist()]
    want = [(l, r, c, int(np.float32(v).view(np.int32))) for l, r, c, v in ref["cand"]]
    assert len(set(cand)) == len(cand) and set(cand) == set(want) and len(want) > 10
    index = {c: i for i, c in enumerate(want)}
    survivors = {c for c, f in zip(cand, got["cflag"].tolist()) if f != 0}
    assert survivors == {c for c, s in zip(want, ref["survives"].tolist()) if s}
    for c, f in zip(cand, got["cflag"].tolist()):
        if f != 0:
            assert f == (1 if ref["refined"][index[c]] is not None else 2), c
    assert got["counts"].tolist() == [len(want), ref["n_refined"], len(ref["xy"]), 0]
    for rec, kept in zip(got["kp"].tolist(), got["kflag"].tolist()):
        k = ref["refined"][index[cand[rec[7]]]]
        assert rec[:3] == bits([k["x"], k["y"], k["size"]]).tolist() and rec[4] == int(bits(k["response"])[0])
        assert rec[5:7] == [k["octave"], k["class_id"]]
        assert bool(kept) == bool(k.get("kept", False))
        if kept:
            assert rec[3] == int(bits(k["angle"])[0]), (rec, k["angle"])
    o.close()


@pytest.mark.parametrize("name", list(S.CASES))
def test_end_to_end_equals_the_restatement_in_the_defined_order(gpu_ctx, name):
    scene, h, w, kw = S.CASES[name]
    ref = S.reference(scene, h, w, **kw)
    o = make(gpu_ctx, **kw)
    img = S.image(scene, h, w)
    got = o.detect_arrays(img)
    assert_same_output(got, ref)
    key = [(c, float(y), float(x)) for (x, y), (_, c) in zip(got[0].tolist(), got[2].tolist())]
    assert [k[0] for k in key] == sorted(k[0] for k in key)                  # class_id ascending
    kps, desc = o.detectAndCompute(img, None)
    if len(ref["xy"]) == 0:
        assert (kps, desc) == ([], None)
    else:
        assert len(kps) == len(desc) == len(ref["xy"]) and desc.dtype == np.uint8
        np.testing.assert_array_equal(desc, ref["desc"])
        assert not (desc[:, 60] & 0xC0).any()                                # the last two bits of byte 60
        i = len(kps) // 2
        k = kps[i]
        assert (k.pt, k.size, k.angle, k.response, k.octave, k.class_id) == \
            (tuple(ref["xy"][i].tolist()), float(ref["aux"][i, 0]), float(ref["aux"][i, 1]), float(ref["aux"][i, 2]), int(ref["lvl"][i, 0]),
             int(ref["lvl"][i, 1]))
    assert o.overflow() == 0
    o.close()


def test_two_runs_are_identical_and_a_larger_instance_changes_nothing(gpu_ctx):
    scene, h, w, _ = S.CASES["two_octaves"]
    img = S.image(scene, h, w)
    a, b = make(gpu_ctx, max_h=90, max_w=170), make(gpu_ctx)
    first = a.detect_arrays(img)
    a.detect_arrays(S.image("mosaic", 61, 97))                               # another frame in between
    for other in (a.detect_arrays(img), b.detect_arrays(img)):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    assert len(first[0]) == len(S.reference(scene, h, w)["xy"]) > 100
    a.close(); b.close()


def test_two_instances_of_different_capacity_alternate_on_one_context(gpu_ctx):
    """Two instances (another frame bound, max_points, and capacities that are exactly the small frame's counts) alive on one
    context and called in turn return, each, what the restatement gives: a piece sized in another unit than its pointer's, or
    two pieces that overlap, would show here."""
    small = S.reference("mosaic", 61, 97)
    specs = [(dict(max_points=40), (83, 163)), (dict(max_h=61, max_w=97, max_candidates=len(small["cand"]), max_keypoints=small["n_refined"]), (61, 97))]
    want = [S.reference("mosaic", 83, 163, max_points=40), small]
    both = [make(gpu_ctx, **kw) for kw, _ in specs]
    for _ in range(2):                                                       # (the first call creates the native instance)
        for o, (_, size), ref in zip(both, specs, want):
            assert_same_output(o.detect_arrays(S.image("mosaic", *size)), ref)
            assert o.overflow() == 0
    assert both[0].capacity != both[1].capacity and both[0].candidate_capacity != both[1].candidate_capacity
    assert both[1].capacity == small["n_refined"] and both[1].candidate_capacity == len(small["cand"])
    for o in both:
        o.close()


def _dev_outputs(ctx, cap, poison=None):
    sizes = dict(xy=cap * 8, aux=cap * 12, lvl=cap * 8, desc=cap * 61, n=4)
    if poison is None:
        return {k: ctx.malloc(v) for k, v in sizes.items()}
    return {k: ctx.upload(np.full(v, poison, np.uint8)) for k, v in sizes.items()}


def test_detect_dev_equals_detect_arrays_and_writes_nothing_beyond_its_rows(gpu_ctx):
    """the device entry on poisoned buffers: the first n rows are the host entry's, every byte past row n - 1 of every output -
    in particular byte 61 n of desc, which a wider store of the last row would touch - is still the poison"""
    scene, h, w, _ = S.CASES["one_octave"]
    img = S.image(scene, h, w)
    o = make(gpu_ctx, max_h=61, max_w=97)
    host = o.detect_arrays(img)
    cap = o.capacity
    d = _dev_outputs(gpu_ctx, cap, poison=0xA5)
    im = gpu_ctx.upload(img)
    o.detect_dev(im, h, w, 1, d["xy"], d["aux"], d["lvl"], d["desc"], d["n"])
    gpu_ctx.sync()
    n = np.zeros(1, np.int32); gpu_ctx.d2h(n, d["n"])
    n = int(n[0])
    assert n == len(host[0]) > 10 and n < cap
    for name, want, row in (("xy", host[0], 8), ("aux", host[1], 12), ("lvl", host[2], 8), ("desc", host[3], 61)):
        raw = np.empty(cap * row, np.uint8); gpu_ctx.d2h(raw, d[name])
        assert raw[:n * row].tobytes() == want.tobytes(), name
        assert (raw[n * row:] == 0xA5).all(), name
    for p in list(d.values()) + [im]:
        gpu_ctx.free(p)
    o.close()


def test_a_frame_beyond_a_capacity_is_voided_not_truncated(gpu_ctx):
    N = load_pkg("_native")
    scene, h, w, _ = S.CASES["two_octaves"]
    ref = S.reference(scene, h, w)
    ncand, nref = len(ref["cand"]), ref["n_refined"]
    img = S.image(scene, h, w)
    for kw, bit in ((dict(max_candidates=ncand - 1), 1), (dict(max_keypoints=nref - 1), 2)):
        o = make(gpu_ctx, **kw)
        assert o.overflow() == 0
        with pytest.raises(N.NativeError, match="candidates and .* keypoints before the quota.*voided"):
            o.detect_arrays(img)
        assert o.overflow() == bit
        d = _dev_outputs(gpu_ctx, o.capacity)
        im = gpu_ctx.upload(img)
        gpu_ctx.h2d(d["n"], np.full(1, 77, np.int32))
        o.detect_dev(im, h, w, 1, d["xy"], d["aux"], d["lvl"], d["desc"], d["n"])
        n = np.full(1, -1, np.int32)
        gpu_ctx.d2h(n, d["n"])
        assert n[0] == 0                                                     # the device count of a voided frame
        small = o.detect_arrays(S.image("mosaic", 61, 97))                   # a frame that fits is served; the word is sticky
        assert_same_output(small, S.reference("mosaic", 61, 97))
        assert o.overflow() == bit
        for p in list(d.values()) + [im]:
            gpu_ctx.free(p)
        o.close()
    exact = make(gpu_ctx, max_candidates=ncand, max_keypoints=nref)          # exactly enough is enough
    assert_same_output(exact.detect_arrays(img), ref)
    assert exact.overflow() == 0 and exact.capacity == nref and exact.candidate_capacity == ncand
    exact.close()
