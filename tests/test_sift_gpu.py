"""SIFT on the GPU (csrc/sift_kernels.hip through sift.py) against the restatement tests/sift_ref.py: every Gaussian and DoG
plane, the candidate sets, the refined keypoints and the orientation histograms through sslam_sift_stage_read, and the
outputs end to end - identical integers, float32 bits and descriptor values, in the defined order.  Shapes are small: what
can go wrong is at edges (odd sides, strides that are no multiple of 4, octaves smaller than the blur radius, octaves without
an interior), not at size."""
import numpy as np
import pytest

import bf_ref
import sift_ref as R
import sift_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

MAXH, MAXW = 100, 136


def make(gpu_ctx, max_h=MAXH, max_w=MAXW, **kw):
    return load_pkg("sift").SIFT_create(max_h=max_h, max_w=max_w, ctx=gpu_ctx, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_output(got, ref):
    xy, aux, octave, desc = got
    assert len(xy) == len(ref["xy"]), (len(xy), len(ref["xy"]))
    assert xy.dtype == np.float32 and aux.dtype == np.float32 and octave.dtype == np.int32 and desc.dtype == np.float32
    assert xy.shape == (len(xy), 2) and aux.shape == (len(xy), 3) and octave.shape == (len(xy),) and desc.shape == (len(xy), 128)
    np.testing.assert_array_equal(bits(xy), bits(ref["xy"]))
    np.testing.assert_array_equal(bits(aux), bits(ref["aux"]))
    np.testing.assert_array_equal(octave, ref["octave"])
    np.testing.assert_array_equal(bits(desc), bits(ref["desc"]))


def assert_defined_order(xy, aux):
    """x, y ascending, size descending, angle ascending - and no two rows agree in all four"""
    key = list(zip(xy[:, 0].tolist(), xy[:, 1].tolist(), (-aux[:, 0].astype(np.float64)).tolist(), aux[:, 1].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)


@pytest.mark.parametrize("name", ["defaults", "small", "three_channels", "layers_5", "stripes_tie"])
def test_every_stage_of_every_octave_equals_the_restatement(gpu_ctx, name):
    scene, h, w, kw = S.CASES[name]
    ref = S.reference(scene, h, w, **kw)
    o = make(gpu_ctx, **kw)
    o.detect_arrays(S.image(scene, h, w))
    nol = kw.get("nOctaveLayers", 3)
    assert ref["sizes"][0] == (2 * w, 2 * h) and min(ref["sizes"][-1]) < 13      # an octave below the smallest blur radius
    got = None
    for oi, (ow, oh) in enumerate(ref["sizes"]):
        info = o.octave_info(oi)
        assert (info["w"], info["h"], info["octaves"], info["layers"], info["threshold"]) == (ow, oh, len(ref["sizes"]), nol + 3, ref["threshold"])
        assert info["interior"] == int(ow > 10 and oh > 10)
        got = o.stage_read(oi)
        np.testing.assert_array_equal(bits(got["gauss"]), bits(ref["gauss"][oi]), err_msg=f"Gaussian planes of octave {oi}")
        np.testing.assert_array_equal(bits(got["dog"]), bits(ref["dog"][oi]), err_msg=f"DoG planes of octave {oi}")
    assert o.octave_info(len(ref["sizes"]))["w"] == 0
    # the candidates of the whole frame as a set, no candidate twice
    cand = [tuple(c) for c in got["cand"].tolist()]
    want = [(oi, l, r, c) for oi, cs in enumerate(ref["cand"]) for l, r, c in cs.tolist()]
    assert len(set(cand)) == len(cand) and set(cand) == set(want) and len(want) > 10
    assert got["counts"].tolist() == [len(want), ref["n_raw"], len(ref["xy"]), 0]
    # the refinement, the response and the smoothed orientation histogram of every candidate
    for key, rec, hist in zip(cand, got["ref"].tolist(), got["hist"]):
        k = ref["refined"][key]
        assert rec[0] == int(k is not None), key
        if k is None:
            continue
        assert rec[1:5] == [k["r"], k["c"], k["layer"], k["octave"]], key
        assert np.array(rec[5:8], np.int32).view(np.uint32).tolist() == bits([k["x"], k["y"], k["size"]]).tolist(), key
        np.testing.assert_array_equal(bits(hist[:36]), bits(ref["hists"][key]), err_msg=str(key))
        assert bits(hist[36]) == bits(k["response"])
    o.close()


END_TO_END = [n for n in S.CASES]


@pytest.mark.parametrize("name", END_TO_END)
def test_end_to_end_equals_the_restatement_in_the_defined_order(gpu_ctx, name):
    scene, h, w, kw = S.CASES[name]
    ref = S.reference(scene, h, w, **kw)
    o = make(gpu_ctx, **kw)
    got = o.detect_arrays(S.image(scene, h, w))
    assert_same_output(got, ref)
    assert_defined_order(got[0], got[1])
    kps, desc = o.detectAndCompute(S.image(scene, h, w), None)
    if len(ref["xy"]) == 0:
        assert (kps, desc) == ([], None)
    else:
        assert len(kps) == len(desc) == len(ref["xy"])
        np.testing.assert_array_equal(desc, ref["desc"])
        assert np.all(desc == np.rint(desc)) and desc.min() >= 0 and desc.max() <= 255
        k = kps[len(kps) // 2]
        i = len(kps) // 2
        assert (k.pt, k.size, k.angle, k.response, k.octave, k.class_id) == (tuple(ref["xy"][i].tolist()), float(ref["aux"][i, 0]),
                                                                             float(ref["aux"][i, 1]), float(ref["aux"][i, 2]),
                                                                             int(ref["octave"][i]), -1)
    assert o.overflow() == 0
    o.close()


def test_two_runs_are_identical_and_a_larger_instance_changes_nothing(gpu_ctx):
    img = S.image("mosaic")
    a, b = make(gpu_ctx), make(gpu_ctx, max_h=240, max_w=333)
    first = a.detect_arrays(img)
    a.detect_arrays(S.image("mosaic", S.HS, S.WS))                           # another frame in between
    for other in (a.detect_arrays(img), b.detect_arrays(img)):
        for x, y in zip(first, other):
            assert x.tobytes() == y.tobytes()
    assert len(first[0]) == 239
    a.close(); b.close()


def test_two_instances_of_different_capacity_alternate_on_one_context(gpu_ctx):
    """An instance lays its memory out from its own capacities.  Two of them (another frame bound, nfeatures, and candidate and
    keypoint capacities that are exactly the small frame's counts: every piece of the two differs in size) alive on one context
    and called in turn return, each, bit for bit what it returns alone on a fresh context - which is the restatement's.  A
    pointer left from the measuring pass, a piece sized in another unit than its pointer's, or two pieces that overlap would
    show here."""
    native = load_pkg("_native")
    small = S.reference("mosaic", S.HS, S.WS)
    specs = [(dict(nfeatures=40), (S.H, S.W)),
             (dict(max_h=S.HS, max_w=S.WS, max_candidates=sum(len(c) for c in small["cand"]), max_keypoints=small["n_raw"]), (S.HS, S.WS))]
    alone = []
    for kw, size in specs:
        ctx = native.Context(0)
        o = make(ctx, **kw)
        alone.append(o.detect_arrays(S.image("mosaic", *size)))
        o.close(); ctx.close()
        assert len(set((alone[-1][2] & 255).tolist())) > 1                   # keypoints in more than one octave
    assert_same_output(alone[0], S.reference("mosaic", S.H, S.W, nfeatures=40))
    assert_same_output(alone[1], small)
    both = [make(gpu_ctx, **kw) for kw, _ in specs]
    for _ in range(2):                                                       # (the first call creates the native instance)
        for o, (_, size), want in zip(both, specs, alone):
            for x, y in zip(o.detect_arrays(S.image("mosaic", *size)), want):
                assert x.tobytes() == y.tobytes()
            assert o.overflow() == 0
    assert both[0].capacity != both[1].capacity and both[0].candidate_capacity != both[1].candidate_capacity
    for o in both:
        o.close()


def test_a_frame_beyond_a_capacity_is_voided_not_truncated(gpu_ctx):
    N = load_pkg("_native")
    ref = S.reference("mosaic")
    ncand, nraw = sum(len(c) for c in ref["cand"]), ref["n_raw"]
    img = S.image("mosaic")
    for kw, bit in ((dict(max_candidates=ncand - 1), 1), (dict(max_keypoints=nraw - 1), 2)):
        o = make(gpu_ctx, **kw)
        assert o.overflow() == 0
        with pytest.raises(N.NativeError, match=f"{ncand} extrema and .* keypoints before the quota.*voided"):
            o.detect_arrays(img)
        assert o.overflow() == bit
        d = [gpu_ctx.upload(img), gpu_ctx.malloc(o.capacity * 8), gpu_ctx.malloc(o.capacity * 12), gpu_ctx.malloc(o.capacity * 4),
             gpu_ctx.malloc(o.capacity * 512), gpu_ctx.upload(np.full(1, 77, np.int32))]
        o.detect_dev(d[0], S.H, S.W, 1, *d[1:])
        n = np.full(1, -1, np.int32)
        gpu_ctx.d2h(n, d[5])
        assert n[0] == 0                                                     # the device count of a voided frame
        small = o.detect_arrays(S.image("mosaic", S.HS, S.WS))               # a frame that fits is served; the word is sticky
        assert_same_output(small, S.reference("mosaic", S.HS, S.WS))
        assert o.overflow() == bit
        for p in d:
            gpu_ctx.free(p)
        o.close()
    exact = make(gpu_ctx, max_candidates=ncand, max_keypoints=nraw)          # exactly enough is enough
    assert_same_output(exact.detect_arrays(img), ref)
    assert exact.overflow() == 0 and exact.capacity == nraw and exact.candidate_capacity == ncand
    exact.close()


def test_the_device_chain_equals_the_host_path_through_the_same_objects(gpu_ctx):
    """detect_dev twice -> match_dev (NORM_L2, D = 128) -> filter_matches_dev on a 1241 x 376 instance, nothing read back in
    between, equals the same chain fed from host arrays; SIFT descriptors are integer-valued, so the L2 distances are exact
    and compare as bits (tests/bf_ref.py)."""
    B, E, native = load_pkg("bf_matcher"), load_pkg("epipolar"), load_pkg("_native")
    f0, f1 = S.shifted_pair()
    h, w = f0.shape
    ctx = gpu_ctx
    o = make(ctx, max_h=376, max_w=1241, nfeatures=300)
    m = B.BFMatcher(B.NORM_L2, crossCheck=True, ctx=ctx)
    host = [o.detect_arrays(f) for f in (f0, f1)]
    cap, rows = o.capacity, o.chain_rows
    assert rows == min(cap, B.MAX_ROWS) and min(len(host[0][0]), len(host[1][0])) >= 100
    dev = []
    for f in (f0, f1):
        d = dict(img=ctx.upload(f), xy=ctx.malloc(cap * 8), aux=ctx.malloc(cap * 12), octave=ctx.malloc(cap * 4), desc=ctx.malloc(cap * 512),
                 n=ctx.malloc(4))
        o.detect_dev(d["img"], h, w, 1, d["xy"], d["aux"], d["octave"], d["desc"], d["n"])
        dev.append(d)
    ij_dev, dist_dev, info_dev = ctx.malloc(cap * 8), ctx.malloc(cap * 4), ctx.malloc(16)
    m.match_dev(ctx, 128, dev[0]["desc"], rows, dev[1]["desc"], rows, ij_dev, dist_dev, info_dev, m_dev=dev[0]["n"], n_dev=dev[1]["n"])
    kept_dev, finfo_dev, mask_dev = ctx.malloc(cap * 8), ctx.malloc(16), ctx.malloc(cap)
    E.filter_matches_dev(ctx, rows, info_dev, dev[0]["xy"], dev[1]["xy"], ij_dev, kept_dev, finfo_dev, thresh=1.0, mask_out_dev=mask_dev)
    ctx.sync()
    # the device entry's outputs and count are the host entry's
    for d, (xy, aux, octave, desc) in zip(dev, host):
        n = np.zeros(1, np.int32); ctx.d2h(n, d["n"])
        assert n[0] == len(xy)
        for name, want in (("xy", xy), ("aux", aux), ("octave", octave), ("desc", desc)):
            got = np.empty_like(want); ctx.d2h(got, d[name])
            assert got.tobytes() == want.tobytes(), name
    # the matches: the host path through the same matcher, and the defined arithmetic of bf_ref
    ij, dist = m.match_arrays(host[0][3], host[1][3])
    ij_ref, dist_ref = bf_ref.match(host[0][3], host[1][3], bf_ref.NORM_L2, True)
    np.testing.assert_array_equal(ij, ij_ref)
    np.testing.assert_array_equal(bits(dist), bits(dist_ref))
    info = np.zeros(4, np.int32); ctx.d2h(info, info_dev)
    assert info.tolist() == [len(ij), len(host[0][0]), len(host[1][0]), 0] and len(ij) >= 50
    got_ij, got_dist = np.empty_like(ij), np.empty_like(dist)
    ctx.d2h(got_ij, ij_dev); ctx.d2h(got_dist, dist_dev)
    np.testing.assert_array_equal(got_ij, ij)
    np.testing.assert_array_equal(bits(got_dist), bits(dist))
    # most mutual pairs are the shift (7, 4)
    dd = host[0][0][ij[:, 0]] - host[1][0][ij[:, 1]]
    assert (np.abs(dd - np.array([7, 4], np.float32)).max(axis=1) < 0.5).mean() > 0.5
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
