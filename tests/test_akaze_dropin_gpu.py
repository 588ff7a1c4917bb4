"""The substitution a maintainer makes in the reference's OpenCV branch for `--detector akaze --matcher bf`:
`_get_opencv_detector` returns `akaze.AKAZE_create()` and `_get_opencv_matcher` `bf_matcher.BFMatcher(NORM_HAMMING,
crossCheck=True)`.  The overlay's untouched `feature_extractor`, `feature_matcher` and `filter_matches_ransac` run on those
objects and return, on a frame and its integer shift, what the restatements (tests/akaze_ref.py, tests/bf_ref.py) return
through the same functions; the device chain returns the same without a host round trip; and a map built from one frame's
61-byte rows is tracked in the shifted frame through the Hamming branch of `reproject_and_match_2d3d` to a pose - the first
real 61-byte input of those paths."""
import types
from types import SimpleNamespace

import numpy as np
import pytest

import akaze_ref as R
import akaze_scenes as S
import bf_ref
import pnp_scenes as PS
import reproject_hamming_ref as HR
from conftest import load_pkg

pytestmark = pytest.mark.gpu

H, W, DX, DY = 83, 163, 7, 4


def frames():
    return S.shifted_pair(H, W, DX, DY)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class RefDetector:
    """akaze_ref behind `detectAndCompute`"""

    def __init__(self, KeyPoint):
        self.KeyPoint = KeyPoint

    def detectAndCompute(self, img, mask=None):
        r = R.detect(img)
        if len(r["xy"]) == 0:
            return [], None
        return [self.KeyPoint(x, y, s, a, resp, o, c) for (x, y), (s, a, resp), (o, c) in zip(r["xy"].tolist(), r["aux"].tolist(), r["lvl"].tolist())], r["desc"]


class RefMatcher:
    """bf_ref behind `match`"""

    def __init__(self, DMatch):
        self.DMatch = DMatch

    def match(self, q, t):
        ij, dist = bf_ref.match(q, t, bf_ref.NORM_HAMMING, True)
        return [self.DMatch(int(a), int(b), 0, float(d)) for (a, b), d in zip(ij.tolist(), dist.tolist())]


def run(fu, args, detector, matcher, fr):
    kp0, des0 = fu.feature_extractor(args, fr[0], detector)
    kp1, des1 = fu.feature_extractor(args, fr[1], detector)
    matches = fu.feature_matcher(args, kp0, kp1, des0, des1, matcher)
    kept = fu.filter_matches_ransac(kp0, kp1, matches, 1.0)
    return kp0, des0, kp1, des1, matches, kept


def test_the_akaze_branch_runs_on_the_substituted_pair_and_equals_the_restatements(gpu_ctx):
    fu, T, A, B = load_pkg("slam.core.features_utils"), load_pkg("slam.core.types"), load_pkg("akaze"), load_pkg("bf_matcher")
    args = SimpleNamespace(use_lightglue=False, detector="akaze", matcher="bf", max_features=1000)
    detector = A.AKAZE_create(max_h=H, max_w=W, ctx=gpu_ctx)
    matcher = B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=gpu_ctx)
    fr = frames()
    got = run(fu, args, detector, matcher, fr)
    want = run(fu, args, RefDetector(T.KeyPoint), RefMatcher(T.DMatch), fr)
    for ka, kb in ((got[0], want[0]), (got[2], want[2])):
        fields = lambda ks: [(k.pt, k.size, k.angle, k.response, k.octave, k.class_id) for k in ks]
        assert fields(ka) == fields(kb) and len(ka) >= 100
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[3])
    for ma, mb in ((got[4], want[4]), (got[5], want[5])):
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in ma] == [(m.queryIdx, m.trainIdx, m.distance) for m in mb]
    kp0, des0, kp1, des1, matches, kept = got
    assert des0.dtype == np.uint8 and des0.shape == (len(kp0), 61) and len(matches) >= 8 and len(kept) >= 8
    assert matches == sorted(matches, key=lambda m: m.distance)
    # matched keypoints are displaced by the shift
    moved = np.array([np.subtract(kp0[m.queryIdx].pt, kp1[m.trainIdx].pt) for m in kept])
    assert (np.abs(moved - (DX, DY)).max(axis=1) < 0.5).mean() > 0.8
    assert detector.detectAndCompute(S.constant(H, W), None) == ([], None)
    assert fu.feature_extractor(args, S.constant(H, W), detector) == ([], [])
    detector.close()


def test_the_device_chain_equals_the_host_path_through_the_same_objects(gpu_ctx):
    """detect_dev twice -> match_dev (NORM_HAMMING, D = 61) -> filter_matches_dev, nothing read back in between, equals the host
    entries and tests/bf_ref.py on the restatement's descriptors"""
    A, B, E = load_pkg("akaze"), load_pkg("bf_matcher"), load_pkg("epipolar")
    ctx = gpu_ctx
    fr = frames()
    o = A.AKAZE_create(max_h=H, max_w=W, ctx=ctx)
    m = B.BFMatcher(B.NORM_HAMMING, crossCheck=True, ctx=ctx)
    host = [o.detect_arrays(f) for f in fr]
    cap, rows = o.capacity, o.chain_rows
    assert rows == min(cap, B.MAX_ROWS)
    dev = []
    for f in fr:
        d = dict(img=ctx.upload(f), xy=ctx.malloc(cap * 8), aux=ctx.malloc(cap * 12), lvl=ctx.malloc(cap * 8), desc=ctx.malloc(cap * 61), n=ctx.malloc(4))
        o.detect_dev(d["img"], H, W, 1, d["xy"], d["aux"], d["lvl"], d["desc"], d["n"])
        dev.append(d)
    ij_dev, dist_dev, info_dev = ctx.malloc(cap * 8), ctx.malloc(cap * 4), ctx.malloc(16)
    m.match_dev(ctx, 61, dev[0]["desc"], rows, dev[1]["desc"], rows, ij_dev, dist_dev, info_dev, m_dev=dev[0]["n"], n_dev=dev[1]["n"])
    kept_dev, finfo_dev, mask_dev = ctx.malloc(cap * 8), ctx.malloc(16), ctx.malloc(cap)
    E.filter_matches_dev(ctx, rows, info_dev, dev[0]["xy"], dev[1]["xy"], ij_dev, kept_dev, finfo_dev, thresh=1.0, mask_out_dev=mask_dev)
    ctx.sync()
    for d, f, (xy, aux, lvl, desc) in zip(dev, fr, host):
        ref = R.detect(f)
        n = np.zeros(1, np.int32); ctx.d2h(n, d["n"])
        assert n[0] == len(xy) == len(ref["xy"])
        np.testing.assert_array_equal(desc, ref["desc"])
        for name, want in (("xy", xy), ("aux", aux), ("lvl", lvl), ("desc", desc)):
            got = np.empty_like(want); ctx.d2h(got, d[name])
            assert got.tobytes() == want.tobytes(), name
    ij, dist = m.match_arrays(host[0][3], host[1][3])
    ij_ref, dist_ref = bf_ref.match(host[0][3], host[1][3], bf_ref.NORM_HAMMING, True)
    np.testing.assert_array_equal(ij, ij_ref)
    np.testing.assert_array_equal(bits(dist), bits(dist_ref))
    info = np.zeros(4, np.int32); ctx.d2h(info, info_dev)
    assert info.tolist() == [len(ij), len(host[0][0]), len(host[1][0]), 0] and len(ij) >= 8
    got_ij, got_dist = np.empty_like(ij), np.empty_like(dist)
    ctx.d2h(got_ij, ij_dev); ctx.d2h(got_dist, dist_dev)
    np.testing.assert_array_equal(got_ij, ij)
    np.testing.assert_array_equal(bits(got_dist), bits(dist))
    finfo = np.zeros(4, np.int32); ctx.d2h(finfo, finfo_dev)
    kept = np.empty((max(int(finfo[0]), 0), 2), np.int32)
    assert len(kept) >= 8
    ctx.d2h(kept, kept_dev)
    dd = host[0][0][kept[:, 0]] - host[1][0][kept[:, 1]]
    assert (np.abs(dd - np.array([DX, DY], np.float32)).max(axis=1) < 0.5).mean() > 0.8
    for d in dev:
        for p in d.values():
            ctx.free(p)
    for p in (ij_dev, dist_dev, info_dev, kept_dev, finfo_dev, mask_dev):
        ctx.free(p)
    o.close()


def test_a_map_of_akaze_rows_is_tracked_in_the_shifted_frame_to_a_pose(gpu_ctx):
    """Frame 0's keypoints become landmarks at depths of 6 .. 10 m in front of the camera (intrinsics K0); the shifted frame is
    the same camera with the principal point moved by the shift, so every landmark projects onto its keypoint's place in
    frame 1; the world frame is turned and moved against the camera's, so the true pose is not the identity.  Map.add_points / add_observation from the 61-byte rows -> reproject_and_match_2d3d
    (compared with tests/reproject_hamming_ref.py) -> solve_pnp_ransac, within the tolerance tests/test_pnp_gpu.py asks of the
    same solver (2 degrees, 0.1 m)."""
    A, P, L = load_pkg("akaze"), load_pkg("slam.core.pnp_utils"), load_pkg("slam.core.landmark_utils")
    fr = frames()
    o = A.AKAZE_create(max_h=H, max_w=W, ctx=gpu_ctx)
    (xy0, _, _, des0), (xy1, _, _, des1) = [o.detect_arrays(f) for f in fr]
    f, cx, cy = 200.0, W / 2, H / 2
    K0 = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], np.float64)
    K1 = np.array([[f, 0, cx - DX], [0, f, cy - DY], [0, 0, 1]], np.float64)
    z = 6.0 + 4.0 * ((np.arange(len(xy0)) * 7) % 11) / 11.0
    Xc = np.stack([(xy0[:, 0] - cx) * z / f, (xy0[:, 1] - cy) * z / f, z], 1)
    a = np.radians(5.0)
    Tcw = np.eye(4)
    Tcw[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    Tcw[:3, 3] = [0.3, -0.2, 0.5]
    X = (Xc - Tcw[:3, 3]) @ Tcw[:3, :3]                                 # R^T (Xc - t)
    m = L.Map()
    ids = m.add_points(X)
    wmap = types.SimpleNamespace(points={})
    for i, pid in enumerate(ids):
        m.points[pid].add_observation(0, i, des0[i])
        wmap.points[pid] = types.SimpleNamespace(position=X[i].copy(), observations=[(0, i, des0[i].copy())])
    m.resync()
    assert m.binary_width == 61 and des0.shape[1] == 61
    r = P.reproject_and_match_2d3d(m, K1, Tcw, xy1, des1, W, H, radius_px=4.0, max_hamm=100)
    want = HR.reproject_and_match_hamming(wmap, K1, Tcw, xy1, des1, W, H, 4.0, 100)
    np.testing.assert_array_equal(r.kp_indices, want[2])
    np.testing.assert_array_equal(r.mp_ids, want[3])
    np.testing.assert_array_equal(bits(r.pts3d), bits(want[0]))
    np.testing.assert_array_equal(bits(r.pts2d), bits(want[1]))
    assert len(r.kp_indices) >= 30
    T, mask = P.solve_pnp_ransac(r.pts3d, r.pts2d, K1, PS.RANSAC_PX, Tcw_init=Tcw, iters=PS.ITERS, conf=PS.CONF)
    assert T is not None and mask.sum() >= 0.5 * len(mask)
    assert PS.rot_err_deg(T[:3, :3], Tcw[:3, :3]) < 2.0 and np.linalg.norm(T[:3, 3] - Tcw[:3, 3]) < 0.1
    o.close()
