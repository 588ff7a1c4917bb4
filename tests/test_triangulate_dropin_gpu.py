"""`triangulate_between_kfs_2view` through the overlay names, the way main_revamped.py:562-585 drives it after promoting
a keyframe: a seeded random-init matcher on two planted frames whose keypoints are the two views of one 3-D scene
(tests/triangulate_scenes.py), on the overlay's `Map` and on a plain dict-of-objects map."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest

import frames
import lg_inputs
import triangulate_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SD_L = dict(seed=1, match_gain=4.0, match_bias=3.0)      # random-init weights that produce matches (not vacuous)


@pytest.fixture(scope="module")
def fu():
    return load_pkg("slam.core.features_utils")


@pytest.fixture(scope="module")
def pipeline(fu, gpu_ctx):
    """init_feature_pipeline(args) on seeded random weights, as tests/test_dropin_names_gpu.py sets it up"""
    W = load_pkg("weights")
    sd = W.random_lightglue_state_dict(SD_L["seed"], match_gain=SD_L["match_gain"], match_bias=SD_L["match_bias"])
    mp = pytest.MonkeyPatch()
    mp.setattr(fu._weights, "random_lightglue_state_dict", lambda seed=0: sd)
    mp.setenv(fu.ENV_ALLOW_RANDOM, "1")
    mp.delenv(fu.ENV_ALIKED, raising=False); mp.delenv(fu.ENV_LIGHTGLUE, raising=False)
    args = SimpleNamespace(use_lightglue=True, min_conf=0.7, ransac_thresh=2.0, min_depth=5.0, max_depth=100.0)
    det, mat = fu.init_feature_pipeline(args)
    mp.undo()
    yield args, det, mat
    det.close(); mat.close()


def planted_views(seed=31, n_good=500, n_far=150, n_decoy=250):
    """two frames' (keypoints, descriptors): the projections of one scene in shuffled order with matching descriptors,
    plus decoys that match nothing"""
    s = S.make_scene("dropin", dict(good=n_good, far=n_far), seed)
    rng = np.random.default_rng(seed)
    n = len(s["pts1"])
    m = n + n_decoy
    d = rng.standard_normal((m, 128)).astype(np.float32); d /= np.linalg.norm(d, axis=1, keepdims=True)
    k0 = np.column_stack([rng.uniform(2, 1238, m), rng.uniform(2, 373, m)]).astype(np.float32)
    k0[:n] = s["pts1"]
    o0 = rng.permutation(m)
    k0, d0 = k0[o0], d[o0]
    d1 = d + 0.05 * rng.standard_normal((m, 128)).astype(np.float32)
    d1[n:] = rng.standard_normal((m - n, 128))
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    k1 = np.column_stack([rng.uniform(2, 1238, m), rng.uniform(2, 373, m)]).astype(np.float32)
    k1[:n] = s["pts2"]
    o1 = rng.permutation(m)
    k1, d1 = k1[o1], d1[o1].astype(np.float32)
    return s, (np.ascontiguousarray(k0), np.ascontiguousarray(d0)), (np.ascontiguousarray(k1), np.ascontiguousarray(d1))


class PlainPoint:
    def __init__(self, pid, position):
        self.id, self.position, self.observations, self.keyframe_idx, self.colour = pid, np.array(position, float), [], -1, np.ones(3)

    def add_observation(self, keyframe_idx, kp_idx, descriptor):
        self.observations.append((keyframe_idx, kp_idx, descriptor))


class PlainMap:
    """a reference-style map: a dict of objects, ids from a counter"""
    def __init__(self):
        self.points, self.poses, self.keyframe_indices, self._next_pid = {}, [], [], 0

    def add_points(self, pts3d, colours=None, keyframe_idx=-1):
        ids = []
        for p in np.asarray(pts3d):
            self.points[self._next_pid] = PlainPoint(self._next_pid, p)
            ids.append(self._next_pid)
            self._next_pid += 1
        return ids


@pytest.mark.parametrize("kind", ["overlay_map", "plain_map"])
def test_new_keyframe_grows_the_map_as_the_reference_loop_would(fu, pipeline, gpu_ctx, kind, caplog):
    args, det, mat = pipeline
    tu = load_pkg("slam.core.triangulation_utils")
    tri = load_pkg("triangulation")
    lmu = load_pkg("slam.core.landmark_utils")
    bau = load_pkg("slam.core.ba_utils")
    s, v0, v1 = planted_views()
    img = frames.structured_frame(43)
    planter = lg_inputs.PlantedExtractor(det, [v0, v1])
    try:
        kp0, des0 = fu.feature_extractor(args, img, det)
        kp1, des1 = fu.feature_extractor(args, img, det)
    finally:
        planter.restore()
    np.testing.assert_array_equal(des0, v0[1]); np.testing.assert_array_equal(kp1._xy, v1[0])
    prev_kf = SimpleNamespace(idx=0, kps=kp0, desc=des0, pose=s["T1"].copy())
    cur_kf = SimpleNamespace(idx=1, kps=kp1, desc=des1, pose=s["T2"].copy())
    wmap = lmu.Map() if kind == "overlay_map" else PlainMap()
    for T in (s["T1"], s["T2"]):
        wmap.poses.append(T.copy())
    wmap.keyframe_indices = [0, 1]
    seeded = wmap.add_points(np.array([[0.0, 0.0, 20.0], [1.0, 0.0, 25.0], [0.0, 1.0, 30.0]]))      # a map that is not empty
    first = wmap._next_pid
    assert first == 3 and seeded == [0, 1, 2]

    log = logging.getLogger("test_triangulate_dropin")
    with caplog.at_level(logging.INFO):
        ids = tu.triangulate_between_kfs_2view(args, s["K"], wmap, prev_kf, cur_kf, mat, log, parallax_min_deg=1.0)
    text = caplog.text
    assert "after_RANSAC=" in text and "Parallax(sample of" in text and "reasons:" in text

    # what the function was to compute, from its own three steps
    raw = fu.feature_matcher(args, kp0, kp1, des0, des1, mat)
    matches = fu.filter_matches_ransac(kp0, kp1, raw, args.ransac_thresh)
    pts1 = np.float32([kp0[m.queryIdx].pt for m in matches]); pts2 = np.float32([kp1[m.trainIdx].pt for m in matches])
    X, kept_idx, reasons, _ = tri.triangulate_2view(pts1, pts2, s["K"], s["T1"], s["T2"], min_depth=5.0, max_depth=100.0,
                                                    use_parallax_gate=True, parallax_min_deg=1.0, reproj_px_max=2.0, ctx=gpu_ctx)
    print(f"{kind}: raw {len(raw)}, filtered {len(matches)}, reasons {reasons}")
    assert len(kept_idx) >= 100 and reasons["low_parallax"] >= 20           # real work on both sides of the gate
    assert ids == list(range(first, first + len(kept_idx))) and wmap._next_pid == first + len(ids)
    assert list(wmap.points.keys()) == seeded + ids
    canon = lmu._canon_desc if kind == "overlay_map" else (lambda d: d)
    for pid, m_idx, x in zip(ids, kept_idx.tolist(), X):
        mp = wmap.points[pid]
        assert np.asarray(mp.position).tobytes() == x.tobytes()
        i1, i2 = matches[m_idx].queryIdx, matches[m_idx].trainIdx
        assert len(mp.observations) == 2
        (f1, k1, dd1), (f2, k2, dd2) = mp.observations
        assert (f1, k1, f2, k2) == (0, i1, 1, i2)
        np.testing.assert_array_equal(dd1, canon(des0[i1])); np.testing.assert_array_equal(dd2, canon(des1[i2]))
    # the planted truth: a kept point is the scene's point
    lut = {tuple(p): j for j, p in enumerate(s["pts1"].tolist())}
    j = np.array([lut[tuple(np.float32(kp0[matches[m].queryIdx].pt).tolist())] for m in kept_idx.tolist()])
    assert (s["reason"][j] == S.KEPT).all()
    assert (np.linalg.norm(X - s["X_true"][j], axis=1) / np.linalg.norm(s["X_true"][j], axis=1)).max() < 1e-3

    if kind == "overlay_map":
        d_pos, d_cnt, _ = wmap.device_arrays(gpu_ctx)
        n = len(wmap)
        pos = np.empty((n, 3)); cnt = np.empty(n, np.int32)
        gpu_ctx.d2h(pos, d_pos); gpu_ctx.d2h(cnt, d_cnt)
        assert pos[3:].tobytes() == X.tobytes() and (cnt[3:] == 2).all() and (cnt[:3] == 0).all()
    # the step that follows in the driver: local BA on the grown map
    for mp in [wmap.points[p] for p in seeded]:
        wmap.points.pop(mp.id)                                   # (the three seeds have no observations)
    before = np.array([np.array(wmap.points[p].position) for p in ids])
    bau.local_bundle_adjustment(wmap, s["K"], [prev_kf, cur_kf], center_kf_idx=1, window_size=6, max_iters=5)
    after = np.array([np.array(wmap.points[p].position) for p in ids])
    assert np.isfinite(after).all() and np.abs(after - before).max() < 0.5


def test_no_matches_gives_an_empty_list(fu, pipeline):
    args, det, mat = pipeline
    tu = load_pkg("slam.core.triangulation_utils")
    lmu = load_pkg("slam.core.landmark_utils")
    kf = SimpleNamespace(idx=0, kps=[], desc=np.zeros((0, 128), np.float32), pose=np.eye(4))
    wmap = lmu.Map()
    assert tu.triangulate_between_kfs_2view(args, S.K, wmap, kf, kf, mat, logging.getLogger("t")) == []
    assert len(wmap) == 0
