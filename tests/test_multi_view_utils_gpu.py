"""`MultiViewTriangulator` / `multi_view_triangulation` through the overlay names (slam/core/multi_view_utils.py), driven the
way the reference's tests/test_multi_view_utils.py drives the module it no longer has: keyframes fed one by one, then
`triangulate_ready_tracks(world_map)` - on the overlay's `Map` and on a plain dict-of-objects map."""
import numpy as np
import pytest

import multiview_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

GATES = dict(max_rep_err=2.0, min_depth=0.1, max_depth=10.0)


class KP:
    def __init__(self, x, y):
        self.pt = (float(x), float(y))


class PlainPoint:
    def __init__(self, pid, position, colour):
        self.id, self.position, self.colour, self.observations, self.keyframe_idx = pid, np.array(position, float), colour, [], -1

    def add_observation(self, keyframe_idx, kp_idx, descriptor):
        self.observations.append((keyframe_idx, kp_idx, descriptor))


class PlainMap:
    """a reference-style map: a dict of objects, ids from a counter"""
    def __init__(self):
        self.points, self._next_pid = {}, 0

    def add_points(self, pts3d, colours=None, keyframe_idx=-1):
        ids = []
        for k, p in enumerate(np.asarray(pts3d)):
            self.points[self._next_pid] = PlainPoint(self._next_pid, p, np.ones(3) if colours is None else np.asarray(colours[k]))
            ids.append(self._next_pid)
            self._next_pid += 1
        return ids

    def get_point_array(self):
        return np.array([p.position for p in self.points.values()]).reshape(-1, 3)


@pytest.fixture(scope="module")
def mvu():
    return load_pkg("slam.core.multi_view_utils")


@pytest.fixture(scope="module")
def lmu():
    return load_pkg("slam.core.landmark_utils")


def _image(seed):
    return np.random.default_rng(seed).integers(0, 256, (480, 640, 3), dtype=np.uint8)


def _descs(frame, n):
    return [np.full(32, (7 * frame + k) % 251, np.uint8) for k in range(n)]


def feed(tri, poses, pts2d, as_array=False, frame0=100):
    """every point is track `pid` and keypoint `pid` of every view; frames are numbered from `frame0`"""
    for f, (pose, uv) in enumerate(zip(poses, pts2d)):
        kps = np.asarray(uv) if as_array else [KP(u, v) for u, v in uv]
        tri.add_keyframe(frame0 + f, pose, kps, {pid: pid for pid in range(len(uv))}, _image(f), _descs(f, len(uv)))


def build(mvu, world_map, seed, merge_radius, gpu_ctx, min_views=2, as_array=False):
    K, poses, pts_w, pts2d = S.five_view_scene(seed)
    tri = mvu.MultiViewTriangulator(K, min_views=min_views, merge_radius=merge_radius, ctx=gpu_ctx, **GATES)
    feed(tri, poses, pts2d, as_array)
    return tri, tri.triangulate_ready_tracks(world_map), pts_w, pts2d


def _snapshot(world_map):
    return [(pid, np.array(p.position).tobytes(), [(f, k, np.asarray(d).tobytes()) for f, k, d in p.observations])
            for pid, p in world_map.points.items()]


@pytest.mark.parametrize("min_views", [2, 3])
def test_every_track_becomes_a_landmark(mvu, lmu, gpu_ctx, min_views):
    world_map = lmu.Map()
    tri, new_ids, pts_w, pts2d = build(mvu, world_map, 1, 0.1, gpu_ctx, min_views)
    assert new_ids == list(range(len(pts_w))) == list(world_map.points)          # (no two true points within the radius: nothing fuses)
    errs = [np.linalg.norm(world_map.points[pid].position - pts_w[pid]) for pid in new_ids]
    rms = float(np.sqrt(np.mean(np.square(errs))))
    print(f"min_views {min_views}: RMS {rms:.4f} m")
    assert rms < 5e-2
    cols = world_map.get_color_array()
    for pid in new_ids:
        mp = world_map.points[pid]
        assert mp.keyframe_idx == 100
        assert [(f, k) for f, k, _ in mp.observations] == [(100 + f, pid) for f in range(5)]
        for f, (_, _, d) in enumerate(mp.observations):
            np.testing.assert_array_equal(d, _descs(f, pid + 1)[pid])
        u, v = np.rint(pts2d[0][pid]).astype(int)
        want = _image(0)[np.clip(v, 0, 479), np.clip(u, 0, 639)][::-1].astype(np.float32) / np.float32(255)
        np.testing.assert_array_equal(cols[pid], want)
    # the single-track function is the same device call: bitwise the landmark
    K, poses, _, _ = S.five_view_scene(1)
    X = mvu.multi_view_triangulation(K, poses, np.float32([v[3] for v in pts2d]), ctx=gpu_ctx, **GATES)
    assert X.dtype == np.float64 and X.tobytes() == np.array(world_map.points[3].position).tobytes()
    assert mvu.multi_view_triangulation(K, poses[:1], pts2d[0][3:4], ctx=gpu_ctx, **GATES) is None


def test_no_image_and_no_descriptors(mvu, lmu, gpu_ctx):
    K, poses, pts_w, pts2d = S.five_view_scene(1)
    tri = mvu.MultiViewTriangulator(K, ctx=gpu_ctx, **GATES)
    for f, (pose, uv) in enumerate(zip(poses, pts2d)):
        tri.add_keyframe(f, pose, uv, {pid: pid for pid in range(len(uv))}, None, None)
    world_map = lmu.Map()
    ids = tri.triangulate_ready_tracks(world_map)
    assert len(ids) == len(pts_w)
    assert (world_map.get_color_array() == 1.0).all()
    assert all(world_map.points[p].observations == [] for p in ids)


@pytest.mark.parametrize("kind", ["overlay_map", "plain_map"])
def test_fusion_equals_the_existing_method_on_the_unfused_map(mvu, lmu, gpu_ctx, kind):
    """seed 7: three true pairs within 0.1 m (the nearest at 0.068).  merge_radius = 0.1 gives the map that merge_radius = 0
    followed by `Map.fuse_closeby_duplicate_landmarks(0.1)` gives: ids, positions and observation lists bit-equal."""
    _, _, pts_w, _ = S.five_view_scene(7)
    d_true = np.linalg.norm(pts_w[:, None] - pts_w[None], axis=2)[np.triu_indices(len(pts_w), 1)]
    assert (d_true < 0.1).sum() == 3 and abs(d_true.min() - 0.068) < 1e-3
    plain = lmu.Map()
    _, ids0, _, _ = build(mvu, plain, 7, 0.0, gpu_ctx)
    assert ids0 == list(range(len(pts_w)))
    p = plain.get_point_array()
    d = np.linalg.norm(p[:, None] - p[None], axis=2)[np.triu_indices(len(p), 1)]
    assert (np.abs(d - 0.1) > 1e-9 * 0.1).all() and (d < 0.1).any()          # no pair on the radius, some inside
    plain.fuse_closeby_duplicate_landmarks(0.1)
    assert len(plain.points) < len(pts_w)
    fused = lmu.Map() if kind == "overlay_map" else PlainMap()
    _, ids, _, _ = build(mvu, fused, 7, 0.1, gpu_ctx, as_array=(kind == "plain_map"))
    assert _snapshot(fused) == _snapshot(plain)
    assert ids == list(fused.points) == list(plain.points)
    if kind == "overlay_map":
        np.testing.assert_array_equal(fused.get_point_array(), plain.get_point_array())
        np.testing.assert_array_equal(fused.soa()[0], plain.soa()[0])


def test_a_rejected_track_waits_for_a_new_observation(mvu, lmu, gpu_ctx, monkeypatch):
    calls = []
    real = mvu._mv.triangulate_tracks

    def counting(K, Tcw, off, *a, **kw):
        calls.append(len(off) - 1)
        return real(K, Tcw, off, *a, **kw)

    monkeypatch.setattr(mvu._mv, "triangulate_tracks", counting)
    K, poses, pts_w, pts2d = S.five_view_scene(1, n_pts=11)
    tri = mvu.MultiViewTriangulator(K, merge_radius=0.0, ctx=gpu_ctx, **GATES)
    bad = 10                                                  # track 10: its second observation is 40 px off
    uv1 = pts2d[1].copy()
    uv1[bad, 1] += 40.0
    everyone = {pid: pid for pid in range(11)}
    tri.add_keyframe(0, poses[0], pts2d[0], everyone)
    tri.add_keyframe(1, poses[1], uv1, everyone)
    world_map = lmu.Map()
    assert tri.triangulate_ready_tracks(world_map) == list(range(10)) and calls == [11]
    assert tri.triangulate_ready_tracks(world_map) == [] and calls == [11]       # nothing new: nothing launched
    tri.add_keyframe(2, poses[2], pts2d[2], {pid: pid for pid in range(10)})     # observations of landmarks only
    assert tri.triangulate_ready_tracks(world_map) == [] and calls == [11]
    tri.add_keyframe(3, poses[3], pts2d[3], {bad: bad})                          # the rejected track gains one: it alone is tried
    out = tri.triangulate_ready_tracks(world_map)
    assert calls == [11, 1] and out in ([], [10])
    assert tri.triangulate_ready_tracks(world_map) == [] and calls == [11, 1]
