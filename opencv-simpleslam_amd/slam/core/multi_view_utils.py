"""`multi_view_triangulation` and `MultiViewTriangulator` on the HIP backend: map growth from every observation of a
track, not only from its first keyframe pair.

The reference's tests import both names from `slam.core.multi_view_utils` (tests/test_multi_view_utils.py) and the function
from `slam.core.triangulation_utils` (tests/test_multi_view_triangulation-minimal.py); its drivers still carry the knobs
(`--mvt_rep_err`, `--merge_radius`, `--min_depth`, `--max_depth`) - the module itself is not in its tree.  What is built
here is the contract those tests and the CLI help record (include/sslam_hip.h states it); PARITY UNPINNED.

    triangulate + gate  `sslam_triangulate_tracks_host`: ONE device call for all ready tracks - the DLT over all of a
                        track's observations, the homogeneous test, depth window, cheirality, MEAN reprojection error
    insert              one `world_map.add_points(X, colours)` in ascending track id, then `add_observation` per
                        observation that has a descriptor, on the overlay's `Map` and on a dict-of-objects map alike
    fuse                `landmark_fusion.fuse_closeby`: the greedy rule of `Map.fuse_closeby_duplicate_landmarks`
                        (landmark_utils.py:138-161) on pairs found by the device search
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from .types import xy_from_keypoints
from ... import landmark_fusion as _fusion
from ... import multiview as _mv


def _tcw(pose_w_c) -> np.ndarray:
    T = np.asarray(pose_w_c, np.float64)
    if T.shape != (4, 4):
        raise ValueError("pose_w_c must be a 4x4 camera-to-world matrix")
    return np.linalg.inv(T)


def multi_view_triangulation(K, poses_w_c, pts2d, min_depth: float = 0.40, max_depth: float = 100.0,
                             max_rep_err: float = 2.0, ctx=None):
    """One track: `poses_w_c` V camera-to-world 4x4 matrices, `pts2d` [V,2] pixels (read as float32).  The world point
    [3] float64, or None when a gate rejects it (fewer than two views, unusable w, a depth outside
    [min_depth, max_depth], a view behind the point, mean reprojection error above `max_rep_err`).  The same device
    call as the triangulator's, with one track."""
    uv = np.asarray(pts2d, np.float32).reshape(-1, 2)
    V = len(uv)
    if len(poses_w_c) != V:
        raise ValueError("poses_w_c / pts2d length mismatch")
    Tcw = np.stack([_tcw(T) for T in poses_w_c]) if V else np.empty((0, 4, 4))
    X, idx, _, _ = _mv.triangulate_tracks(K, Tcw, [0, V], np.arange(V, dtype=np.int32), uv, min_depth, max_depth,
                                          max_rep_err, ctx=ctx)
    return X[0].copy() if len(idx) else None


class _KeyframeRecord:
    __slots__ = ("frame_idx", "Tcw", "xy", "img", "descs")

    def __init__(self, frame_idx, Tcw, xy, img, descs):
        self.frame_idx, self.Tcw, self.xy, self.img, self.descs = frame_idx, Tcw, xy, img, descs


class MultiViewTriangulator:
    """Collects the observations of feature tracks keyframe by keyframe and turns every track with at least `min_views`
    of them into a landmark."""

    def __init__(self, K, min_views: int = 2, merge_radius: float = 0.10, max_rep_err: float = 2.0,
                 min_depth: float = 0.40, max_depth: float = 100.0, ctx=None):
        self.K = np.asarray(K, np.float64).reshape(3, 3).copy()
        self.min_views = int(min_views)
        self.merge_radius = float(merge_radius)
        self.max_rep_err = float(max_rep_err)
        self.min_depth = float(min_depth)
        self.max_depth = float(max_depth)
        self.ctx = ctx
        self._kfs: List[_KeyframeRecord] = []
        self._tracks: Dict[int, list] = {}               # track_id -> [(keyframe slot, kp_idx)] in insertion order
        self._done = set()                               # tracks that became landmarks
        self._tried: Dict[int, int] = {}                 # rejected track -> its observation count when it was rejected

    def add_keyframe(self, frame_idx, pose_w_c, kps, track_map, img=None, descs=None) -> None:
        """`kps`: anything with `.pt` per item, a `KeyPointList`, or an [n,2] array; `track_map` {track_id: kp_idx};
        `img` BGR uint8 or None; `descs` indexable by kp_idx, or None."""
        xy = (np.asarray(kps, np.float32).reshape(-1, 2) if isinstance(kps, np.ndarray) else xy_from_keypoints(kps)).copy()
        slot = len(self._kfs)
        for tid, kp_idx in track_map.items():
            if not 0 <= int(kp_idx) < len(xy):
                raise IndexError(f"track {tid}: keypoint {kp_idx} outside the {len(xy)} keypoints of frame {frame_idx}")
        self._kfs.append(_KeyframeRecord(int(frame_idx), _tcw(pose_w_c), xy, img, descs))
        for tid, kp_idx in track_map.items():
            self._tracks.setdefault(int(tid), []).append((slot, int(kp_idx)))

    def _colour(self, slot: int, kp_idx: int) -> np.ndarray:
        kf = self._kfs[slot]
        if kf.img is None:
            return np.ones(3, np.float32)
        img = np.asarray(kf.img)
        h, w = img.shape[:2]
        u = int(np.clip(np.rint(kf.xy[kp_idx, 0]), 0, w - 1))
        v = int(np.clip(np.rint(kf.xy[kp_idx, 1]), 0, h - 1))
        return np.asarray(img[v, u, :3], np.float32)[::-1] / np.float32(255.0)          # BGR -> RGB

    def triangulate_ready_tracks(self, world_map) -> List[int]:
        """Every track with at least `min_views` observations that is not a landmark yet (a rejected one only after it
        gained an observation), in ascending track id: one device call, the kept ones added to `world_map`, then the
        fusion within `merge_radius`.  Returns the new ids that are still in `world_map.points`."""
        ready = sorted(t for t, obs in self._tracks.items()
                       if t not in self._done and len(obs) >= self.min_views and self._tried.get(t) != len(obs))
        if not ready:
            return []
        counts = np.fromiter((len(self._tracks[t]) for t in ready), np.int64, len(ready))
        off = np.zeros(len(ready) + 1, np.int32)
        np.cumsum(counts, out=off[1:])
        view = np.fromiter((s for t in ready for s, _ in self._tracks[t]), np.int32, int(off[-1]))
        uv = np.empty((int(off[-1]), 2), np.float32)
        o = 0
        for t in ready:
            for s, k in self._tracks[t]:
                uv[o] = self._kfs[s].xy[k]
                o += 1
        Tcw = np.stack([kf.Tcw for kf in self._kfs])
        X, kept, _, _ = _mv.triangulate_tracks(self.K, Tcw, off, view, uv, self.min_depth, self.max_depth,
                                               self.max_rep_err, ctx=self.ctx)
        kept = kept.tolist()
        kept_set = set(kept)
        for i, t in enumerate(ready):
            if i not in kept_set:
                self._tried[t] = len(self._tracks[t])
        if not kept:
            return []
        firsts = [self._tracks[ready[i]][0] for i in kept]
        colours = np.stack([self._colour(s, k) for s, k in firsts])
        new_ids = list(world_map.add_points(np.ascontiguousarray(X, np.float64), colours))
        if len(new_ids) != len(kept):
            raise RuntimeError("Map.add_points returned no ids.")
        for pid, i, (s0, _) in zip(new_ids, kept, firsts):
            t = ready[i]
            mp = world_map.points[pid]
            mp.keyframe_idx = self._kfs[s0].frame_idx
            for s, k in self._tracks[t]:
                kf = self._kfs[s]
                if kf.descs is not None:
                    mp.add_observation(kf.frame_idx, k, kf.descs[k])
            self._done.add(t)
            self._tried.pop(t, None)
        if self.merge_radius > 0:
            _fusion.fuse_closeby(world_map, self.merge_radius, self.ctx)
        return [pid for pid in new_ids if pid in world_map.points]
