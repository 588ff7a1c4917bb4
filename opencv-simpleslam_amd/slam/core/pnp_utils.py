"""Drop-in for the reference's `slam/core/pnp_utils.py` on the HIP backend: `reproject_and_match_2d3d`
(pnp_utils.py:224-304), the PnP solvers `solve_pnp_ransac` (:307-341) and `refine_pose_pnp` (:200-221) - OpenCV's
classic `solvePnPRansac(SOLVEPNP_ITERATIVE)` restated on the GPU, no cv2 - plus the cv2-free helpers around them
(`Matches2D3D`, `_project_points`, `predict_pose_const_vel`).  A maintainer patches in the functions:

    import slam.core.pnp_utils as ref
    for name in ("reproject_and_match_2d3d", "solve_pnp_ransac", "refine_pose_pnp"):
        setattr(ref, name, getattr(amd_pnp_utils, name))

Four correspondences (OpenCV's P3P minimal solver) are outside this backend's scope and raise NotImplementedError.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ... import _native
from ... import pnp as _pnp
from .landmark_utils import BIN_ROW, DESC_DIM, MAX_OBS_CHECK, gather_rows


@dataclass
class Matches2D3D:
    pts3d: np.ndarray          # (N,3) world
    pts2d: np.ndarray          # (N,2) image
    kp_indices: List[int]      # indices into current frame keypoints
    mp_ids: List[int]          # matched map point ids


def _pose_inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    Ti = np.eye(4, dtype=T.dtype)
    Ti[:3, :3] = R.T
    Ti[:3, 3] = -R.T @ t
    return Ti


def predict_pose_const_vel(Tcw_prevprev, Tcw_prev):
    """T_pred = T_prev * inv(T_prevprev) * T_prev (pnp_utils.py:26-30)."""
    return Tcw_prev @ _pose_inverse(Tcw_prevprev) @ Tcw_prev


def _kp_coords(kps):
    if isinstance(kps, (list, tuple)):
        if len(kps) == 0:
            return np.empty((0, 2), np.float32)
        if hasattr(kps[0], "pt"):
            return np.float32([kp.pt for kp in kps])
    kps = np.asarray(kps)
    if kps.size == 0:
        return np.empty((0, 2), np.float32)
    assert kps.ndim == 2 and kps.shape[1] >= 2, "kps must be (N,2)"
    return np.ascontiguousarray(kps[:, :2], np.float32)


def _snapshot(world_map, dtype, stored, width, uint8):
    """SoA view of `world_map.points` for the kernel: ids, positions, and per point the count and the rows of `width`
    elements that `gather_rows` - the reference's skip rule - keeps, in zeroed rows of `stored` elements."""
    Q = len(world_map.points)
    ids = np.fromiter(world_map.points.keys(), np.int64, Q)
    pts = np.empty((Q, 3), np.float64)
    cnt = np.zeros(Q, np.int32)
    rows = np.zeros((Q, MAX_OBS_CHECK, stored), dtype)
    gather_rows(world_map.points.values(), pts, cnt, rows, width, uint8)
    return ids, pts, cnt, rows


def snapshot_map_points(world_map):
    """The float form: the 128-d descriptors (whatever their dtype, cast to float32) among the last six observations,
    valid ones first; count 0 when the LAST observation has none (pnp_utils.py:46-50 / :270-272)."""
    return _snapshot(world_map, np.float32, DESC_DIM, DESC_DIM, None)


def snapshot_map_points_binary(world_map, width: int):
    """The binary form: the uint8 rows of exactly `width` bytes, zero padded to 64.  A uint8 row of another width - the
    1-byte placeholder of triangulation_utils - is left out: the reference scores it `inf`."""
    return _snapshot(world_map, np.uint8, BIN_ROW, width, True)


def _float_map_refusal(world_map, width):
    """A binary frame found no uint8 row of its width in a non-empty map: refuse when the map holds float descriptors
    (the reference would return no match, every distance being `inf`); a map without any descriptor just has no match."""
    for mp in world_map.points.values():
        for _, _, d in mp.observations:
            if d is not None and np.asarray(d).dtype != np.uint8:
                raise NotImplementedError(
                    f"binary frame descriptors ({width} bytes) against a float-descriptor map: the reference matches "
                    "nothing there (every distance is inf); this backend refuses instead of returning an empty record")


@dataclass(frozen=True)
class _Form:
    """One descriptor form of the association: what differs between the float and the Hamming branch."""
    dtype: type                # of a descriptor element
    stored: int                # elements of a stored observation row
    binary: bool               # the native entries take the row width, and a map may hold no row of the frame's form
    dev: str                   # native entry on the SoA map's device arrays
    host: str                  # native entry on host arrays
    soa: str                   # the SoA map's host accessor ...
    device_arrays: str         # ... and its device accessor (a map that has it IS an SoA map)


_FLOAT = _Form(np.float32, DESC_DIM, False, "sslam_reproject_match_dev", "sslam_reproject_match_host", "soa", "device_arrays")
_HAMMING = _Form(np.uint8, BIN_ROW, True, "sslam_reproject_match_hamming_dev", "sslam_reproject_match_hamming_host",
                 "soa_binary", "device_arrays_binary")


def _associate(f, world_map, K, Tcw_pred, pts2d, des, img_w, img_h, radius_px, thr, ctx):
    """kp_of_point per map point for frame rows `des` [N][B] of form `f` -> (ids, positions, kp_of_point), or None where a
    binary frame finds no row of its form in the map.  Hamming (pnp_utils.py:264-266, `_desc_distance` :78-112): equal
    minima go to the lowest keypoint index."""
    P, lib, (N, B) = _native.ptr, _native.lib(), des.shape
    Kd, Td = np.ascontiguousarray(K, np.float64).reshape(9), np.ascontiguousarray(Tcw_pred, np.float64).reshape(16)
    soa = hasattr(world_map, f.device_arrays)
    if f.binary and soa and world_map.binary_width != B:
        if world_map.binary_width is None:
            _float_map_refusal(world_map, B)
            return None
        raise ValueError(f"reproject_and_match_2d3d: frame descriptors of {B} bytes against a map whose binary "
                         f"descriptors have {world_map.binary_width} bytes")
    ids, pts, cnt, rows = getattr(world_map, f.soa)() if soa else _snapshot(world_map, f.dtype, f.stored, B, f.binary or None)
    if f.binary and not cnt.any():
        _float_map_refusal(world_map, B)
        return None
    Q = len(ids)

    def call(entry, m_pos, m_cnt, m_rows, kp, frame, out, info, *n_kp_dev):
        _native.check(getattr(lib, entry)(
            ctx.handle, Q, P(m_pos), P(m_cnt), P(m_rows), P(Kd), P(Td), N, P(kp), P(frame), *((B,) if f.binary else ()),
            int(img_w), int(img_h), float(radius_px), float(thr), P(out), None, info, *n_kp_dev), entry)
    if soa:
        # SoA map (slam/core/landmark_utils.py of this overlay): its arrays already live on the GPU,
        # only the rows touched since the last call travel; no walk over the dict of objects
        d_map = getattr(world_map, f.device_arrays)(ctx)
        scr = _dev_scratch(ctx, Q, N)
        ctx.h2d(scr["kp"], pts2d); ctx.h2d(scr["des"], des)
        call(f.dev, *d_map, scr["kp"], scr["des"], scr["out"], P(scr["info"]),
             *((None,) if f.binary else ()))     # (n_kp_dev: every frame row uploaded here is live)
        out = np.empty(Q, np.int32); info4 = np.empty(4, np.int32)
        ctx.d2h(out, scr["out"]); ctx.d2h(info4, scr["info"])
        if info4[1]:
            raise _native.NativeError(f"more than the candidate capacity of keypoints within {radius_px} px of one projection")
    else:
        out = np.full(Q, -1, np.int32)
        call(f.host, pts, cnt, rows, pts2d, des, out, (C.c_int32 * 2)())
    return ids, pts, out


def reproject_and_match_2d3d(world_map, K, Tcw_pred, kps_cur, des_cur, img_w, img_h, radius_px: float = 12.0,
                             max_hamm: int = 64, max_l2: float = 0.8, use_cosine: bool = False, ctx=None):
    """Same signature and result as the reference.  Float descriptors: `use_cosine` changes nothing there either, the
    distance is always L2, only the threshold's name differs (pnp_utils.py:118).  uint8 descriptors of 2..64 bytes: the
    Hamming branch with `max_hamm`; where accepted minima tie, the lowest keypoint index wins (the reference's order
    is cKDTree's traversal order there).  A uint8 frame against a float-descriptor map raises NotImplementedError."""
    empty = Matches2D3D(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), [], [])
    if des_cur is None or len(des_cur) == 0 or not world_map.points:
        return empty
    pts2d = _kp_coords(kps_cur)
    if len(pts2d) == 0:
        return empty
    des = np.asarray(des_cur)
    if des.dtype == np.uint8:
        f, thr = _HAMMING, max_hamm
        des = np.ascontiguousarray(des).reshape(len(pts2d), -1)
        B = des.shape[1]
        if B > BIN_ROW:
            raise ValueError(f"reproject_and_match_2d3d: binary descriptors of {B} bytes; this backend covers 2..{BIN_ROW}")
        if B < 2:
            raise ValueError(f"reproject_and_match_2d3d: binary descriptors of {B} byte; this backend covers 2..{BIN_ROW}")
    else:
        f, thr = _FLOAT, max_l2
        des = np.ascontiguousarray(des, np.float32).reshape(len(pts2d), -1)
        if des.shape[1] != DESC_DIM:
            raise ValueError("reproject_and_match_2d3d expects 128-d descriptors")
    r = _associate(f, world_map, K, Tcw_pred, pts2d, des, img_w, img_h, radius_px, thr, ctx or _native.default_context())
    if r is None:
        return empty
    ids, pts, out = r
    hit = np.flatnonzero(out >= 0)
    if len(hit) == 0:
        return empty
    return Matches2D3D(pts[hit].astype(np.float32), pts2d[out[hit]].copy(), [int(i) for i in out[hit]],
                       [int(i) for i in ids[hit]])


def _dev_scratch(ctx, Q, N):
    """Device buffers of the current-frame inputs / outputs of the association, grown on demand.  They
    live ON the context object (`ctx.scratch`, released by `Context.close`): a module-level table keyed
    by `id(ctx)` would hand the pointers of a collected context to a new one that reuses the id."""
    cur = ctx.scratch.get("reproject")
    if cur is None or cur["Q"] < Q or cur["N"] < N:
        if cur is not None:
            ctx.sync()
            for p_ in cur["_ptrs"]:
                ctx.free(p_)
        Qc, Nc = max(Q, 2 * (cur["Q"] if cur else 0), 1024), max(N, (cur["N"] if cur else 0), 1024)
        cur = {"Q": Qc, "N": Nc, "kp": ctx.malloc(Nc * 8), "des": ctx.malloc(Nc * DESC_DIM * 4),
               "out": ctx.malloc(Qc * 4), "info": ctx.malloc(16)}
        cur["_ptrs"] = (cur["kp"], cur["des"], cur["out"], cur["info"])
        ctx.scratch["reproject"] = cur
    return cur


def _pnp_inputs(pts3d, pts2d):
    p3 = np.asarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.asarray(pts2d, np.float32).reshape(-1, 2)
    if len(p3) == 4:
        raise NotImplementedError("4 correspondences: OpenCV takes its P3P minimal solver there, which this backend "
                                  "does not cover (the tracker asks for >= --pnp_min_inliers, default 30)")
    return p3, p2


def solve_pnp_ransac(pts3d: np.ndarray, pts2d: np.ndarray, K: np.ndarray, ransac_px: float,
                     Tcw_init: Optional[np.ndarray] = None, iters: int = 200,
                     conf: float = 0.999, ctx=None) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """Same signature and result as the reference: (T_cw, inlier_mask) or (None, empty).  Only whether `Tcw_init` is
    given matters: OpenCV then starts its final refinement from the last RANSAC sample's pose (see pnp.py)."""
    if len(pts3d) < 4:
        return None, np.zeros((0,), dtype=bool)
    p3, p2 = _pnp_inputs(pts3d, pts2d)
    ok, T, mask, _ = _pnp.solve_pnp_ransac(p3, p2, K, float(ransac_px), float(conf), int(iters),
                                           use_guess=Tcw_init is not None, ctx=ctx)
    if not ok or int(mask.sum()) < 4:
        return None, np.zeros((len(p3),), dtype=bool)
    return T, mask


def refine_pose_pnp(K: np.ndarray, pts3d: np.ndarray, pts2d: np.ndarray, ransac_px: float = 2.0, ctx=None):
    """Same signature and result as the reference: (R, t) float64, or (None, None)."""
    p3 = np.asarray(pts3d, dtype=np.float32)
    p2 = np.asarray(pts2d, dtype=np.float32)
    if len(p3) < 4 or len(p2) < 4:
        return None, None
    p3, p2 = _pnp_inputs(p3, p2)
    ok, T, _, _ = _pnp.solve_pnp_ransac(p3, p2, K, float(ransac_px), 0.999, 200, use_guess=False, ctx=ctx)
    if not ok:
        return None, None
    return T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
