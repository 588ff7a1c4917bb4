"""Landmark fusion with the pair search on the HIP backend.

`close_pairs` stands in for `cKDTree(points).query_pairs(radius)` of `Map.fuse_closeby_duplicate_landmarks`
(slam/core/landmark_utils.py:138-161): every (i, j), i < j, within `radius` (closed), sorted.  `fuse_closeby` applies that
method's greedy rule to the pairs - sorted, the lower row absorbs, positions averaged on the host, the absorbed landmark
popped - on the overlay's `Map` (positions read from its device mirror) and on a plain dict-of-objects map.
There is no CPU fallback: the search is the device call or an error.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native

MAX_PAIRS = 1 << 24              # more pairs than this is not a map with duplicates but a wrong radius


def _is_overlay_map(m) -> bool:
    return hasattr(m, "device_arrays") and hasattr(m, "points") and hasattr(m, "_n")


def close_pairs(points_or_map, radius: float, ctx=None, pair_capacity: int | None = None) -> np.ndarray:
    """Sorted [m,2] int32 pairs (i < j) of rows within `radius` of each other.  `points_or_map`: an [n,3] array (uploaded),
    or the overlay's `Map` (rows of its arrays in dict order, read from its device mirror).  `pair_capacity` sizes the
    first run's buffer (default 4 n, at least 1024); when the map holds more pairs, the exact count the first run
    returns sizes a second one."""
    ctx = ctx or _native.default_context()
    radius = float(radius)
    if not np.isfinite(radius) or radius < 0:
        raise ValueError("radius must be finite and >= 0")
    lib = _native.lib()
    P = _native.ptr
    if _is_overlay_map(points_or_map):
        d_pos = points_or_map.device_arrays(ctx)[0]
        n = int(points_or_map._n)
        entry, name, pos = lib.sslam_close_pairs_dev, "sslam_close_pairs_dev", int(d_pos)
    else:
        pos = np.ascontiguousarray(points_or_map, np.float64).reshape(-1, 3)
        n = len(pos)
        entry, name = lib.sslam_close_pairs_host, "sslam_close_pairs_host"
    if n < 2:
        return np.empty((0, 2), np.int32)
    cap = max(4 * n, 1024) if pair_capacity is None else int(pair_capacity)
    if cap < 0:
        raise ValueError("pair_capacity must be >= 0")
    cap = min(cap, MAX_PAIRS)
    count = C.c_int64(0)
    for _ in range(2):
        pairs = np.empty((max(cap, 1), 2), np.int32)
        _native.check(entry(ctx.handle, n, P(pos), radius, cap, P(pairs), C.byref(count)), name)
        m = int(count.value)
        if m > MAX_PAIRS:
            raise ValueError(f"{m} pairs within radius {radius} (more than {MAX_PAIRS}): not a fusion radius for this map")
        if m <= cap:
            break
        cap = m
    else:
        raise _native.NativeError(f"{name}: the pair count changed between two runs on the same points")
    pairs = pairs[:m]
    return np.ascontiguousarray(pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))])


def fuse_closeby(world_map, radius: float, ctx=None) -> None:
    """`Map.fuse_closeby_duplicate_landmarks(radius)` with the pair search on the device: the same pairs in the same
    order through the same greedy rule, so the same map.  A plain dict-of-objects map needs `points` and
    `get_point_array()` (rows in dict order)."""
    if len(world_map.points) < 2:
        return
    overlay = _is_overlay_map(world_map)
    if overlay:
        world_map._compact()
        pairs = close_pairs(world_map, radius, ctx)
    else:
        pairs = close_pairs(np.asarray(world_map.get_point_array(), np.float64).reshape(-1, 3), radius, ctx)
    ids = list(world_map.points.keys())
    removed = set()
    for i, j in pairs.tolist():
        ida, idb = ids[i], ids[j]
        if idb in removed or ida in removed:
            continue
        world_map.points[ida].position = (world_map.points[ida].position + world_map.points[idb].position) * 0.5
        removed.add(idb)
    for idx in removed:
        world_map.points.pop(idx, None)
    if overlay:
        world_map._compact()
