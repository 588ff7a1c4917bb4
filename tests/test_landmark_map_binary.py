"""The binary mirror of the overlay's SoA map (slam/core/landmark_utils.py: `_binary`, `binary_width`,
`soa_binary`, `device_arrays_binary`): after every kind of mutation it equals what a walk over the dict of objects
rebuilds (pnp_utils.snapshot_map_points_binary), it follows the reference's skip rule, it travels to the device by
touched rows with a dirty range of its own, and a float-only map is what it was before the mirror existed.  The device
is tests/fake_device.py: host logic only, no GPU."""
import types

import numpy as np
import pytest

import map_ops
from conftest import load_pkg
from fake_device import FakeContext

B = 32


class RecordingContext(FakeContext):
    """A FakeContext that remembers every upload as (address, bytes)."""

    def __init__(self):
        super().__init__()
        self.uploads = []

    def h2d(self, dptr, arr):
        self.uploads.append((int(dptr), np.ascontiguousarray(arr).nbytes))
        super().h2d(dptr, arr)


@pytest.fixture()
def L():
    return load_pkg("slam.core.landmark_utils")


@pytest.fixture()
def P():
    return load_pkg("slam.core.pnp_utils")


def rows(rng, n=None, width=B):
    return rng.integers(0, 256, (width,) if n is None else (n, width), dtype=np.uint8)


def check(m, P, width=B):
    """Arrays, dict and a fresh walk over the objects agree; rows are zero beyond the width and beyond the count."""
    ids, pos, cnt, brows = m.soa_binary()
    w_ids, w_pos, w_cnt, w_rows = P.snapshot_map_points_binary(m, width)
    assert len(ids) == len(m) == len(m.points)
    np.testing.assert_array_equal(ids, np.fromiter(m.points.keys(), np.int64))
    np.testing.assert_array_equal(ids, w_ids); np.testing.assert_array_equal(pos, w_pos)
    np.testing.assert_array_equal(cnt, w_cnt)
    assert brows.dtype == np.uint8 and brows.shape == (len(ids), 6, 64)
    for q in range(len(ids)):
        np.testing.assert_array_equal(brows[q, :cnt[q]], w_rows[q, :cnt[q]])
        assert not brows[q, :cnt[q], width:].any()
    return ids, pos, cnt, brows


def test_mirror_follows_every_mutation(L, P):
    rng = np.random.default_rng(5)
    m = L.Map()
    assert m.binary_width is None
    ids = m.add_points(rng.uniform(-1, 1, (40, 3)))
    assert m.binary_width is None and not m.soa_binary()[2].any()
    for j, pid in enumerate(ids):
        for f in range(j % 9):                                          # up to 8 observations: the last six count
            m.points[pid].add_observation(f, j, rows(rng))
    assert m.binary_width == B
    _, _, cnt, brows = check(m, P)
    assert cnt.max() == 6 and (cnt == 0).any()
    last = np.asarray(m.points[ids[8]].observations[-1][2])             # 8 observations: rows are observations 2..7
    np.testing.assert_array_equal(brows[8, 5, :B], last)
    np.testing.assert_array_equal(brows[8, 0, :B], m.points[ids[8]].observations[2][2])
    # the float arrays of such a map hold nothing
    assert not m.soa()[2].any()
    # points.pop / del: holes compacted away (triangulation_utils.py:105)
    m.points.pop(ids[7], None)
    del m.points[ids[0]]
    check(m, P)
    # a foreign landmark object (the reference's dataclass shape) is adopted with its observations
    foreign = types.SimpleNamespace(id=100000, position=np.array([1.0, 2.0, 3.0]), keyframe_idx=3,
                                    observations=[(0, 1, rows(rng)), (1, 2, None), (2, 3, rows(rng))])
    m.points[100000] = foreign
    ids_now, _, cnt, brows = check(m, P)
    assert ids_now[-1] == 100000 and cnt[-1] == 2
    np.testing.assert_array_equal(brows[-1, 1, :B], foreign.observations[2][2])
    # a free-standing MapPoint with observations replaces an existing key in place
    mp = L.MapPoint(ids[3], np.array([0.5, 0.5, 0.5]))
    mp.add_observation(4, 4, rows(rng))
    m.points[ids[3]] = mp
    assert list(m.points.keys())[2] == ids[3]
    _, _, cnt, _ = check(m, P)
    assert cnt[2] == 1
    # the duplicate merge removes a landmark and compacts
    m.points[ids[10]].position = m.points[ids[11]].position + 1e-3
    before = len(m)
    m.fuse_closeby_duplicate_landmarks(0.05)
    assert len(m) == before - 1 and ids[11] not in m.points
    check(m, P)
    # growth past the initial capacity keeps the rows
    keep = m.soa_binary()[3][:5].copy()
    big = m.add_points(rng.uniform(-1, 1, (3000, 3)))
    assert len(m._binary.cnt) >= len(m) > 1024 and len(m._binary.rows) == len(m._binary.cnt)
    m.points[big[-1]].add_observation(9, 9, rows(rng))
    _, _, cnt, brows = check(m, P)
    np.testing.assert_array_equal(brows[:5], keep)
    assert cnt[-1] == 1 and not cnt[-3000:-1].any()
    m.points.clear()
    assert len(m.soa_binary()[0]) == 0 and m.binary_width == B         # the width stays fixed


def test_from_reference_and_resync(L, P):
    import reproject_hamming_scenes as HS
    for case in (HS.CASES[4], HS.CASES[3][:1] + (60, 50) + HS.CASES[3][3:]):     # B = 32, and the odd 61
        sc = HS.make_case(*case)
        m = L.Map.from_reference(sc["wmap"])
        assert m.binary_width == sc["B"]
        _, _, cnt, _ = check(m, P, sc["B"])
        assert cnt.max() == 6 and (cnt == 0).any()
    # resync after observations were appended directly
    pid = m.point_ids()[0]
    m.points[pid].observations.append((50, 50, np.full(61, 255, np.uint8)))
    m.resync()
    _, _, cnt, brows = check(m, P, 61)
    assert cnt[0] >= 1 and (brows[0, cnt[0] - 1, :61] == 255).all() and not brows[0, cnt[0] - 1, 61:].any()


def test_last_observation_none_rule(L, P):
    rng = np.random.default_rng(6)
    m = L.Map()
    a, b = m.add_points(np.zeros((2, 3)))
    for f in range(3):
        m.points[a].add_observation(f, 0, rows(rng))
        m.points[b].add_observation(f, 0, rows(rng))
    m.points[a].observations.insert(1, (9, 9, None))                    # a None in the middle is only skipped
    m.points[b].observations.append((9, 9, None))                       # a None LAST empties the point
    m.resync()
    _, _, cnt, _ = check(m, P)
    assert list(cnt) == [3, 0]
    m.points[b].add_observation(10, 0, rows(rng))                       # a descriptor last again: the None in between is skipped
    assert list(check(m, P)[2]) == [3, 4]


def test_rows_of_another_width_are_not_mirrored(L, P):
    rng = np.random.default_rng(7)
    m = L.Map()
    a, b, c = m.add_points(np.zeros((3, 3)))
    m.points[a].add_observation(0, 0, np.zeros(1, np.uint8))            # the 1-byte placeholder of triangulation_utils: fixes nothing
    assert m.binary_width is None and m.soa_binary()[2][0] == 0
    m.points[a].add_observation(1, 0, np.zeros(65, np.uint8))           # wider than a stored row: fixes nothing either
    assert m.binary_width is None
    m.points[a].add_observation(2, 0, rows(rng))                        # the first row of 2..64 bytes fixes the width
    assert m.binary_width == B
    m.points[b].add_observation(0, 0, rows(rng, width=61))              # another width: stored in the list, not mirrored
    m.points[b].add_observation(1, 0, rows(rng))
    m.points[c].add_observation(0, 0, rows(rng, width=16))
    m.points[c].add_observation(1, 0, np.zeros(1, np.uint8))            # a placeholder LAST is a descriptor (not None): the point keeps its rows
    assert m.binary_width == B
    _, _, cnt, brows = check(m, P)
    assert list(cnt) == [1, 1, 0]
    np.testing.assert_array_equal(brows[1, 0, :B], m.points[b].observations[1][2])
    assert len(m.points[b].observations) == 2
    # float and binary observations on one landmark go to their own mirrors
    m.points[c].add_observation(2, 0, rng.standard_normal(128).astype(np.float32))
    m.points[c].add_observation(3, 0, rows(rng))
    assert m.soa()[2][2] == 1 and m.soa_binary()[2][2] == 1
    check(m, P)


def test_device_mirror_uploads_only_touched_rows(L):
    rng = np.random.default_rng(8)
    ctx = RecordingContext()
    m = L.Map()
    ids = m.add_points(rng.uniform(-1, 1, (100, 3)))
    for pid in ids:
        m.points[pid].add_observation(0, 0, rows(rng))
    row_bytes = 6 * 64
    d_pos, d_cnt, d_rows = m.device_arrays_binary(ctx)
    n = len(ids)
    assert (d_rows, n * row_bytes) in ctx.uploads and (d_pos, n * 24) in ctx.uploads and (d_cnt, n * 4) in ctx.uploads
    np.testing.assert_array_equal(ctx.view(d_rows, n * row_bytes), m.soa_binary()[3].reshape(-1))
    np.testing.assert_array_equal(ctx.i32(d_cnt, n), m.soa_binary()[2])
    # nothing touched: positions and counts only
    ctx.uploads.clear()
    assert m.device_arrays_binary(ctx) == (d_pos, d_cnt, d_rows)
    assert sorted(ctx.uploads) == sorted([(d_pos, n * 24), (d_cnt, n * 4)])
    # two touched rows: exactly their range travels
    m.points[ids[40]].add_observation(1, 1, rows(rng))
    m.points[ids[43]].add_observation(1, 1, rows(rng))
    ctx.uploads.clear()
    m.device_arrays_binary(ctx)
    assert (d_rows + 40 * row_bytes, 4 * row_bytes) in ctx.uploads and len(ctx.uploads) == 3
    np.testing.assert_array_equal(ctx.view(d_rows, n * row_bytes), m.soa_binary()[3].reshape(-1))
    # a float upload in between must not clear the binary dirty range (and the other way round)
    m.points[ids[7]].add_observation(2, 2, rows(rng))
    m.points[ids[7]].add_observation(3, 3, rng.standard_normal(128).astype(np.float32))
    f_pos, f_cnt, f_desc = m.device_arrays(ctx)
    assert f_desc != d_rows and f_pos != d_pos
    ctx.uploads.clear()
    m.device_arrays_binary(ctx)
    assert (d_rows + 7 * row_bytes, row_bytes) in ctx.uploads
    np.testing.assert_array_equal(ctx.view(d_rows, n * row_bytes), m.soa_binary()[3].reshape(-1))
    m.points[ids[9]].add_observation(4, 4, rng.standard_normal(128).astype(np.float32))
    m.device_arrays_binary(ctx)
    ctx.uploads.clear()
    m.device_arrays(ctx)
    assert (f_desc + 9 * 6 * 128 * 4, 6 * 128 * 4) in ctx.uploads
    np.testing.assert_array_equal(ctx.f32(f_desc, n * 6 * 128), m.soa()[3].reshape(-1))
    # growth past the capacity reallocates and uploads everything
    m.add_points(rng.uniform(-1, 1, (2000, 3)))
    ctx.uploads.clear()
    g_pos, g_cnt, g_rows = m.device_arrays_binary(ctx)
    assert g_rows != d_rows and (g_rows, len(m) * row_bytes) in ctx.uploads
    np.testing.assert_array_equal(ctx.view(g_rows, len(m) * row_bytes), m.soa_binary()[3].reshape(-1))


def test_float_only_map_is_unchanged(L, P):
    """A map that never saw a uint8 descriptor: the float arrays and `soa()` are those of a walk over the objects (the
    code that has not changed), byte for byte, the binary mirror is empty and no width is fixed."""
    m = map_ops.run(L.Map())
    ids, pos, cnt, desc = m.soa()
    w_ids, w_pos, w_cnt, w_desc = P.snapshot_map_points(m)
    for a, b in ((ids, w_ids), (pos, w_pos), (cnt, w_cnt)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert desc.dtype == np.float32 and desc.shape == (len(ids), 6, 128)
    for q in range(len(ids)):
        assert desc[q, :cnt[q]].tobytes() == w_desc[q, :cnt[q]].tobytes()
    assert m.binary_width is None and not m.soa_binary()[2].any() and not m.soa_binary()[3].any()
    assert len(m.soa()) == 4
    ctx = RecordingContext()
    d_pos, d_cnt, d_desc = m.device_arrays(ctx)
    n = len(ids)
    assert sorted(ctx.uploads) == sorted([(d_pos, n * 24), (d_cnt, n * 4), (d_desc, n * 6 * 128 * 4)])
    assert ctx.view(d_desc, n * 6 * 128 * 4).tobytes() == m.soa()[3].tobytes()
