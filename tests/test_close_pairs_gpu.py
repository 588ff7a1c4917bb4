"""`sslam_close_pairs_host` / `_dev` (landmark_fusion.close_pairs) against `sorted(cKDTree(p).query_pairs(r))`, the search
inside `Map.fuse_closeby_duplicate_landmarks`: sizes 0, 1, 2, one 256-point tile less one / exactly / plus one and three tiles
(513), duplicates planted inside a tile, between tiles 0 and 1 and between tiles 0 and 2.  Equality of the pair LISTS can
only be asked when no pair sits on the radius, so each case first asserts on the CPU that no distance lies within 1e-9
relative of r (the two sides round dx^2 + dy^2 + dz^2 differently by a few 1e-16)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from conftest import load_pkg

pytestmark = pytest.mark.gpu

RADIUS = 0.05
PLANTED = ((10, 20), (100, 300), (5, 512), (255, 256), (0, 1))      # inside tile 0, tiles 0-1, tiles 0-2, across the tile edge


def cloud(n, seed=3):
    """n points in a 3 m box (a few natural pairs within RADIUS at n = 513) + the planted near-duplicates that fit"""
    rng = np.random.default_rng(seed + n)
    p = rng.uniform(0.0, 3.0, (n, 3))
    for a, b in PLANTED:
        if b < n:
            d = rng.standard_normal(3)
            p[b] = p[a] + d / np.linalg.norm(d) * RADIUS * rng.uniform(0.1, 0.8)
    return p


def expected(p, r):
    if len(p) < 2:
        return np.empty((0, 2), np.int32)
    i, j = np.triu_indices(len(p), 1)
    d = np.linalg.norm(p[i] - p[j], axis=1)
    assert (np.abs(d - r) > 1e-9 * r).all()                  # no pair on the radius
    return np.array(sorted(cKDTree(p).query_pairs(r)), np.int32).reshape(-1, 2)


@pytest.fixture(scope="module")
def fusion():
    return load_pkg("landmark_fusion")


@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513])
def test_pairs_equal_the_kd_tree(fusion, gpu_ctx, n):
    p = cloud(n)
    want = expected(p, RADIUS)
    planted = sum(b < n for _, b in PLANTED)
    assert len(want) >= planted
    got = fusion.close_pairs(p, RADIUS, ctx=gpu_ctx)
    print(f"n = {n}: {len(got)} pairs ({planted} planted)")
    assert got.dtype == np.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_three_hundred_identical_points(fusion, gpu_ctx):
    """more pairs than the first run's default buffer (1200 slots): the exact count sizes the second run"""
    p = np.tile([[0.25, -1.5, 7.0]], (300, 1))
    got = fusion.close_pairs(p, RADIUS, ctx=gpu_ctx)
    assert len(got) == 44850
    i, j = np.triu_indices(300, 1)
    np.testing.assert_array_equal(got, np.column_stack([i, j]).astype(np.int32))


def test_a_small_buffer_takes_the_second_run(fusion, gpu_ctx):
    p = cloud(513)
    want = expected(p, RADIUS)
    assert len(want) > 4
    np.testing.assert_array_equal(fusion.close_pairs(p, RADIUS, ctx=gpu_ctx, pair_capacity=4), want)
    np.testing.assert_array_equal(fusion.close_pairs(p, RADIUS, ctx=gpu_ctx, pair_capacity=0), want)


def test_a_non_finite_coordinate_pairs_with_nothing(fusion, gpu_ctx):
    p = cloud(257)
    want = expected(p, RADIUS)
    q = p.copy()
    q[10, 1] = np.nan
    q[100] = np.inf
    keep = ~np.isin(want, (10, 100)).any(axis=1)
    assert keep.sum() < len(want)
    np.testing.assert_array_equal(fusion.close_pairs(q, RADIUS, ctx=gpu_ctx), want[keep])


def test_the_device_pointer_entry_on_an_overlay_map(fusion, gpu_ctx):
    lmu = load_pkg("slam.core.landmark_utils")
    p = cloud(513)
    m = lmu.Map()
    ids = m.add_points(p)
    m.points.pop(ids[7])                                     # a hole: the rows are compacted before they are read
    rows = np.delete(p, 7, axis=0)
    want = expected(rows, RADIUS)
    np.testing.assert_array_equal(fusion.close_pairs(m, RADIUS, ctx=gpu_ctx), want)
    np.testing.assert_array_equal(fusion.close_pairs(rows, RADIUS, ctx=gpu_ctx), want)


def test_more_than_2_to_the_24_pairs_is_an_error(fusion, gpu_ctx):
    n = 5800                                                 # n (n - 1) / 2 = 16 817 100 > 2^24 = 16 777 216
    with pytest.raises(ValueError, match="16817100"):
        fusion.close_pairs(np.zeros((n, 3)), RADIUS, ctx=gpu_ctx)


def test_bad_arguments_are_errors(fusion, gpu_ctx):
    with pytest.raises(ValueError):
        fusion.close_pairs(cloud(10), -1.0, ctx=gpu_ctx)
    with pytest.raises(ValueError):
        fusion.close_pairs(cloud(10), np.nan, ctx=gpu_ctx)
