"""Deterministic small images for the SIFT tests: the generators of tests/orb_scenes.py (the block mosaic with blobs and
noise, the repeated tile, the constant image, the shifted pair) at the sizes the SIFT tests use, and a scene of stripes whose extrema tie exactly.
tests/sift_ref.py is their reference; `reference` caches a restatement run per (scene, size, parameters) so that the tests of
one module share it."""
import functools

import numpy as np

import sift_ref as R
from orb_scenes import constant, mosaic, shifted_pair, tiles  # noqa: F401  (shifted_pair is used by the tests)

H, W = 97, 131             # odd sides, a stride that is no multiple of 4; 7 octaves from 262 x 194 down to 4 x 3
HS, WS = 33, 41            # 5 octaves from 82 x 66 down to 5 x 4: the coarse ones are smaller than the blur radius

def stripes(h=H, w=W, seed=2):
    """every row the same: the DoG is constant along y, so every extremum along x EQUALS its neighbours above and below - exact
    ties, whatever the arithmetic - and whole columns are candidates (none survives the edge test: det = 0)"""
    rng = np.random.default_rng(seed)
    row = np.repeat(rng.integers(20, 236, -(-w // 6)), 6)[:w]
    return np.tile(row.astype(np.uint8), (h, 1))


SCENES = {"stripes": stripes, "mosaic_fine": functools.partial(mosaic, seed=3, block=4), "mosaic": mosaic, "mosaic3": functools.partial(mosaic, channels=3), "tiles": tiles, "constant": constant}


@functools.lru_cache(maxsize=None)
def image(name, h=H, w=W):
    img = SCENES[name](h, w)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name, h=H, w=W, **kw):
    """sift_ref.detect of a scene, computed once per parameter set and shared (do not modify)"""
    return R.detect(image(name, h, w), **kw)


# the end-to-end cases: scene, size, parameters
CASES = {
    "defaults": ("mosaic", H, W, {}),
    "small": ("mosaic", HS, WS, {}),
    "three_channels": ("mosaic3", HS, WS, {}),
    "layers_1": ("mosaic", H, W, dict(nOctaveLayers=1)),
    "layers_5": ("mosaic", HS, WS, dict(nOctaveLayers=5)),
    "contrast_rejects_most": ("mosaic", H, W, dict(contrastThreshold=0.3)),
    "contrast_rejects_none": ("mosaic", HS, WS, dict(contrastThreshold=0.004)),
    "edge_2": ("mosaic", H, W, dict(edgeThreshold=2)),
    "sigma_1_2": ("mosaic", H, W, dict(sigma=1.2)),
    "quota_cuts": ("mosaic", H, W, dict(nfeatures=10)),
    "quota_cuts_on_a_tie": ("mosaic", H, W, dict(nfeatures=40)),
    "tiles": ("tiles", H, W, dict(contrastThreshold=0.01)),
    "stripes_tie": ("stripes", HS, WS, {}),
    "duplicates": ("mosaic_fine", H, W, {}),
    "thin_12": ("mosaic", 12, W, {}),
    "no_interior_5x40": ("mosaic", 5, 40, {}),
    "constant": ("constant", HS, WS, {}),
}
