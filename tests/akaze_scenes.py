"""Deterministic small images for the AKAZE tests: the generators of tests/orb_scenes.py (the block mosaic with blobs and noise,
the repeated tile, the constant image, the shifted pair) at the smallest sizes at which each structure of the evolution
exists.  tests/akaze_ref.py is their reference; `reference` caches a restatement run per (scene, size, parameters) so that the
tests of one module share it."""
import functools

import akaze_ref as R
from orb_scenes import constant, mosaic, shifted_pair, tiles  # noqa: F401  (shifted_pair is used by the tests)

SCENES = {"mosaic": mosaic, "mosaic3": functools.partial(mosaic, channels=3), "mosaic_coarse": functools.partial(mosaic, seed=4, block=31),
          "tiles": tiles, "constant": constant}


@functools.lru_cache(maxsize=None)
def image(name, h, w):
    img = SCENES[name](h, w)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _reference(name, h, w, kw):
    return R.detect(image(name, h, w), **dict(kw))


def reference(name, h, w, **kw):
    """akaze_ref.detect of a scene, computed once per parameter set and shared (do not modify)"""
    return _reference(name, h, w, tuple(sorted(kw.items())))


# the end-to-end cases: scene, h, w, parameters
CASES = {
    "one_octave": ("mosaic", 61, 97, {}),                       # odd sides, a stride that is no multiple of 4; octave 1 would be 48 x 30
    "two_octaves": ("mosaic", 83, 163, {}),                     # octave 1 is 81 x 41, just above the cut; the halving of odd sides
    "cut_159x80": ("mosaic", 80, 159, {}),                      # 79 x 40: the width is below 80
    "cut_160x79": ("mosaic", 79, 160, {}),                      # 80 x 39: the height is below 40
    "cut_160x80": ("mosaic", 80, 160, {}),                      # 80 x 40: two octaves
    "three_octaves": ("mosaic", 161, 323, {}),
    "four_octaves_defaults": ("mosaic_coarse", 323, 643, {}),   # all 16 levels, 166 steps, both diffusion forms
    "octaves_1": ("mosaic", 83, 163, dict(nOctaves=1)),
    "layers_1": ("mosaic", 83, 163, dict(nOctaveLayers=1)),
    "layers_5": ("mosaic", 61, 97, dict(nOctaveLayers=5)),
    "threshold_rejects_most": ("mosaic", 61, 97, dict(threshold=0.02)),
    "threshold_rejects_none": ("mosaic", 61, 97, dict(threshold=1e-9)),
    "max_points_cuts": ("mosaic", 61, 97, dict(max_points=10)),
    "max_points_cuts_on_a_tie": ("tiles", 61, 97, dict(max_points=3)),
    "three_channels": ("mosaic3", 61, 97, {}),
    "tiles": ("tiles", 61, 97, {}),
    "constant": ("constant", 61, 97, {}),
    "thin_10": ("mosaic", 10, 97, {}),
}
