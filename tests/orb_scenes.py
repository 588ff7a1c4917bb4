"""Deterministic small images for the ORB tests: mosaics of small blocks (checker corners of varied contrast), seeded noise
blobs, a repeated tile whose scores tie, a constant image.  tests/orb_ref.py is their reference; `reference` caches a
restatement run per (scene, parameters) so that the tests of one module share it."""
import functools

import numpy as np

import orb_ref as R

H, W = 97, 131             # odd sides, a stride that is no multiple of 4


def mosaic(h=H, w=W, seed=1, block=5, channels=1):
    """blocks of `block` pixels with intensities from a few levels (corners of every contrast from 8 to 200), smooth seeded
    blobs on top and +-2 of noise"""
    rng = np.random.default_rng(seed)
    levels = np.array([20, 28, 60, 90, 140, 220], np.float64)
    by, bx = -(-h // block), -(-w // block)
    img = np.kron(levels[rng.integers(0, len(levels), (by, bx))], np.ones((block, block)))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(6):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, 9), rng.uniform(-50, 50)
        img = img + a * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    img = img + rng.integers(-2, 3, (h, w))
    g = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if channels == 1:
        return g
    # three channels whose fixed-point grey is not simply one of them
    out = np.stack([np.roll(g, 1, axis=1), g, np.roll(g, 1, axis=0)], axis=2)
    return np.ascontiguousarray(out)


def tiles(h=H, w=W, period=12):
    """a repeated tile: a bright pixel on a dimmer 3 x 3 pad on a dark ground every `period` pixels - the pixel is a strict
    maximum of the FAST score, and every repetition away from the edge has the same score and the same response"""
    t = np.full((period, period), 30, np.uint8)
    t[4:7, 4:7] = 120
    t[5, 5] = 200
    t[5, 6] = 130                      # (not symmetric: the orientation is defined)
    return np.tile(t, (-(-h // period), -(-w // period)))[:h, :w].copy()


def constant(h=H, w=W, v=77):
    return np.full((h, w), v, np.uint8)


def shifted_pair(h=120, w=160, dx=7, dy=4, seed=5):
    """two crops of one mosaic, the second moved by (dx, dy): a keypoint at (x, y) of the first is at (x - dx, y - dy) of the
    second wherever both see it"""
    big = mosaic(h + dy, w + dx, seed)
    return big[:h, :w].copy(), big[dy:dy + h, dx:dx + w].copy()


SCENES = {"mosaic": mosaic, "mosaic3": functools.partial(mosaic, channels=3), "tiles": tiles, "constant": constant}


@functools.lru_cache(maxsize=None)
def image(name, h=H, w=W):
    img = SCENES[name](h, w)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name, h=H, w=W, **kw):
    """orb_ref.detect of a scene, computed once per parameter set and shared (do not modify)"""
    return R.detect(image(name, h, w), **kw)
