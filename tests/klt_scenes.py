"""Scenes of the pyramidal Lucas-Kanade tests: pairs of `frames.structured_frame` (a planted shift of 3 px in x, wrapping
around) whose top-left third is flat, and 150 points that also fall outside the image.  Four cases
(h, w, winSize (width, height), maxLevel) chosen for the pyramid's stop rule, odd sizes at every level, a non-square window and
a single level.  `outcomes(case)` counts the level-0 exits of the restatement; tests/test_klt_ref.py asserts that every branch
occurs in every case, so that none is left untested by accident."""
import functools

import numpy as np

import klt_ref as R
from frames import structured_frame

CASES = {
    "stop_at_2": (120, 160, (21, 21), 3),
    "odd_sizes": (97, 131, (21, 21), 3),
    "non_square": (61, 75, (9, 15), 2),
    "one_level": (48, 64, (5, 5), 0),
}
EFFECTIVE_LEVELS = {"stop_at_2": 2, "odd_sizes": 2, "non_square": 2, "one_level": 0}
N_POINTS = 150
SHIFT = 3
CRITERIA = (3, 30, 0.01)                 # cv2's default; the reference's front end runs (3, 30, 1e-3)
MAIN4 = dict(criteria=(3, 30, 1e-3), minEigThreshold=1e-4, err_thresh=12.0, fb_thresh=1.5)


def frame(idx, h, w, c=1):
    """structured_frame(idx) with the flat patch; c = 3 / 4 gives DISTINCT planes (the grey plane, its roll and its complement)."""
    f = structured_frame(idx, h, w, 1).copy()
    f[:h // 3, :w // 3] = 128
    if c == 1:
        return f
    planes = [f, np.roll(f, 7, axis=0), 255 - f, np.roll(f, 5, axis=1)][:c]
    return np.ascontiguousarray(np.stack(planes, -1))


def points(h, w, n=N_POINTS):
    rng = np.random.default_rng(5)
    x = rng.uniform(-2, w + 2, n)
    y = rng.uniform(-2, h + 2, n)
    return np.stack([x, y], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(frame0, frame1, points [150,2], winSize, maxLevel); the arrays are shared and read-only."""
    h, w, win, max_level = CASES[name]
    out = (frame(0, h, w), frame(1, h, w), points(h, w))
    for a in out:
        a.setflags(write=False)
    return out + (win, max_level)


@functools.lru_cache(maxsize=None)
def pyramids(name):
    f0, f1, _, win, max_level = scene(name)
    return R.Pyramid(f0, win, max_level), R.Pyramid(f1, win, max_level)


@functools.lru_cache(maxsize=None)
def forward(name, criteria=CRITERIA, flags=0):
    """The restatement's forward result of a case: (next_pts, status, err, exits), computed once and shared."""
    p0, p1 = pyramids(name)
    _, _, pts, win, max_level = scene(name)
    out = R.calc_optical_flow_pyr_lk(p0, p1, pts, None, winSize=win, maxLevel=max_level, criteria=criteria, flags=flags,
                                     return_exits=True)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def backward(name, criteria=CRITERIA, flags=0):
    p0, p1 = pyramids(name)
    _, _, _, win, max_level = scene(name)
    nxt = forward(name, criteria, flags)[0]
    out = R.calc_optical_flow_pyr_lk(p1, p0, nxt, None, winSize=win, maxLevel=max_level, criteria=criteria, flags=flags,
                                     return_exits=True)
    for a in out:
        a.setflags(write=False)
    return out


def outcomes(name):
    """{exit reason: count} at level 0 of the forward pass."""
    ex = forward(name)[3]
    return {int(k): int((ex == k).sum()) for k in np.unique(ex)}
