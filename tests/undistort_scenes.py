"""Cameras, sizes, images and hand-made maps of the undistortion tests (CPU and GPU).  Sizes are the smallest that reach each
path of the remap kernel (a lane owns four consecutive destination pixels; the last H W mod 4 take a byte path)."""
import numpy as np

# calibrations at 640 x 480: (fx, fy, cx, cy), D
CAMERAS = {
    # the public TUM RGB-D freiburg1 calibration (ROS default of the dataset's web page)
    "tum_fr1": ((517.3, 516.5, 318.6, 255.3), [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]),
    "barrel": ((420.0, 418.0, 322.5, 238.5), [-0.32, 0.11, 0.0008, -0.0006, -0.018]),
    "pincushion": ((600.0, 602.0, 315.0, 244.0), [0.18, 0.05, -0.0012, 0.0009]),
    "rational8": ((480.0, 481.0, 320.5, 241.5), [0.85, 0.31, 0.0011, -0.0007, 0.021, 1.15, 0.52, 0.055]),
    "zero": ((500.0, 505.0, 319.5, 239.5), [0.0, 0.0, 0.0, 0.0]),
}
BARREL = ("barrel", "rational8")         # cameras whose undistorted image covers the viewport at alpha = 0
ALPHAS = (0.0, 1.0)

# W x H of the remap tests
SIZES = [(1, 1), (3, 1), (5, 3),         # byte tails only (fewer than four pixels ... one quad + tail for 5 x 3)
         (4, 1),                         # exactly one quad, no tail
         (37, 23),                       # H W odd, W C no multiple of 4 for any C
         (64, 4),                        # one full workgroup of quads
         (161, 97),                      # several workgroups, tail of 1
         (640, 480)]
MAP_SIZE = (161, 97)                     # every camera x alpha runs at this size
CHANNELS = (1, 3, 4)


def camera(name, size):
    """-> (K [3,3], D) of `name` scaled from 640 x 480 to `size` = (W, H)"""
    (fx, fy, cx, cy), D = CAMERAS[name]
    sx, sy = size[0] / 640.0, size[1] / 480.0
    K = np.array([[fx * sx, 0, (cx + 0.5) * sx - 0.5], [0, fy * sy, (cy + 0.5) * sy - 0.5], [0, 0, 1]])
    return K, np.array(D, np.float64)


def has_optimal_matrix(size):
    """the 9 x 9 grid of getOptimalNewCameraMatrix degenerates on an image one pixel wide or high: those sizes run with
    new_K = K"""
    return min(size) >= 16


def image(size, C, seed=0):
    W, H = size
    rng = np.random.default_rng(1000 * seed + 10 * W + H + C)
    return rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)


# ---- hand-made maps: a 13 x 7 destination over an 11 x 9 source ------------------------------------------------------
HAND_DST = (13, 7)
HAND_SRC = (11, 9)
CATEGORIES = ("integer", "tie_down", "tie_up", "below_zero", "above_last", "at_zero", "at_last", "far", "beyond_int32", "inf", "nan")


def hand_values(last):
    """coordinate values per category for an axis whose last source index is `last`"""
    return {
        "integer": [1.0, 2.0, 5.0, float(last - 1)],
        "tie_down": [2 + 1 / 64, 4 + 1 / 64, 0 + 1 / 64],       # x 32 = k 32 + 0.5: rounds to the even k 32
        "tie_up": [2 + 3 / 64, 6 + 3 / 64, 1 + 3 / 64],         # x 32 = k 32 + 1.5: rounds to the even k 32 + 2
        "below_zero": [-0.5, -0.25, -0.96875, -0.03125],
        "above_last": [last + 0.5, last + 0.25, last + 0.96875],
        "at_zero": [0.0],
        "at_last": [float(last)],
        "far": [1e6, -1e6],
        "beyond_int32": [3e8, -3e8],
        "inf": [np.inf, -np.inf],
        "nan": [np.nan],
    }


def classify(v, last):
    """the category of one float32 coordinate, or None for an ordinary fractional one"""
    v = float(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "inf"
    if abs(v * 32) >= 2.0 ** 31:
        return "beyond_int32"
    if abs(v) >= 32768:
        return "far"
    if v == 0:
        return "at_zero"
    if v == last:
        return "at_last"
    if -1 < v < 0:
        return "below_zero"
    if last < v < last + 1:
        return "above_last"
    t = v * 32
    if t - np.floor(t) == 0.5:
        return "tie_down" if int(np.floor(t)) % 2 == 0 else "tie_up"
    if v == np.floor(v):
        return "integer"
    return None


def hand_maps():
    """-> (mapx, mapy) float32 [7, 13]: every category on each axis, against ordinary values on the other axis, and the
    special ones against each other"""
    W, H = HAND_DST
    rng = np.random.default_rng(7)
    mapx = rng.uniform(0.3, HAND_SRC[0] - 1.3, (H, W)).astype(np.float32)
    mapy = rng.uniform(0.3, HAND_SRC[1] - 1.3, (H, W)).astype(np.float32)
    vx, vy = hand_values(HAND_SRC[0] - 1), hand_values(HAND_SRC[1] - 1)
    flat_x = [v for c in CATEGORIES for v in vx[c]]
    flat_y = [v for c in CATEGORIES for v in vy[c]]
    fx, fy = mapx.reshape(-1), mapy.reshape(-1)
    n = len(flat_x)
    assert 2 * n + 8 <= fx.size
    fx[:n] = flat_x                                      # x special, y ordinary
    fy[n:n + len(flat_y)] = flat_y                       # y special, x ordinary
    o = n + len(flat_y)
    for j, (a, b) in enumerate([(-0.5, -0.5), (HAND_SRC[0] - 0.5, HAND_SRC[1] - 0.5), (np.nan, 2.0), (2.0, np.inf),
                                (3e8, -3e8), (0.0, 0.0), (HAND_SRC[0] - 1.0, HAND_SRC[1] - 1.0), (1e6, 1 + 1 / 64)]):
        fx[o + j], fy[o + j] = a, b                      # corners and special against special
    return mapx, mapy


def assert_categories(mapx, mapy):
    """every category occurs on both axes (a scene cannot quietly stop reaching a branch)"""
    for m, last in ((mapx, HAND_SRC[0] - 1), (mapy, HAND_SRC[1] - 1)):
        seen = {classify(v, last) for v in m.reshape(-1)}
        missing = [c for c in CATEGORIES if c not in seen]
        assert not missing, missing
