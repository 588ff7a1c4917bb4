"""Scenes and parameter sets of the stereo tests: small pairs with a planted disparity, and the sizes at which the kernels of
csrc/stereo_kernels.hip take another path (one wave of paths, a lone computed column, fewer rows than the block, diagonals that
leave through the side, every lane split of the path kernel)."""
import numpy as np

# (W, H, D, blockSize, d0): the planted-constant cases that the restatement must solve within half a pixel
PLANTED = [(96, 32, 16, 5, 6), (97, 33, 32, 11, 13), (80, 24, 32, 3, 0), (80, 24, 32, 3, 31)]


def planted_pair(W, H, D, d0, seed=0, channels=1):
    """left = T[:, :W], right = T[:, d0:d0 + W] of uniform noise T: the left pixel x shows the right pixel x - d0"""
    rng = np.random.default_rng(seed)
    shape = (H, W + D) if channels == 1 else (H, W + D, channels)
    T = rng.integers(0, 256, shape, dtype=np.uint8)
    return np.ascontiguousarray(T[:, :W]), np.ascontiguousarray(T[:, d0:d0 + W])


def planted_params(D, bs, **kw):
    return dict(dict(minDisparity=0, numDisparities=D, blockSize=bs, P1=8 * bs * bs, P2=32 * bs * bs), **kw)


def two_plane_pair(W=128, H=40, D=32, seed=1):
    """background at disparity 4, a block 20 columns wide over the full height at disparity 20 -> (left, right, truth [H, W])"""
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (H, W + D), dtype=np.uint8)
    x0 = 70
    truth = np.full((H, W), 4, np.int32)
    truth[:, x0:x0 + 20] = 20
    xs = np.arange(W)[None, :] + D                              # the left image is cut from the columns D .. D + W of the right canvas
    left = np.take_along_axis(right, xs - truth, 1)
    return np.ascontiguousarray(left), np.ascontiguousarray(right[:, D:D + W]), truth


def smooth_pair(W, H, d0, seed=0):
    """a low-contrast textured pair (many near-ties), the right image the left shifted by d0 with fresh noise of one grey level"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W + d0]
    base = 120 + 60 * np.sin(xx / 5.0 + yy / 9.0) + 30 * np.cos(xx / 2.3 - yy / 3.1) + rng.integers(-6, 7, (H, W + d0))
    T = np.clip(base, 0, 255).astype(np.uint8)
    noise = rng.integers(-1, 2, (H, W))
    return np.ascontiguousarray(T[:, :W]), np.clip(T[:, d0:d0 + W].astype(np.int32) + noise, 0, 255).astype(np.uint8)


def _p(D, bs, **kw):
    return dict(dict(numDisparities=D, blockSize=bs), **kw)


def gpu_cases():
    """name -> (left, right, StereoSGBM_create keywords)"""
    cases = {}
    for W, H, D, bs, d0 in PLANTED:
        cases[f"planted_{W}x{H}_D{D}_bs{bs}_d{d0}"] = (*planted_pair(W, H, D, d0), planted_params(D, bs))
    l, r, _ = two_plane_pair()
    cases["two_plane"] = (l, r, planted_params(32, 5))
    for extra in (1, 63, 65):                                   # path kernels at and around one wave of computed columns
        cases[f"W_maxD_plus_{extra}"] = (*planted_pair(16 + extra, 9, 16, 3, seed=extra), _p(16, 3, P1=24, P2=96))
    cases["W_equal_maxD"] = (*planted_pair(32, 6, 32, 2), _p(32, 3))
    cases["W_below_maxD"] = (*planted_pair(20, 5, 32, 2), _p(32, 5))
    cases["H1"] = (*planted_pair(70, 1, 16, 5, seed=3), _p(16, 5, P1=100, P2=400))
    cases["H2_below_bs"] = (*planted_pair(70, 2, 16, 5, seed=4), _p(16, 7, P1=100, P2=400))
    cases["H_above_W1"] = (*planted_pair(39, 50, 32, 9, seed=5), _p(32, 3, P1=30, P2=120))     # 7 computed columns, 50 rows
    for D in (16, 32, 48, 64, 80, 128, 208, 256):               # every lane split of the path kernel, and D no power of two
        cases[f"D{D}_300x12"] = (*smooth_pair(300, 12, min(D - 3, 21), seed=D), _p(D, 5, P1=200, P2=800, uniquenessRatio=5))
    for bs in (1, 3, 11):
        cases[f"bs{bs}"] = (*smooth_pair(90, 21, 7, seed=bs), _p(32, bs, P1=8 * bs * bs, P2=32 * bs * bs))
    cases["P_defaults"] = (*smooth_pair(85, 17, 5, seed=7), _p(16, 3))
    for u in (0, 15):
        cases[f"uniq{u}"] = (*smooth_pair(85, 17, 9, seed=8), _p(32, 5, P1=200, P2=800, uniquenessRatio=u))
    for d12 in (0, 3):
        cases[f"disp12_{d12}"] = (*smooth_pair(85, 17, 9, seed=9), _p(32, 5, P1=50, P2=200, disp12MaxDiff=d12))
    for cap in (0, 63):
        cases[f"cap{cap}"] = (*smooth_pair(85, 17, 9, seed=10), _p(32, 5, P1=200, P2=800, preFilterCap=cap))
    cases["minD5"] = (*smooth_pair(85, 17, 11, seed=11), _p(16, 5, minDisparity=5, P1=200, P2=800))
    flat = np.full((14, 75), 77, np.uint8)
    cases["constant"] = (flat, flat.copy(), _p(32, 3, P1=10, P2=40))       # every cost ties: the lowest-d and the largest-x rules
    return cases
