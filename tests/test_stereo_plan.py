"""The stereo host plan (csrc/stereo_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small extern "C"
shim with the host compiler and compared with tests/stereo_ref.py - the normalised parameters, the largest costs, the workspace
extents, the lane split of the path kernel, the paths of every direction and every refusal with its message."""
import ctypes
import itertools
import shutil
import subprocess

import numpy as np
import pytest

import stereo_ref as R
from conftest import PKG_NAME, ROOT

SHIM = r"""
#include "stereo_plan.hpp"
using namespace sslam;
// out: minD D bs P1 P2 d12 uniq ftzero maxD invalid max_pixel_cost max_block_cost
extern "C" void sg_norm_shim(int minD, int D, int bs, int P1, int P2, int d12, int cap, int uniq, int* out) {
    const SgbmParams p = sgbm_normalise(minD, D, bs, P1, P2, d12, cap, uniq);
    const int v[] = {p.minD, p.D, p.bs, p.P1, p.P2, p.d12, p.uniq, p.ftzero, p.maxD, p.invalid, sgbm_max_pixel_cost(p), sgbm_max_block_cost(p)};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
}
// out: px cols vol bytes
extern "C" void sg_extents_shim(int w, int h, int maxD, int D, unsigned long long* out) {
    const SgbmExtents e = sgbm_extents(w, h, maxD, D);
    out[0] = e.px; out[1] = e.cols; out[2] = e.vol; out[3] = e.bytes;
}
extern "C" void sg_split_shim(int D, int* out) { out[0] = sgbm_group_lanes(D); out[1] = sgbm_d_per_lane(D); out[2] = sgbm_paths_per_block(D); }
extern "C" int sg_path_count_shim(int dir, int H, int W1) { return sgbm_path_count(dir, H, W1); }
extern "C" int sg_path_blocks_shim(int dir, int H, int W1, int D) { return sgbm_path_blocks(dir, H, W1, D); }
extern "C" void sg_path_shim(int dir, int p, int H, int W1, int* out) {
    const SgbmPath q = sgbm_path(dir, p, H, W1);
    out[0] = q.y0; out[1] = q.x0; out[2] = q.dy; out[3] = q.dx; out[4] = q.len;
}
extern "C" void sg_consts_shim(long long* c) {
    const long long v[] = {SGBM_MODE_SGBM, SGBM_MAX_SIDE, SGBM_MAX_COST, (long long)SGBM_MAX_WORKSPACE, SGBM_DIRECTIONS, SGBM_PATH_T, SGBM_STAGE_PF_LEFT,
                           SGBM_STAGE_PF_RIGHT, SGBM_STAGE_C, SGBM_STAGE_S, SGBM_STAGE_RAW, SGBM_STAGE_RIGHT, SGBM_STAGE_CHECKED};
    for (int i = 0; i < 13; ++i) c[i] = v[i];
}
extern "C" int sg_create_shim(int w, int h, int minD, int D, int bs, int P1, int P2, int d12, int cap, int uniq, int spw, int spr, int mode, char* msg,
                              int n) {
    return sgbm_check_create(w, h, minD, D, bs, P1, P2, d12, cap, uniq, spw, spr, mode, msg, (size_t)n);
}
extern "C" int sg_image_shim(int w, int h, int c, int mw, int mh, char* msg, int n) { return sgbm_check_image(w, h, c, mw, mh, msg, (size_t)n); }
"""

KEYS = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio", "speckleWindowSize",
        "speckleRange", "mode")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ found: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("stereo_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "stereo_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    i, vp = ctypes.c_int, ctypes.c_void_p
    lib.sg_norm_shim.argtypes = [i] * 8 + [vp]
    lib.sg_extents_shim.argtypes = [i] * 4 + [vp]
    lib.sg_split_shim.argtypes = [i, vp]
    lib.sg_path_count_shim.argtypes = [i] * 3
    lib.sg_path_blocks_shim.argtypes = [i] * 4
    lib.sg_path_shim.argtypes = [i] * 4 + [vp]
    lib.sg_consts_shim.argtypes = [vp]
    lib.sg_create_shim.argtypes = [i] * 13 + [ctypes.c_char_p, i]
    lib.sg_image_shim.argtypes = [i] * 5 + [ctypes.c_char_p, i]
    return lib


def test_normalisation_equals_the_restatement(shim):
    out = np.zeros(12, np.int32)
    for minD, D, bs, P1, P2, d12, cap, uniq in itertools.product((0, 5), (16, 256), (1, 11), (-1, 0, 7, 968), (-2, 0, 3, 8, 3872), (-1, 0, 3), (0, 15, 16, 31, 63),
                                                                 (-1, 0, 15, 100)):
        shim.sg_norm_shim(minD, D, bs, P1, P2, d12, cap, uniq, out.ctypes.data)
        p = R.Params(minD, D, bs, P1, P2, d12, cap, uniq)
        assert out.tolist() == [p.minD, p.D, p.bs, p.P1, p.P2, p.d12, p.uniq, p.ftzero, p.maxD, p.invalid, p.max_pixel_cost(), p.max_block_cost()]
        assert p.P2 > p.P1 >= 1 and p.d12 >= 1 and p.ftzero % 2 == 1 and 15 <= p.ftzero <= 63
    shim.sg_norm_shim(0, 32, 11, 968, 3872, 0, 0, 0, out.ctypes.data)           # the prototype's configuration
    assert out.tolist() == [0, 32, 11, 968, 3872, 1, 0, 15, 32, -16, 70, 8470]


def test_constants_and_lane_split(shim):
    c = np.zeros(13, np.int64)
    shim.sg_consts_shim(c.ctypes.data)
    assert c.tolist() == [R.MODE_SGBM, R.MAX_SIDE, R.MAX_COST, R.MAX_WORKSPACE, len(R.DIRECTIONS), 256] + [R.STAGES[k] for k in
                                                                                                       ("pf_left", "pf_right", "C", "S", "raw", "right", "checked")]
    s = np.zeros(3, np.int32)
    for D in range(16, 257, 16):
        shim.sg_split_shim(D, s.ctypes.data)
        lanes, per, paths = s.tolist()
        if D in (16, 32, 64, 128, 256):
            assert (lanes, per) == {16: (16, 1), 32: (32, 1), 64: (64, 1), 128: (64, 2), 256: (64, 4)}[D]
            assert lanes & (lanes - 1) == 0                                   # the shuffles' width
        assert D <= lanes * per < 2 * D and lanes * paths == 256 and lanes in (16, 32, 64) and per in (1, 2, 4)


def test_extents_equal_the_restatement(shim):
    e = np.zeros(4, np.uint64)
    for w, h, maxD, D in ((1, 1, 16, 16), (16, 9, 16, 16), (17, 9, 16, 16), (96, 32, 16, 16), (300, 12, 256, 256), (1241, 376, 32, 32), (1241, 376, 128, 128),
                          (1241, 376, 256, 256), (1241, 376, 261, 256), (16384, 16384, 16, 16), (4096, 2048, 300, 256)):
        shim.sg_extents_shim(w, h, maxD, D, e.ctypes.data)
        cols = max(w - maxD, 0)
        assert e.tolist() == [w * h, cols, h * cols * D, R.workspace_bytes(w, h, maxD, D)], (w, h, maxD, D)
    shim.sg_extents_shim(1241, 376, 32, 32, e.ctypes.data)
    assert int(e[2]) * 2 == 376 * 1209 * 32 * 2 and 29e6 < int(e[2]) * 2 < 30e6   # the prototype's cost volume: 29 MB
    assert 95e6 < int(e[3]) < 100e6                                             # an instance of it: 98.4 MB


def test_paths_cover_every_pixel_once_and_equal_the_restatement(shim):
    q = np.zeros(5, np.int32)
    for H, W1 in ((1, 1), (1, 9), (9, 1), (2, 54), (5, 8), (8, 5), (7, 7), (50, 7), (12, 63), (12, 65)):
        for k, (dy, dx) in enumerate(R.DIRECTIONS):
            n = shim.sg_path_count_shim(k, H, W1)
            assert n == R.path_count(k, H, W1)
            seen = np.zeros((H, W1), np.int32)
            for p in range(n):
                shim.sg_path_shim(k, p, H, W1, q.ctypes.data)
                y0, x0, gy, gx, ln = q.tolist()
                assert (y0, x0, ln) == R.path_start(k, p, H, W1) and (gy, gx) == (dy, dx) and ln >= 1
                ys, xs = y0 + gy * np.arange(ln), x0 + gx * np.arange(ln)
                assert ys.min() >= 0 and ys.max() < H and xs.min() >= 0 and xs.max() < W1       # every step inside the region
                seen[ys, xs] += 1
            assert (seen == 1).all(), (H, W1, k)
            for D in (16, 32, 48, 64, 80, 128, 208, 256):
                per_block = 256 // min(1 << (D - 1).bit_length(), 64)
                assert shim.sg_path_blocks_shim(k, H, W1, D) == -(-n // per_block)


REFUSALS = [
    (dict(mode=1), "mode 1 is not built (only MODE_SGBM = 0)"),
    (dict(mode=2), "mode 2 is not built (only MODE_SGBM = 0)"),
    (dict(mode=3), "mode 3 is not built (only MODE_SGBM = 0)"),
    (dict(speckleWindowSize=100), "speckleWindowSize 100: the speckle filter is not built (want 0)"),
    (dict(minDisparity=-1), "minDisparity -1 < 0"),
    (dict(numDisparities=0), "numDisparities 0 is not a multiple of 16 in 16..256"),
    (dict(numDisparities=24), "numDisparities 24 is not a multiple of 16 in 16..256"),
    (dict(numDisparities=272), "numDisparities 272 is not a multiple of 16 in 16..256"),
    (dict(blockSize=0), "blockSize 0 is not odd in 1..11"),
    (dict(blockSize=4), "blockSize 4 is not odd in 1..11"),
    (dict(blockSize=13), "blockSize 13 is not odd in 1..11"),
    (dict(preFilterCap=-1), "preFilterCap -1 outside 0..63"),
    (dict(preFilterCap=64), "preFilterCap 64 outside 0..63"),
    (dict(uniquenessRatio=101), "uniquenessRatio 101 > 100"),
    (dict(w=0), "image size 0x60 outside 1..16384"),
    (dict(w=16385), "image size 16385x60 outside 1..16384"),
    (dict(h=0), "image size 100x0 outside 1..16384"),
    (dict(h=16385), "image size 100x16385 outside 1..16384"),
    (dict(blockSize=11, P2=32767 - 8470 + 1), "P2 24298 with blockSize 11: the largest block cost 8470 (= 11^2 x 70 per pixel) + P2 exceeds 32767"),
    (dict(blockSize=11, preFilterCap=63, P2=30000), "P2 30000 with blockSize 11: the largest block cost 11374 (= 11^2 x 94 per pixel) + P2 exceeds 32767"),
    (dict(blockSize=1, P1=40000), "P2 40001 with blockSize 1: the largest block cost 70 (= 1^2 x 70 per pixel) + P2 exceeds 32767"),
    (dict(w=16384, h=16384), f"workspace of {R.workspace_bytes(16384, 16384, 32, 32)} bytes exceeds 4294967296"),
    (dict(w=4096, h=2048, numDisparities=256), f"workspace of {R.workspace_bytes(4096, 2048, 256, 256)} bytes exceeds 4294967296"),
]


def test_every_refusal_with_its_message(shim):
    base = dict(w=100, h=60, minDisparity=0, numDisparities=32, blockSize=5, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                speckleWindowSize=0, speckleRange=0, mode=0)
    msg = ctypes.create_string_buffer(240)

    def create(**kw):
        a = dict(base, **kw)
        msg.value = b""
        rc = shim.sg_create_shim(a["w"], a["h"], *[a[k] for k in KEYS], msg, 240)
        return rc, msg.value.decode(), R.check_create(a["w"], a["h"], *[a[k] for k in KEYS])
    assert create() == (0, "", None)
    for kw in (dict(numDisparities=16), dict(numDisparities=256), dict(blockSize=1), dict(blockSize=11, P1=968, P2=3872), dict(preFilterCap=63),
               dict(uniquenessRatio=100), dict(uniquenessRatio=-1), dict(w=1, h=1), dict(w=16, h=3), dict(speckleRange=7), dict(disp12MaxDiff=-1),
               dict(blockSize=11, P2=32767 - 8470), dict(w=1241, h=376, numDisparities=256), dict(minDisparity=40)):
        assert create(**kw) == (0, "", None), kw
    for kw, text in REFUSALS:
        rc, got, ref = create(**kw)
        assert rc != 0 and got == text == ref, (kw, got, ref)
    for (w, h, c), text in (((10, 10, 2), "2 channels (want 1, 3 or 4)"), ((0, 10, 1), "image size 0x10 outside 1..16384"),
                            ((101, 60, 1), "image 101x60 is larger than the instance's 100x60"), ((100, 61, 3), "image 100x61 is larger than the instance's 100x60")):
        msg.value = b""
        assert shim.sg_image_shim(w, h, c, 100, 60, msg, 240) != 0 and msg.value.decode() == text == R.check_image(w, h, c, 100, 60)
    for c in (1, 3, 4):
        assert shim.sg_image_shim(100, 60, c, 100, 60, msg, 240) == 0 and R.check_image(100, 60, c, 100, 60) is None
