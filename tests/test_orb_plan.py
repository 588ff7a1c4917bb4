"""The ORB host plan (csrc/orb_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small extern "C"
shim with the host compiler and compared with tests/orb_ref.py - level sizes and scales, quotas, `umax`, the blur taps, the
float constants, the border, the slab and candidate extents (which must not overlap), the capacities (at least the NMS
bound), the tile tables, the default pattern and every refusal - over sizes from 7 x 7 to 2048 x 2048, scale factors 1.05 /
1.2 / 2.0 and 1..16 levels."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import orb_ref as R
from conftest import PKG_NAME, ROOT

LEVEL_INTS = ("w", "h", "stride", "rows", "active", "quota", "cut1_n", "fast_tx", "fast_ty", "fast_base", "pad_tx", "pad_ty", "pad_base",
              "cand_cap")
PLAN_INTS = ("w", "h", "nlevels", "border", "nactive", "fast_tiles", "blur_tiles")
PLAN_FLOATS = ("harris_k", "harris_scale4", "atan_p1", "atan_p3", "atan_p5", "atan_p7", "atan_eps", "deg2rad", "patch_size")
PLAN_FLOAT_FIELDS = ("harris_k", "harris_scale4", "atan.p1", "atan.p3", "atan.p5", "atan.p7", "atan.eps", "atan.deg2rad", "patch_size")   # in OrbPlan
NL, NP, NF = len(LEVEL_INTS), len(PLAN_INTS), len(PLAN_FLOATS)

SHIM = r"""
#include "orb_plan.hpp"
using namespace sslam;
static OrbParams params(int nfeatures, double sf, int nlevels, int edge, int score, int fast) {
    OrbParams p; p.nfeatures = nfeatures; p.scale_factor = sf; p.nlevels = nlevels; p.edge_threshold = edge; p.score_type = score;
    p.fast_threshold = fast; return p;
}
extern "C" void orb_plan_shim(int nfeatures, double sf, int nlevels, int edge, int score, int fast, int w, int h, int* pi, float* pf,
                              int* li, long long* ll, float* lf, int* tables) {
    const OrbPlan P = orb_plan(params(nfeatures, sf, nlevels, edge, score, fast), w, h);
    const int v[] = {%s};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) pi[i] = v[i];
    const float f[] = {%s};
    for (size_t i = 0; i < sizeof(f) / sizeof(f[0]); ++i) pf[i] = f[i];
    ll[0] = P.slab_bytes; ll[1] = P.cand_total;
    for (int l = 0; l < ORB_MAX_LEVELS; ++l) {
        const OrbLevel& L = P.lv[l];
        const int u[] = {%s};
        for (size_t i = 0; i < sizeof(u) / sizeof(u[0]); ++i) li[l * %d + i] = u[i];
        ll[2 + 2 * l] = L.off; ll[3 + 2 * l] = L.cand_off;
        lf[l] = L.scale;
    }
    for (int i = 0; i < 16; ++i) tables[i] = P.umax[i];
    for (int i = 0; i < 7; ++i) tables[16 + i] = P.gauss[i];
}
extern "C" int orb_params_shim(int nfeatures, double sf, int nlevels, int edge, int score, int fast, int max_w, int max_h, char* msg, int n) {
    return orb_check_params(params(nfeatures, sf, nlevels, edge, score, fast), max_w, max_h, msg, (size_t)n);
}
extern "C" int orb_image_shim(int w, int h, int c, int max_w, int max_h, char* msg, int n) { return feat_check_image(w, h, c, max_w, max_h, msg, (size_t)n); }
extern "C" int orb_pattern_check_shim(const signed char* p, char* msg, int n) { return orb_check_pattern((const int8_t*)p, msg, (size_t)n); }
extern "C" void orb_pattern_shim(signed char* out) { orb_default_pattern((int8_t*)out); }
extern "C" long long orb_capacity_shim(int nfeatures, double sf, int nlevels, int edge, int max_w, int max_h) {
    return orb_capacity(params(nfeatures, sf, nlevels, edge, 0, 20), max_w, max_h);
}
extern "C" void orb_constants_shim(int* o) {
    const int v[] = {ORB_MAX_LEVELS, ORB_MAX_SIDE, ORB_MAX_FEATURES, ORB_PATCH, ORB_HALF, ORB_REACH, ORB_PATTERN_POINTS, ORB_TILE_W, ORB_TILE_H, ORB_FAST_W, ORB_FAST_H};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}
""" % (", ".join("P." + n for n in PLAN_INTS), ", ".join("P." + n for n in PLAN_FLOAT_FIELDS), ", ".join("L." + n for n in LEVEL_INTS), NL)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("orb_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "orb_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    lib.orb_plan_shim.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 6
    lib.orb_plan_shim.restype = None
    lib.orb_params_shim.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int]
    lib.orb_image_shim.argtypes = [ctypes.c_int] * 5 + [ctypes.c_char_p, ctypes.c_int]
    lib.orb_pattern_check_shim.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    lib.orb_pattern_shim.argtypes = [ctypes.c_void_p]
    lib.orb_capacity_shim.argtypes = [ctypes.c_int, ctypes.c_double] + [ctypes.c_int] * 4
    lib.orb_capacity_shim.restype = ctypes.c_longlong
    lib.orb_constants_shim.argtypes = [ctypes.c_void_p]
    return lib


def plan(lib, w, h, nfeatures=500, sf=1.2, nlevels=8, edge=31, score=0, fast=20):
    pi, pf = np.zeros(NP, np.int32), np.zeros(NF, np.float32)
    li, ll, lf, tb = np.zeros((16, NL), np.int32), np.zeros(2 + 32, np.int64), np.zeros(16, np.float32), np.zeros(23, np.int32)
    lib.orb_plan_shim(nfeatures, float(np.float32(sf)), nlevels, edge, score, fast, w, h, *(a.ctypes.data for a in (pi, pf, li, ll, lf, tb)))
    P = dict(zip(PLAN_INTS, pi.tolist()))
    P.update(zip(PLAN_FLOATS, pf))
    P["slab_bytes"], P["cand_total"] = int(ll[0]), int(ll[1])
    P["lv"] = [dict(zip(LEVEL_INTS, li[lv].tolist()), off=int(ll[2 + 2 * lv]), cand_off=int(ll[3 + 2 * lv]), scale=lf[lv]) for lv in range(nlevels)]
    P["umax"], P["gauss"] = tb[:16].tolist(), tb[16:].tolist()
    return P


SIZES = [(7, 7), (7, 2048), (2048, 7), (8, 9), (31, 33), (63, 63), (62, 200), (64, 400), (400, 64), (97, 131), (100, 80), (640, 480),
         (1241, 376), (1000, 1001), (1919, 1081), (2048, 2048), (2047, 13)]


def check(P, w, h, nfeatures, sf, nlevels, edge, score):
    b = R.border(edge)
    assert (P["w"], P["h"], P["nlevels"], P["border"]) == (w, h, nlevels, b)
    sizes, scales, quota = R.level_sizes(w, h, sf, nlevels), R.level_scales(sf, nlevels), R.quotas(nfeatures, sf, nlevels)
    alive, spans, cspans, ft, bt = True, [], [], 0, 0
    for lv in range(nlevels):
        L = P["lv"][lv]
        assert (L["w"], L["h"]) == sizes[lv], (w, h, sf, lv)
        assert L["scale"].tobytes() == scales[lv].tobytes()
        assert L["quota"] == quota[lv] and L["cut1_n"] == (2 * quota[lv] if score == 0 else quota[lv])
        alive = alive and min(sizes[lv]) >= 2 * edge + 1
        assert L["active"] == alive
        if not alive:
            continue
        assert (L["stride"], L["rows"]) == (L["w"] + 2 * b, L["h"] + 2 * b)
        spans.append((L["off"], L["off"] + L["stride"] * L["rows"]))
        assert L["cand_cap"] >= -(-L["w"] // 2) * -(-L["h"] // 2)                   # the NMS bound
        cspans.append((L["cand_off"], L["cand_off"] + L["cand_cap"]))
        assert L["fast_tx"] * 32 >= L["w"] > (L["fast_tx"] - 1) * 32 and L["fast_ty"] * 32 >= L["h"] > (L["fast_ty"] - 1) * 32
        assert L["pad_tx"] * 32 >= L["stride"] > (L["pad_tx"] - 1) * 32 and L["pad_ty"] * 8 >= L["rows"] > (L["pad_ty"] - 1) * 8
        assert (L["fast_base"], L["pad_base"]) == (ft, bt)
        ft += L["fast_tx"] * L["fast_ty"]
        bt += L["pad_tx"] * L["pad_ty"]
    assert P["nactive"] == len(spans) and (P["fast_tiles"], P["blur_tiles"]) == (ft, bt)
    for s, total in ((spans, P["slab_bytes"]), (cspans, P["cand_total"])):
        for (a0, a1), (b0, b1) in zip(s, s[1:]):
            assert a0 < a1 <= b0                                                      # in order, no overlap
        assert not s or (s[0][0] == 0 and s[-1][1] <= total)
    assert all(o % 256 == 0 for o, _ in spans)


def test_the_plan_equals_the_restatement_over_the_sweep(shim):
    n = 0
    for w, h in SIZES:
        for sf in (1.05, 1.2, 2.0):
            for nlevels in range(1, 17):
                for edge, score, nfeatures in ((31, 0, 500), (3, 1, 6000), (8, 0, 37)):
                    check(plan(shim, w, h, nfeatures, sf, nlevels, edge, score), w, h, nfeatures, sf, nlevels, edge, score)
                    n += 1
    assert n == len(SIZES) * 3 * 16 * 3


def test_tables_constants_and_the_default_pattern(shim):
    P = plan(shim, 640, 480)
    assert P["umax"] == R.umax_table()
    assert P["gauss"] == R.gauss_taps().tolist()
    p1, p3, p5, p7 = R.ATAN_P
    for name, want in (("harris_k", R.F32(0.04)), ("harris_scale4", R.harris_scale4()), ("atan_p1", p1), ("atan_p3", p3), ("atan_p5", p5),
                       ("atan_p7", p7), ("atan_eps", R.EPS32), ("deg2rad", R.F32(np.pi / 180.0)), ("patch_size", R.F32(31))):
        assert P[name].tobytes() == np.float32(want).tobytes(), name
    pat = np.zeros((512, 2), np.int8)
    shim.orb_pattern_shim(pat.ctypes.data)
    np.testing.assert_array_equal(pat, R.default_pattern())
    c = np.zeros(11, np.int32)
    shim.orb_constants_shim(c.ctypes.data)
    assert c.tolist() == [R.MAX_LEVELS, 16384, 1 << 20, R.PATCH, R.HALF, R.REACH, 512, 32, 8, 32, 32]


def test_the_capacity_bounds_every_smaller_frame(shim):
    for sf, nlevels, edge in ((1.2, 8, 31), (2.0, 16, 3), (1.05, 16, 8)):
        cap = shim.orb_capacity_shim(500, float(np.float32(sf)), nlevels, edge, 640, 480)
        big = plan(shim, 640, 480, 500, sf, nlevels, edge)
        assert cap == max(big["cand_total"], 1)
        for w, h in ((640, 480), (639, 480), (640, 1), (17, 480), (320, 240), (1, 1)):
            P = plan(shim, w, h, 500, sf, nlevels, edge)
            assert P["cand_total"] <= cap and P["slab_bytes"] <= big["slab_bytes"]


def test_every_refusal(shim):
    msg = ctypes.create_string_buffer(200)

    def params(nfeatures=500, sf=1.2, nlevels=8, edge=31, score=0, fast=20, max_w=640, max_h=480):
        msg.value = b""
        return shim.orb_params_shim(nfeatures, sf, nlevels, edge, score, fast, max_w, max_h, msg, 200), msg.value.decode()
    assert params() == (0, "")
    for kw, word in ((dict(nfeatures=0), "nfeatures 0"), (dict(nfeatures=(1 << 20) + 1), "nfeatures"), (dict(sf=1.0), "scaleFactor"),
                     (dict(sf=2.0000005), "scaleFactor"), (dict(sf=float("nan")), "scaleFactor"), (dict(nlevels=0), "nlevels 0"),
                     (dict(nlevels=17), "nlevels 17"), (dict(edge=2), "edgeThreshold 2"), (dict(score=2), "scoreType 2"),
                     (dict(score=-1), "scoreType"), (dict(fast=0), "fastThreshold 0"), (dict(fast=255), "fastThreshold 255"),
                     (dict(max_w=0), "frame size"), (dict(max_h=16385), "frame size")):
        rc, text = params(**kw)
        assert rc != 0 and word in text, (kw, text)
    assert params(sf=2.0)[0] == 0 and params(sf=1.0000001)[0] == 0 and params(edge=3, fast=1)[0] == 0 and params(fast=254, score=1)[0] == 0

    def image(w, h, c, max_w=640, max_h=480):
        msg.value = b""
        return shim.orb_image_shim(w, h, c, max_w, max_h, msg, 200), msg.value.decode()
    assert image(640, 480, 1) == (0, "") and image(1, 1, 3)[0] == 0 and image(5, 5, 4)[0] == 0
    for a, word in (((641, 480, 1), "larger than the instance's 640x480"), ((640, 481, 3), "larger"), ((640, 480, 2), "2 channels"),
                    ((0, 480, 1), "frame size"), ((640, 0, 1), "frame size")):
        rc, text = image(*a)
        assert rc != 0 and word in text, (a, text)
    pat = R.default_pattern().copy()
    assert shim.orb_pattern_check_shim(pat.ctypes.data, msg, 200) == 0
    for v in (16, -16, 127, -128):
        bad = pat.copy(); bad[300, 1] = v
        assert shim.orb_pattern_check_shim(bad.ctypes.data, msg, 200) != 0 and b"pattern point 300" in msg.value
