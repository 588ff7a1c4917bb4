"""The AKAZE host plan (csrc/akaze_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small extern "C"
shim with the host compiler and compared with tests/akaze_ref.py - level counts and sizes at the octave cut, esigma / etime /
sigma_size / borders, plane offsets (which must not overlap), the FED tables and the taps bit for bit, the gauss25 table, the
float constants, the one-workgroup decision, the capacities and every refusal with its message."""
import ctypes
import math
import shutil
import subprocess

import numpy as np
import pytest

import akaze_ref as R
from conftest import PKG_NAME, ROOT
from orb_ref import ATAN_P, EPS32

SHIM = r"""
#include "akaze_plan.hpp"
#include <cstring>
using namespace sslam;
static AkzParams params(int noct, int nol, double thr, int maxp) { AkzParams p; p.noct = noct; p.nol = nol; p.threshold = thr; p.max_points = maxp; return p; }
// pi: w, h, nlev, noct, interior, max_tiles; ll: plane_floats, tmp_floats, then off per level;
// li per level: octave, sublevel, w, h, sigma_size, border, fed_n (filled by the FED shim), tx, ty, one_wg; ld: esigma, etime; lf: size, radius, ratio, half, norm, wnorm, quat
extern "C" void akz_plan_shim(int noct, int nol, int w, int h, int* pi, long long* ll, int* li, double* ld, float* lf) {
    const AkzPlan P = akz_plan(params(noct, nol, 0.001, -1), w, h);
    const int v[] = {P.w, P.h, P.nlev, P.noct, P.interior, P.max_tiles};
    for (int i = 0; i < 6; ++i) pi[i] = v[i];
    ll[0] = P.plane_floats; ll[1] = P.tmp_floats;
    for (int k = 0; k < P.nlev; ++k) {
        const AkzLevel& L = P.lv[k];
        ll[2 + k] = L.off;
        const int u[] = {L.octave, L.sublevel, L.w, L.h, L.sigma_size, L.border, 0, L.tx, L.ty, L.one_wg};
        for (int i = 0; i < 10; ++i) li[10 * k + i] = u[i];
        ld[2 * k] = L.esigma; ld[2 * k + 1] = L.etime;
        const float f[] = {L.size, L.radius, L.ratio, L.half, L.norm, L.wnorm, L.quat};
        for (int i = 0; i < 7; ++i) lf[7 * k + i] = f[i];
    }
}
extern "C" int akz_fed_shim(int noct, int nol, int* off, int* n, float* tau, int cap) {
    const AkzFed F = akz_fed(params(noct, nol, 0.001, -1));
    for (int i = 0; i < noct * nol; ++i) { off[i] = F.off[i]; n[i] = F.n[i]; }
    if (F.total > cap) return -1;
    for (int i = 0; i < F.total; ++i) tau[i] = F.tau[i];
    return F.total;
}
extern "C" int akz_fed_cycle_shim(double T, int ordered, float* tau, int cap) {
    const std::vector<float> t = akz_fed_steps(T, ordered != 0);
    if ((int)t.size() > cap) return -1;
    for (size_t i = 0; i < t.size(); ++i) tau[i] = t[i];
    return (int)t.size();
}
extern "C" int akz_taps_shim(double sigma, float* taps) { const std::vector<float> t = akz_gauss_taps(sigma); for (size_t i = 0; i < t.size(); ++i) taps[i] = t[i]; return (int)t.size(); }
extern "C" void akz_consts_shim(float* f, int* c, float* g) {
    const AkzConsts k = akz_consts();
    const float v[] = {k.atan.p1, k.atan.p3, k.atan.p5, k.atan.p7, k.atan.eps, k.atan.deg2rad, k.win_step, k.pi3, k.two_pi, k.five_pi3, k.img_div, k.kfallback, k.koctave};
    for (int i = 0; i < 13; ++i) f[i] = v[i];
    const int u[] = {AKZ_DESCRIPTOR_MLDB, AKZ_DIFF_PM_G2, AKZ_MAX_OCTAVES, AKZ_MAX_SUBLEVELS, AKZ_MAX_LEVELS, AKZ_MIN_OCTAVE_W, AKZ_MIN_OCTAVE_H, AKZ_DESC_BYTES,
                     AKZ_DESC_BITS, AKZ_NBINS, AKZ_WG_PIXELS, AKZ_WG_T, AKZ_WG_PER_THREAD, AKZ_FIXED_LOG2, AKZ_N_WINDOWS, AKZ_ORI_SAMPLES};
    for (int i = 0; i < 16; ++i) c[i] = u[i];
    std::memcpy(g, AKZ_GAUSS25, sizeof AKZ_GAUSS25);
}
extern "C" int akz_params_shim(int dt, int ds, int dc, double thr, int noct, int nol, int diff, int maxp, int max_w, int max_h, char* msg, int n) {
    AkzParams p; p.descriptor_type = dt; p.descriptor_size = ds; p.descriptor_channels = dc; p.threshold = thr; p.noct = noct; p.nol = nol;
    p.diffusivity = diff; p.max_points = maxp;
    return akz_check_params(p, max_w, max_h, msg, (size_t)n);
}
extern "C" int akz_image_shim(int w, int h, int c, int max_w, int max_h, char* msg, int n) { return feat_check_image(w, h, c, max_w, max_h, msg, (size_t)n); }
extern "C" long long akz_capacity_shim(int maxp, int max_w, int max_h, int co, int ko, int* cand, int* rows) {
    const AkzParams p = params(4, 4, 0.001, maxp);
    akz_capacities(p, max_w, max_h, co, ko, cand, rows);
    return akz_instance_bytes(p, max_w, max_h, *cand, *rows);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("akaze_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "akaze_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    i, dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    lib.akz_plan_shim.argtypes = [i, i, i, i, vp, vp, vp, vp, vp]
    lib.akz_plan_shim.restype = None
    lib.akz_fed_shim.argtypes = [i, i, vp, vp, vp, i]
    lib.akz_fed_cycle_shim.argtypes = [dbl, i, vp, i]
    lib.akz_taps_shim.argtypes = [dbl, vp]
    lib.akz_consts_shim.argtypes = [vp, vp, vp]
    lib.akz_consts_shim.restype = None
    lib.akz_params_shim.argtypes = [i, i, i, dbl, i, i, i, i, i, i, ctypes.c_char_p, i]
    lib.akz_image_shim.argtypes = [i] * 5 + [ctypes.c_char_p, i]
    lib.akz_capacity_shim.argtypes = [i] * 5 + [vp, vp]
    lib.akz_capacity_shim.restype = ctypes.c_longlong
    return lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def plan(lib, w, h, noct=4, nol=4):
    pi, ll, li = np.zeros(6, np.int32), np.zeros(2 + 64, np.int64), np.zeros((64, 10), np.int32)
    ld, lf = np.zeros((64, 2), np.float64), np.zeros((64, 7), np.float32)
    lib.akz_plan_shim(noct, nol, w, h, pi.ctypes.data, ll.ctypes.data, li.ctypes.data, ld.ctypes.data, lf.ctypes.data)
    P = dict(zip(("w", "h", "nlev", "noct", "interior", "max_tiles"), pi.tolist()))
    P["plane_floats"], P["tmp_floats"] = ll[:2].tolist()
    names = ("octave", "sublevel", "w", "h", "sigma_size", "border", "_", "tx", "ty", "one_wg")
    P["lv"] = [dict(zip(names, li[k].tolist()), off=int(ll[2 + k]), esigma=float(ld[k, 0]), etime=float(ld[k, 1]), f=lf[k].copy()) for k in range(P["nlev"])]
    return P


SIZES = [(1, 1), (97, 10), (10, 97), (11, 11), (97, 61), (163, 83), (159, 80), (160, 79), (160, 80), (323, 161), (643, 323), (1241, 376), (640, 480),
         (4096, 2160), (16384, 16384)]


def test_levels_offsets_and_the_one_workgroup_decision_equal_the_restatement(shim):
    for w, h in SIZES:
        for noct, nol in ((4, 4), (1, 4), (8, 1), (3, 5), (8, 8)):
            P = plan(shim, w, h, noct, nol)
            lv = R.levels(w, h, noct, nol)
            assert (P["w"], P["h"], P["nlev"], P["noct"], P["tmp_floats"]) == (w, h, len(lv), lv[-1]["octave"] + 1, w * h), (w, h)
            off = 0
            for k, (L, G) in enumerate(zip(lv, P["lv"])):
                assert [G[n] for n in ("octave", "sublevel", "w", "h", "sigma_size", "border")] == [L[n] for n in ("octave", "sublevel", "w", "h", "sigma_size", "border")]
                assert (G["esigma"], G["etime"], G["off"]) == (L["esigma"], L["etime"], off), (w, h, k)     # in order, no overlap
                off += L["w"] * L["h"]
                a, b = R.scharr_taps(L["sigma_size"])
                o = L["octave"]
                want = [L["size"], L["radius"], np.float32(1 << o), np.float32(0.5 * ((1 << o) - 1)), a, b, np.float32(L["sigma_size"] ** 4)]
                assert bits(G["f"]).tolist() == bits(want).tolist(), (w, h, k)
                interior = L["w"] > 2 * L["border"] and L["h"] > 2 * L["border"]
                assert (G["tx"], G["ty"]) == ((-(-L["w"] // 64), -(-L["h"] // 4)) if interior else (0, 0))
                assert G["one_wg"] == int(k > 0 and L["w"] * L["h"] <= R.WG_PIXELS)
            assert P["plane_floats"] == off
            assert P["interior"] == int(w > 2 * lv[0]["border"] and h > 2 * lv[0]["border"])
            assert P["max_tiles"] == max(G["tx"] * G["ty"] for G in P["lv"])


def test_the_octave_cut_and_the_documented_sizes(shim):
    assert [(plan(shim, w, h)["noct"]) for w, h in ((159, 80), (160, 79), (160, 80), (97, 61), (163, 83), (323, 161), (643, 323))] == [1, 1, 2, 1, 2, 3, 4]
    P = plan(shim, 1241, 376)
    assert [(L["w"], L["h"]) for L in P["lv"][::4]] == [(1241, 376), (620, 188), (310, 94), (155, 47)]
    assert [L["sigma_size"] for L in P["lv"]] == [2, 3, 3, 4] * 4
    assert [L["one_wg"] for L in P["lv"]] == [0] * 12 + [1] * 4              # 155 x 47 fits one workgroup's LDS, 310 x 94 does not
    assert [L["one_wg"] for L in plan(shim, 160, 80)["lv"]] == [0] + [1] * 7   # 160 x 80 = 12 800 pixels and 80 x 40


def test_the_fed_tables_equal_the_restatement_bit_for_bit(shim):
    for noct, nol in ((4, 4), (1, 1), (8, 1), (3, 5), (8, 8)):
        off, n, tau = np.zeros(64, np.int32), np.zeros(64, np.int32), np.zeros(1 << 16, np.float32)
        total = shim.akz_fed_shim(noct, nol, off.ctypes.data, n.ctypes.data, tau.ctypes.data, len(tau))
        lv = R.levels(16384, 16384, noct, nol)
        assert len(lv) == noct * nol and total >= 0
        at = 0
        for k in range(1, len(lv)):
            want = R.fed_steps(lv[k]["etime"] - lv[k - 1]["etime"])
            assert (off[k], n[k]) == (at, len(want))
            assert bits(tau[at:at + len(want)]).tolist() == bits(want).tolist(), (noct, nol, k)
            at += len(want)
        assert total == at and n[0] == 0
        if (noct, nol) == (4, 4):
            assert n[:16].tolist() == [0, 3, 3, 4, 4, 5, 6, 7, 8, 10, 12, 14, 17, 20, 24, 29] and total == 166
    buf = np.zeros(4096, np.float32)
    for T in (0.7, 3.3, 100.0, 15728.64):
        k = shim.akz_fed_cycle_shim(T, 0, buf.ctypes.data, len(buf))
        assert bits(buf[:k]).tolist() == bits(R.fed_unordered(T)).tolist()


def test_taps_constants_and_the_gauss25_table(shim):
    buf = np.zeros(16, np.float32)
    for sigma, n in ((1.6, 9), (1.0, 5)):
        assert shim.akz_taps_shim(sigma, buf.ctypes.data) == n == len(R.gauss_taps(sigma))
        assert bits(buf[:n]).tolist() == bits(R.gauss_taps(sigma)).tolist()
    f, c, g = np.zeros(13, np.float32), np.zeros(16, np.int32), np.zeros((7, 7), np.float32)
    shim.akz_consts_shim(f.ctypes.data, c.ctypes.data, g.ctypes.data)
    want = [*ATAN_P, EPS32, R.DEG2RAD, np.float32(0.15), R.PI3, R.TWO_PI, R.FIVE_PI3, np.float32(255), np.float32(0.03), np.float32(0.75)]
    assert bits(f).tolist() == bits(want).tolist()
    assert c.tolist() == [R.DESCRIPTOR_MLDB, R.DIFF_PM_G2, R.MAX_OCTAVES, R.MAX_SUBLEVELS, 64, R.MIN_OCTAVE_W, R.MIN_OCTAVE_H, R.DESC_BYTES, R.DESC_BITS,
                          R.KCONTRAST_NBINS, R.WG_PIXELS, 1024, 20, R.FIXED_LOG2, R.N_WINDOWS, 109]
    assert c[11] * c[12] >= c[10] and 8 * c[10] <= 160 * 1024
    assert bits(g).tolist() == bits(R.GAUSS25).tolist()
    assert abs(float(g[0, 0]) - 1 / (2 * math.pi * 6.25)) < 1e-6               # a Gaussian of sigma 2.5
    i, j = np.mgrid[-6:7, -6:7]
    assert int((i * i + j * j < 36).sum()) == 109


def test_capacities(shim):
    def cap(maxp, w, h, co=0, ko=0):
        c, r = ctypes.c_int(0), ctypes.c_int(0)
        b = shim.akz_capacity_shim(maxp, w, h, co, ko, ctypes.byref(c), ctypes.byref(r))
        return c.value, r.value, b
    assert cap(-1, 1241, 376)[:2] == (1241 * 376 // 8, 1241 * 376 // 16)
    assert cap(-1, 40, 40)[:2] == (1024, 1024)
    assert cap(500, 4096, 2160)[:2] == (4096 * 2160 // 8, 16384)
    assert cap(100000, 1241, 376)[1] == 1241 * 376 // 16
    assert cap(-1, 1241, 376, 77, 55)[:2] == (77, 55)
    c, r, b = cap(-1, 1241, 376)
    planes = sum(L["w"] * L["h"] for L in R.levels(1241, 376))
    assert b == 4 * (5 * planes + 5 * 1241 * 376) + 20 * c + 141 * r and b < 0.07e9
    assert cap(-1, 4096, 2160)[2] < 1.4e9


REFUSALS = [
    (dict(dt=3), "descriptor_type 3 is not supported (only DESCRIPTOR_MLDB = 5)"),
    (dict(dt=4), "descriptor_type 4 is not supported (only DESCRIPTOR_MLDB = 5)"),
    (dict(ds=64), "descriptor_size 64 is not supported (only 0: the full 486 bits)"),
    (dict(dc=1), "descriptor_channels 1 is not supported (only 3)"),
    (dict(thr=0.0), "threshold 0 is not positive and finite"),
    (dict(thr=float("inf")), "threshold inf is not positive and finite"),
    (dict(thr=float("nan")), "threshold nan is not positive and finite"),
    (dict(noct=0), "nOctaves 0 outside 1..8"),
    (dict(noct=9), "nOctaves 9 outside 1..8"),
    (dict(nol=0), "nOctaveLayers 0 outside 1..8"),
    (dict(nol=9), "nOctaveLayers 9 outside 1..8"),
    (dict(diff=2), "diffusivity 2 is not supported (only DIFF_PM_G2 = 1)"),
    (dict(maxp=0), "max_points 0 is neither -1 nor in 1..1048576"),
    (dict(maxp=-2), "max_points -2 is neither -1 nor in 1..1048576"),
    (dict(max_w=0), "frame size 0x100 outside 1..16384"),
    (dict(max_h=16385), "frame size 100x16385 outside 1..16384"),
]


def test_every_refusal_with_its_message(shim):
    base = dict(dt=5, ds=0, dc=3, thr=0.001, noct=4, nol=4, diff=1, maxp=-1, max_w=100, max_h=100)
    msg = ctypes.create_string_buffer(200)

    def check(**kw):
        a = dict(base, **kw)
        msg.value = b""
        rc = shim.akz_params_shim(a["dt"], a["ds"], a["dc"], a["thr"], a["noct"], a["nol"], a["diff"], a["maxp"], a["max_w"], a["max_h"], msg, 200)
        return rc, msg.value.decode()
    assert check() == (0, "")
    assert check(maxp=1)[0] == 0 and check(noct=8, nol=8)[0] == 0 and check(noct=1, nol=1)[0] == 0
    codes = set()
    for kw, text in REFUSALS:
        rc, got = check(**kw)
        assert rc != 0 and got == text, (kw, got)
        assert R.check_params(**{{"dt": "descriptor_type", "ds": "descriptor_size", "dc": "descriptor_channels", "thr": "threshold", "noct": "nOctaves",
                                  "nol": "nOctaveLayers", "diff": "diffusivity", "maxp": "max_points"}[k]: v for k, v in kw.items()
                                 if k not in ("max_w", "max_h")}) is not None or "max_" in next(iter(kw))
        codes.add(rc)
    assert len(codes) == 9
    for (w, h, c), text in (((10, 10, 2), "2 channels (want 1, 3 or 4)"), ((0, 10, 1), "frame size 0x10"),
                            ((101, 100, 1), "frame 101x100 is larger than the instance's 100x100"), ((100, 101, 3), "frame 100x101 is larger than the instance's 100x100")):
        msg.value = b""
        assert shim.akz_image_shim(w, h, c, 100, 100, msg, 200) != 0 and msg.value.decode() == text
    assert shim.akz_image_shim(100, 100, 4, 100, 100, msg, 200) == 0
