"""The SIFT host plan (csrc/sift_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small extern "C"
shim with the host compiler and compared with tests/sift_ref.py - octave counts and sizes for odd and thin frames, the slab
extents (which must not overlap), the extrema tile table, the sigmas, the taps bit for bit, the integer threshold, the float
constants, the capacities and every refusal with its message."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import sift_ref as R
from conftest import PKG_NAME, ROOT

SHIM = r"""
#include "sift_plan.hpp"
using namespace sslam;
static SiftParams params(int nfeatures, int nol, double contrast, double edge, double sigma) {
    SiftParams p; p.nfeatures = nfeatures; p.nol = nol; p.contrast = contrast; p.edge = edge; p.sigma = sigma; return p;
}
// pi: w, h, nol, noct, ext_tiles, threshold, tail_first; ll: gauss_floats, dog_floats, tmp_floats, then goff, doff per octave; oi: w, h, tx, ty, tile_base per octave
extern "C" void sift_plan_shim(int nol, double contrast, int w, int h, int* pi, long long* ll, int* oi) {
    const SiftPlan P = sift_plan(params(0, nol, contrast, 10, 1.6), w, h);
    const int v[] = {P.w, P.h, P.nol, P.noct, P.ext_tiles, P.threshold, P.tail_first};
    for (int i = 0; i < 7; ++i) pi[i] = v[i];
    ll[0] = P.gauss_floats; ll[1] = P.dog_floats; ll[2] = P.tmp_floats;
    for (int o = 0; o < SIFT_MAX_OCTAVES; ++o) {
        const SiftOctave& O = P.oc[o];
        ll[3 + 2 * o] = O.goff; ll[4 + 2 * o] = O.doff;
        const int u[] = {O.w, O.h, O.tx, O.ty, O.tile_base};
        for (int i = 0; i < 5; ++i) oi[5 * o + i] = u[i];
    }
}
extern "C" int sift_taps_shim(int nol, double sigma, int* n, int* off, double* sig, float* taps, int cap) {
    const SiftTaps T = sift_taps(params(0, nol, 0.04, 10, sigma));
    for (int i = 0; i < nol + 3; ++i) { n[i] = T.n[i]; off[i] = T.off[i]; sig[i] = T.sigma[i]; }
    if ((int)T.taps.size() > cap) return -1;
    for (size_t i = 0; i < T.taps.size(); ++i) taps[i] = T.taps[i];
    return (int)T.taps.size();
}
extern "C" void sift_consts_shim(float* f, int* c) {
    const SiftConsts k = sift_consts();
    const float v[] = {k.atan.p1, k.atan.p3, k.atan.p5, k.atan.p7, k.atan.eps, k.atan.deg2rad, k.flt_epsilon, k.img_scale, k.deriv_scale, k.second_scale, k.cross_scale};
    for (int i = 0; i < 11; ++i) f[i] = v[i];
    const int u[] = {SIFT_MAX_OCTAVES, SIFT_MAX_OCTAVE_LAYERS, SIFT_MAX_SIDE, SIFT_MAX_FEATURES, SIFT_IMG_BORDER, SIFT_MAX_INTERP_STEPS, SIFT_ORI_BINS,
                     SIFT_DESCR_WIDTH, SIFT_DESCR_BINS, SIFT_DESCR_LEN, SIFT_TILE_W, SIFT_TILE_H, SIFT_HIST_SCALE_LOG2};
    for (int i = 0; i < 13; ++i) c[i] = u[i];
}
extern "C" int sift_params_shim(int nfeatures, int nol, double contrast, double edge, double sigma, int max_w, int max_h, char* msg, int n) {
    return sift_check_params(params(nfeatures, nol, contrast, edge, sigma), max_w, max_h, msg, (size_t)n);
}
extern "C" int sift_image_shim(int w, int h, int c, int max_w, int max_h, char* msg, int n) { return feat_check_image(w, h, c, max_w, max_h, msg, (size_t)n); }
extern "C" long long sift_capacity_shim(int nfeatures, int nol, int max_w, int max_h, int co, int ko, int* cand, int* rows) {
    const SiftParams p = params(nfeatures, nol, 0.04, 10, 1.6);
    sift_capacities(p, max_w, max_h, co, ko, cand, rows);
    return sift_instance_bytes(p, max_w, max_h, *cand, *rows);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("sift_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "sift_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    i, dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    lib.sift_plan_shim.argtypes = [i, dbl, i, i, vp, vp, vp]
    lib.sift_plan_shim.restype = None
    lib.sift_taps_shim.argtypes = [i, dbl, vp, vp, vp, vp, i]
    lib.sift_consts_shim.argtypes = [vp, vp]
    lib.sift_params_shim.argtypes = [i, i, dbl, dbl, dbl, i, i, ctypes.c_char_p, i]
    lib.sift_image_shim.argtypes = [i] * 5 + [ctypes.c_char_p, i]
    lib.sift_capacity_shim.argtypes = [i] * 6 + [vp, vp]
    lib.sift_capacity_shim.restype = ctypes.c_longlong
    return lib


def plan(lib, w, h, nol=3, contrast=0.04):
    pi, ll, oi = np.zeros(7, np.int32), np.zeros(3 + 32, np.int64), np.zeros((16, 5), np.int32)
    lib.sift_plan_shim(nol, contrast, w, h, pi.ctypes.data, ll.ctypes.data, oi.ctypes.data)
    P = dict(zip(("w", "h", "nol", "noct", "ext_tiles", "threshold", "tail_first"), pi.tolist()))
    P["gauss_floats"], P["dog_floats"], P["tmp_floats"] = ll[:3].tolist()
    P["oc"] = [dict(zip(("w", "h", "tx", "ty", "tile_base"), oi[o].tolist()), goff=int(ll[3 + 2 * o]), doff=int(ll[4 + 2 * o])) for o in range(16)]
    return P


SIZES = [(1, 1), (2, 2), (1, 300), (5, 40), (40, 5), (12, 131), (7, 2048), (33, 41), (97, 131), (131, 97), (100, 80), (640, 480), (1241, 376),
         (1000, 1001), (1919, 1081), (4096, 2160), (16384, 16384), (16384, 3)]


def test_octaves_slabs_and_tiles_equal_the_restatement(shim):
    for w, h in SIZES:
        for nol in (1, 3, 8):
            P = plan(shim, w, h, nol)
            sizes = R.octave_sizes(w, h)
            assert (P["w"], P["h"], P["nol"], P["noct"]) == (w, h, nol, len(sizes)), (w, h)
            assert P["tmp_floats"] == 4 * w * h
            g = d = tiles = 0
            for o, (ow, oh) in enumerate(sizes):
                O = P["oc"][o]
                assert (O["w"], O["h"], O["goff"], O["doff"], O["tile_base"]) == (ow, oh, g, d, tiles), (w, h, o)   # in order, no overlap
                g += ow * oh * (nol + 3)
                d += ow * oh * (nol + 2)
                if ow > 10 and oh > 10:
                    assert O["tx"] * 64 >= ow > (O["tx"] - 1) * 64 and O["ty"] * 4 >= oh > (O["ty"] - 1) * 4
                else:
                    assert (O["tx"], O["ty"]) == (0, 0)                         # a side <= 10: no interior, no tile
                tiles += O["tx"] * O["ty"]
            assert (P["gauss_floats"], P["dog_floats"], P["ext_tiles"]) == (g, d, tiles)
            # the octaves one workgroup computes: the trailing run of at most 8 192 pixels, never octave 0
            small = [ow * oh <= 8192 for ow, oh in sizes]
            first = len(sizes)
            while first > 1 and small[first - 1]:
                first -= 1
            assert P["tail_first"] == first, (w, h)
    assert plan(shim, 97, 131)["noct"] == 7 and plan(shim, 1241, 376)["noct"] == 9 and plan(shim, 1, 1)["noct"] == 0
    assert plan(shim, 16384, 16384)["noct"] == 14 <= R.MAX_OCTAVES
    assert plan(shim, 97, 131)["tail_first"] == 2 and plan(shim, 33, 41)["tail_first"] == 1 and plan(shim, 1241, 376)["tail_first"] == 4


def test_the_threshold(shim):
    for nol in range(1, 9):
        for c in (0.04, 0.004, 0.2, 0.3, 0.09, 1e-6, 1.0, 0.0235294117647, 0.02353):
            assert plan(shim, 64, 64, nol, c)["threshold"] == R.threshold(c, nol)
    assert plan(shim, 64, 64, 3, 0.04)["threshold"] == 1 and plan(shim, 64, 64, 1, 0.04)["threshold"] == 5


def test_sigmas_and_taps_bit_for_bit(shim):
    for sigma in (1.6, 1.2, 0.51, 1.0, 2.4, 8.0):
        for nol in range(1, 9):
            n, off, sig, taps = np.zeros(11, np.int32), np.zeros(11, np.int32), np.zeros(11, np.float64), np.zeros(4096, np.float32)
            total = shim.sift_taps_shim(nol, sigma, n.ctypes.data, off.ctypes.data, sig.ctypes.data, taps.ctypes.data, 4096)
            want = R.sigmas(sigma, nol)
            assert sig[:nol + 3].tobytes() == np.array(want, np.float64).tobytes(), (sigma, nol)
            at = 0
            for i, s in enumerate(want):
                t = R.gauss_taps(s)
                assert (n[i], off[i]) == (len(t), at) and len(t) % 2 == 1 and len(t) == (R.cv_round(8 * s + 1) | 1)
                assert taps[at:at + len(t)].tobytes() == t.tobytes(), (sigma, nol, i)
                assert abs(float(t.astype(np.float64).sum()) - 1) < len(t) * 2.0 ** -24
                at += len(t)
            assert total == at
    t = R.gauss_taps(R.sigmas(1.6, 3)[0])
    assert len(t) == 11 and t[5] == t.max() and np.array_equal(t, t[::-1])


def test_constants(shim):
    f, c = np.zeros(11, np.float32), np.zeros(13, np.int32)
    shim.sift_consts_shim(f.ctypes.data, c.ctypes.data)
    p1, p3, p5, p7 = R.ATAN_P
    want = (p1, p3, p5, p7, R.EPS32, R.F32(np.pi / 180.0), R.FLT_EPSILON, R.IMG_SCALE, R.DERIV_SCALE, R.SECOND_SCALE, R.CROSS_SCALE)
    for got, w in zip(f, want):
        assert got.tobytes() == np.float32(w).tobytes()
    assert R.FLT_EPSILON == np.finfo(np.float32).eps
    assert c.tolist() == [R.MAX_OCTAVES, 8, 16384, 1 << 20, R.IMG_BORDER, R.MAX_INTERP_STEPS, R.ORI_BINS, R.DESCR_W, R.DESCR_BINS, 128, 64, 4,
                          R.HIST_SCALE_LOG2]
    # the worst bin at the default sigma, 4 761 samples of magnitude < 361, fits in 63 bits at the plan's scale (with room
    # for the largest accepted sigma: 481^2 samples)
    assert 4761 * 361 * 2 ** R.HIST_SCALE_LOG2 < 2 ** 63 and 481 * 481 * 361 * 2 ** R.HIST_SCALE_LOG2 < 2 ** 63


def test_capacities(shim):
    def cap(nfeatures, w, h, co=0, ko=0, nol=3):
        c, k = ctypes.c_int(0), ctypes.c_int(0)
        b = shim.sift_capacity_shim(nfeatures, nol, w, h, co, ko, ctypes.byref(c), ctypes.byref(k))
        return c.value, k.value, b
    assert cap(0, 1241, 376)[:2] == (4 * 1241 * 376 // 32,) * 2
    assert cap(6000, 1241, 376)[:2] == (4 * 1241 * 376 // 32, 24000)
    assert cap(2048, 1241, 376)[:2] == (4 * 1241 * 376 // 32, 16384)
    assert cap(0, 33, 41)[:2] == (1024, 1024) and cap(6000, 33, 41)[:2] == (1024, 1024)
    assert cap(0, 1241, 376, 100, 0)[:2] == (100, 100) and cap(0, 1241, 376, 0, 7)[:2] == (4 * 1241 * 376 // 32, 7)
    assert cap(500, 131, 97, 242, 238)[:2] == (242, 238)
    # the cost of an instance, by the arithmetic the header states: about 0.15 GB at 1241 x 376, about 2.6 GB at 4096 x 2160
    assert 0.14e9 < cap(6000, 1241, 376)[2] < 0.16e9 and 2.5e9 < cap(6000, 4096, 2160)[2] < 2.7e9
    P = plan(shim, 1241, 376)
    assert cap(0, 1241, 376, 1, 1)[2] == 4 * (P["gauss_floats"] + P["dog_floats"] + 2 * P["tmp_floats"]) + 208 + 576


def test_every_refusal(shim):
    msg = ctypes.create_string_buffer(200)

    def params(nfeatures=0, nol=3, contrast=0.04, edge=10.0, sigma=1.6, max_w=640, max_h=480):
        msg.value = b""
        return shim.sift_params_shim(nfeatures, nol, contrast, edge, sigma, max_w, max_h, msg, 200), msg.value.decode()
    assert params() == (0, "")
    nan = float("nan")
    for kw, word in ((dict(nfeatures=-1), "nfeatures -1"), (dict(nfeatures=(1 << 20) + 1), "nfeatures"), (dict(nol=0), "nOctaveLayers 0"),
                     (dict(nol=9), "nOctaveLayers 9"), (dict(contrast=0.0), "contrastThreshold 0"), (dict(contrast=-0.04), "contrastThreshold"),
                     (dict(contrast=nan), "contrastThreshold"), (dict(edge=0.0), "edgeThreshold 0"), (dict(edge=-10.0), "edgeThreshold"),
                     (dict(edge=float("inf")), "edgeThreshold"), (dict(sigma=0.5), "sigma 0.5"), (dict(sigma=8.5), "sigma 8.5"),
                     (dict(sigma=nan), "sigma"), (dict(sigma=-1.6), "sigma"), (dict(max_w=0), "frame size"), (dict(max_h=16385), "frame size")):
        rc, text = params(**kw)
        assert rc != 0 and word in text, (kw, text)
    assert params(nfeatures=1 << 20)[0] == 0 and params(nol=1, sigma=8.0)[0] == 0 and params(nol=8, sigma=0.5000001, contrast=1e-9, edge=0.5)[0] == 0
    assert R.check_params(nfeatures=-1) == "nfeatures" and R.check_params(nOctaveLayers=9) == "nOctaveLayers" and R.check_params(sigma=0.5) == "sigma"
    assert R.check_params(contrastThreshold=0) == "contrastThreshold" and R.check_params(edgeThreshold=0) == "edgeThreshold" and R.check_params() is None

    def image(w, h, c, max_w=640, max_h=480):
        msg.value = b""
        return shim.sift_image_shim(w, h, c, max_w, max_h, msg, 200), msg.value.decode()
    assert image(640, 480, 1) == (0, "") and image(1, 1, 3)[0] == 0 and image(5, 5, 4)[0] == 0
    for a, word in (((641, 480, 1), "larger than the instance's 640x480"), ((640, 481, 3), "larger"), ((640, 480, 2), "2 channels"),
                    ((0, 480, 1), "frame size"), ((640, 0, 1), "frame size")):
        rc, text = image(*a)
        assert rc != 0 and word in text, (a, text)
