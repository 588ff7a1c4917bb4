"""The ALIKED call plan (csrc/al_plan.hpp) on the CPU.  Everything the host decides about one extraction - the resize rule and
padding, the launch splits of every kernel, whether the instance takes the frame, the workspace extents - is integer and
double arithmetic over about 2 000 legal network sizes times 16 batch sizes, of which the GPU suite samples a dozen.  This test
compiles the header (plain C++17, no HIP) behind a small extern "C" shim with the host compiler and compares it with
 - the project's oracle (oracle/aliked_ref.py: resize_plan, pad_amounts) for the sizes, and
 - `parent_plan` / `parent_extents` / `parent_debug_cap` below: Python restatements of the arithmetic as the host code spelled it
   between its launches before the plan existed (resize_plan, al_dims, al_enqueue, carve_frame and sslam_aliked_debug_read of
   the commit before al_plan.hpp), NOT transcriptions of the header."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from oracle import aliked_ref as R

INTS = ("F", "KF", "blur", "ky", "kx", "H", "W", "C", "h", "w", "Hp", "Wp", "pl", "pt", "to_float_gx", "pad_gx",
        "b1_strips", "b1_nblk", "b1_hs", "b1_nb", "b2_strips", "b2_nblk", "b2_hs", "b2_nb", "b2_waves", "b2_gx",
        "H2", "W2", "HW2", "H3", "W3", "HW3", "H4", "W4", "HW4", "pool3_gx", "pool4_gx", "off3_gx", "dcn3_gx", "off4_gx",
        "dcn4_gx", "gate2_gx", "gate3_gx", "gate4_gx", "gate34_gx", "agg_pre_gx", "tail_gx", "tail_gy", "nbx", "nby",
        "n_tiles", "nms_gx", "npx", "collect_gx", "agg_tile")
FLOATS = ("sy", "sx", "mo3", "mo4", "mo", "sy2", "sx2", "sy8", "sx8", "sy32", "sx32", "scale_x", "scale_y")
KPT = ("NK", "refine_gx", "patch_gx", "offsets_gx", "sample_gx", "finalize_gx", "rows_x16", "rows64", "rows64_x16", "plane")
EXTENTS = ("ctrl", "in_u8", "fsrc", "img", "x1", "x2", "p3", "off", "t3", "x3", "p3cl", "t3cl", "p4cl", "t4cl", "p4", "t4", "x4",
           "g2", "g3", "g4", "g2cl", "g3cl", "g4cl", "s8", "rnorm", "g1cl", "pre2", "pre3", "pre4", "score", "nms", "bsum",
           "cand", "hist", "kp_index", "sel_keys", "kp_norm", "kp_score", "patch", "h32", "pos", "sampled", "feats", "raw",
           "out_xy", "out_desc", "out_score", "out_n")
CONSTANTS = ("AL_LONG_SIDE", "AL_PAD_DIV", "MAX_FRAMES", "B1_SW", "B2_SW", "DCN3_CS", "DCN4_CS", "AGG_PRE", "ST_W", "ST_H",
             "NHALO", "NW_R", "NW_OW", "NW_OH", "HBINS", "COLLECT_PPT", "SEL_CAP", "EDGE_CAP", "CAND_CAP", "REFINE_KPB",
             "SDDH_KSPLIT")
T64x64, T64x128 = 0, 1                      # enum ALAggTile
NONE, SIZE, FRAMES, BLUR = 0, 1, 2, 3       # enum ALRefusal

SHIM = r"""
#include "al_plan.hpp"
using namespace sslam;
extern "C" void al_plan_shim(int H, int W, int C, int F, int* o, float* f) {
    const ALPlan p = al_plan(H, W, C, F);
    const Dims& d = p.d;
    const int v[] = {%s};
    const float w[] = {%s};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
    for (size_t i = 0; i < sizeof(w) / sizeof(w[0]); ++i) f[i] = w[i];
}
// kx, ky >= 0 replace the plan's taps (no legal image reaches the blur refusal)
extern "C" int al_refusal_shim(int H, int W, int C, int F, int kx, int ky, int Hp_cap, int Wp_cap, int max_frames, char* msg, int n) {
    ALPlan p = al_plan(H, W, C, F);
    if (kx >= 0) p.kx = kx;
    if (ky >= 0) p.ky = ky;
    return (int)al_refusal(p, Hp_cap, Wp_cap, max_frames, msg, (size_t)n);
}
extern "C" void al_kpt_shim(int NK, long long* o) {
    const ALKptPlan k = al_kpt_plan(NK);
    const long long v[] = {%s};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}
extern "C" void al_extents_shim(long long HWp, long long HWi, long long NK, long long* o) {
    const ALExtents e = al_extents((size_t)HWp, (size_t)HWi, (size_t)NK);
    const size_t v[] = {%s};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = (long long)v[i];
}
extern "C" void al_constants_shim(int* o) {
    const int v[] = {%s};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) o[i] = v[i];
}
extern "C" int al_dims_bytes() { return (int)sizeof(Dims); }
""" % (", ".join(("d." if n in ("H", "W", "C", "h", "w", "Hp", "Wp", "pl", "pt") else "p.") + n if n != "agg_tile" else "(int)p.agg_tile"
                 for n in INTS),
       ", ".join("p." + n for n in FLOATS), ", ".join("(long long)k." + n for n in KPT), ", ".join("e." + n for n in EXTENTS),
       ", ".join(CONSTANTS))

# The sweep.  A "network size" is what the launch sequence sees of a frame: (h, w) and the blur taps (ky, kx).  These heights
# and widths reach 3 623 distinct ones, 3 583 of them legal, with blur taps up to 15 (3 621 / 3 581 without H = 2100)
HEIGHTS = list(range(16, 2101)) + [4096, 8192]
WIDTHS = (16, 17, 31, 32, 33, 64, 100, 131, 480, 640, 1000, 1024, 1241, 1280, 1920, 2048, 2064, 4096, 8192)
CAP = 1024 + 32                             # sslam_aliked_create_batched: Hp_cap = Wp_cap


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("al_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "al_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    lib.al_plan_shim.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)]
    lib.al_plan_shim.restype = None
    lib.al_refusal_shim.argtypes = [ctypes.c_int] * 9 + [ctypes.c_char_p, ctypes.c_int]
    lib.al_kpt_shim.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
    lib.al_kpt_shim.restype = None
    lib.al_extents_shim.argtypes = [ctypes.c_longlong] * 3 + [ctypes.POINTER(ctypes.c_longlong)]
    lib.al_extents_shim.restype = None
    return lib


_OI, _OF = (ctypes.c_int * len(INTS))(), (ctypes.c_float * len(FLOATS))()


def plan(lib, H, W, C=3, F=1):
    lib.al_plan_shim(H, W, C, F, _OI, _OF)
    p = dict(zip(INTS, _OI))
    p.update(zip(FLOATS, (np.float32(x) for x in _OF)))
    return p


def refusal(lib, H, W, F=1, kx=-1, ky=-1, Hp_cap=CAP, Wp_cap=CAP, max_frames=16):
    msg = ctypes.create_string_buffer(160)
    rc = lib.al_refusal_shim(H, W, 3, F, kx, ky, Hp_cap, Wp_cap, max_frames, msg, 160)
    return rc, msg.value.decode()


def extents(lib, HWp, HWi, NK):
    out = (ctypes.c_longlong * len(EXTENTS))()
    lib.al_extents_shim(HWp, HWi, NK, out)
    return dict(zip(EXTENTS, out))


def constants(lib):
    out = (ctypes.c_int * len(CONSTANTS))()
    lib.al_constants_shim(out)
    return dict(zip(CONSTANTS, out))


def cdiv(a, b):
    return (a + b - 1) // b


def f32(x):
    return np.float32(x)


def parent_plan(H, W, C, F):
    """What the parent's entry points and al_enqueue computed for one call, rule by rule as they were written there."""
    # resize_plan(H, W, 1024)
    ar = W / H
    if ar > 1.0:
        h, w = int(1024 / ar), 1024
    else:
        h, w = 1024, int(1024 * ar)
    fy, fx = H / h, W / w
    blur = int(max(fy, fx) > 1.0)
    sgy = (fy - 1.0) / 2.0 if (fy - 1.0) / 2.0 > 0.001 else 0.001
    sgx = (fx - 1.0) / 2.0 if (fx - 1.0) / 2.0 > 0.001 else 0.001
    ksy, ksx = 2.0 * 2 * sgy, 2.0 * 2 * sgx
    ky, kx = int(ksy if ksy > 3 else 3), int(ksx if ksx > 3 else 3)
    ky += ky % 2 == 0
    kx += kx % 2 == 0
    # al_dims
    pad_h, pad_w = (((h // 32) + 1) * 32 - h) % 32, (((w // 32) + 1) * 32 - w) % 32
    Hp, Wp, pl, pt = h + pad_h, w + pad_w, pad_w // 2, pad_h // 2
    q = dict(F=F, KF=4 * F, blur=blur, ky=ky, kx=kx, sy=f32(sgy), sx=f32(sgx), H=H, W=W, C=C, h=h, w=w, Hp=Hp, Wp=Wp, pl=pl, pt=pt)
    # al_enqueue, launch by launch
    q.update(to_float_gx=cdiv(W, 256), pad_gx=cdiv(Wp, 256))                     # al_to_float, al_resize_pad (and al_aggregate)
    strips = cdiv(Wp, 30)                                                         # block1
    nblk = max(1, min(cdiv(Hp, 4), 3072 // max(1, strips * F)))
    hs1 = cdiv(Hp, nblk)
    q.update(b1_strips=strips, b1_nblk=nblk, b1_hs=hs1, b1_nb=cdiv(Hp, hs1))
    H2, W2 = Hp // 2, Wp // 2                                                     # block2
    strips = cdiv(W2, 30)
    nblk = max(1, min(cdiv(H2, 3), 1024 // max(1, strips * F)))
    hs2 = cdiv(H2, nblk)
    nb = cdiv(H2, hs2)
    n_waves = strips * nb * F
    q.update(H2=H2, W2=W2, HW2=H2 * W2, b2_strips=strips, b2_nblk=nblk, b2_hs=hs2, b2_nb=nb, b2_waves=n_waves, b2_gx=cdiv(n_waves, 4))
    H3, W3 = Hp // 8, Wp // 8                                                     # block3: DCN3_CS = 1
    HW3 = H3 * W3
    q.update(H3=H3, W3=W3, HW3=HW3, pool3_gx=cdiv(32 * HW3, 256), off3_gx=cdiv(W3, 32), dcn3_gx=1 * cdiv(W3, 32),
             mo3=f32(max(H3, W3)) / f32(4.0))
    H4, W4 = Hp // 32, Wp // 32                                                   # block4: DCN4_CS = 4
    HW4 = H4 * W4
    q.update(H4=H4, W4=W4, HW4=HW4, pool4_gx=cdiv(64 * HW4, 256), off4_gx=cdiv(W4, 32), dcn4_gx=4 * cdiv(W4, 32),
             mo4=f32(max(H4, W4)) / f32(4.0))
    ba, bb = cdiv(32 * HW3, 256), cdiv(32 * HW4, 256)                             # gates
    q.update(gate2_gx=cdiv(H2 * W2, 256), gate3_gx=ba, gate4_gx=bb, gate34_gx=ba + bb)
    step = lambda full, S: f32(full // S - 1) / f32(full - 1)                     # Pyr
    q.update(sy2=step(Hp, 2), sx2=step(Wp, 2), sy8=step(Hp, 8), sx8=step(Wp, 8), sy32=step(Hp, 32), sx32=step(Wp, 32))
    q.update(agg_pre_gx=cdiv(H2 * W2 + HW3 + HW4, 256), tail_gx=cdiv(Wp, 32), tail_gy=cdiv(Hp, 8))
    nbx, nby, npx = cdiv(w, 64 - 2 * 10), cdiv(h, 48 - 2 * 10), h * w             # DKD
    q.update(nbx=nbx, nby=nby, n_tiles=nbx * nby, nms_gx=cdiv(nbx * nby, 4), npx=npx, collect_gx=cdiv(npx, 256 * 16))
    q.update(mo=f32(max(h, w)) / f32(4.0), agg_tile=T64x128 if F >= 4 else T64x64,
             scale_x=f32(w) / f32(W), scale_y=f32(h) / f32(H))
    return q


def parent_refusal(q, Hp_cap, Wp_cap, max_frames):
    """The three SSLAM_REQUIREs of the parent's al_enqueue, in their order."""
    if not (q["Hp"] <= Hp_cap and q["Wp"] <= Wp_cap and q["h"] >= 8 and q["w"] >= 8):
        return SIZE, "sslam_aliked: network size %dx%d outside the instance capacity %dx%d" % (q["Hp"], q["Wp"], Hp_cap, Wp_cap)
    if not (1 <= q["F"] <= max_frames):
        return FRAMES, "sslam_aliked: %d frames, instance capacity %d" % (q["F"], max_frames)
    if not (q["kx"] <= 31 and q["ky"] <= 31):
        return BLUR, "sslam_aliked: blur kernel too large (%d,%d)" % (q["kx"], q["ky"])
    return NONE, ""


def parent_extents(HWp, HWi, NK):
    """carve_frame of the parent's sslam_aliked_create_batched, buffer by buffer."""
    return dict(ctrl=1, in_u8=HWi * 4, fsrc=3 * HWi, img=3 * HWp, x1=16 * HWp, x2=32 * HWp // 4, p3=32 * HWp // 64,
                off=18 * HWp // 64, t3=64 * HWp // 64, x3=64 * HWp // 64, p3cl=32 * HWp // 64, t3cl=64 * HWp // 64,
                p4cl=64 * HWp // 1024, t4cl=128 * HWp // 1024, p4=64 * HWp // 1024, t4=128 * HWp // 1024, x4=128 * HWp // 1024,
                g2=32 * HWp // 4, g3=32 * HWp // 64, g4=32 * HWp // 1024, g2cl=32 * HWp // 4, g3cl=32 * HWp // 64,
                g4cl=32 * HWp // 1024, s8=8 * HWp, rnorm=HWp, g1cl=32 * HWp, pre2=13 * HWp // 4, pre3=13 * HWp // 64,
                pre4=13 * HWp // 1024, score=HWp, nms=HWp, bsum=4096, cand=1024 * 1024, hist=4096, kp_index=8192, sel_keys=8192,
                kp_norm=2 * NK + 64, kp_score=NK + 64, patch=(NK + 64) * 1152, h32=4 * (NK + 64) * 32, pos=NK * 32 + 64,
                sampled=(NK * 16 + 64) * 128, feats=(NK * 16 + 64) * 128, raw=4 * (NK + 64) * 128, out_xy=2 * NK,
                out_desc=NK * 128, out_score=NK, out_n=16)


def parent_debug_cap(q, NK):
    """`cap` (bytes) of every case of the parent's sslam_aliked_debug_read, and the buffer it reads."""
    HWp, hw = q["Hp"] * q["Wp"], q["h"] * q["w"]
    return {0: ("score", hw * 4), 1: ("kp_index", 8192 * 4), 3: ("x1", 16 * HWp * 4), 4: ("x2", 32 * HWp // 4 * 4),
            5: ("x3", 64 * HWp // 64 * 4), 6: ("x4", 128 * HWp // 1024 * 4), 7: ("img", 3 * HWp * 4), 8: ("nms", hw * 4),
            9: ("kp_norm", NK * 8), 10: ("g1cl", 32 * HWp * 4), 11: ("rnorm", HWp * 4), 12: ("g2", 32 * HWp // 4 * 4),
            13: ("g3", 32 * HWp // 64 * 4), 14: ("g4", 32 * HWp // 1024 * 4), 15: ("pre2", 13 * HWp // 4 * 4),
            16: ("pre3", 13 * HWp // 64 * 4), 17: ("pre4", 13 * HWp // 1024 * 4), 18: ("s8", 8 * HWp * 4), 19: ("pos", NK * 32 * 4),
            20: ("patch", NK * 1152 * 4)}


def debug_cap(lib, q, NK):
    """The same caps as the head's sslam_aliked_debug_read forms them: the extents of the last frame's sizes, but 0 and 8 the
    un-padded map and 9, 19, 20 the bare max_kpts rows (1 is SEL_CAP through the extents)."""
    e = extents(lib, q["Hp"] * q["Wp"], q["H"] * q["W"], NK)
    by_extent = {1: "kp_index", 3: "x1", 4: "x2", 5: "x3", 6: "x4", 7: "img", 10: "g1cl", 11: "rnorm", 12: "g2", 13: "g3", 14: "g4",
                 15: "pre2", 16: "pre3", 17: "pre4", 18: "s8"}
    cap = {which: (name, e[name] * 4) for which, name in by_extent.items()}
    cap.update({0: ("score", q["h"] * q["w"] * 4), 8: ("nms", q["h"] * q["w"] * 4), 9: ("kp_norm", NK * 8),
                19: ("pos", NK * 32 * 4), 20: ("patch", NK * 1152 * 4)})
    return cap


@pytest.fixture(scope="module")
def sweep(shim):
    """Every (H, W) of the sweep once: Dims and the resize parameters against the oracle on the way, and one (H, W) per distinct
    network size (h, w, ky, kx) for the tests of what depends on the network size alone."""
    sizes, n, max_taps = {}, 0, 0
    for a in HEIGHTS:
        for b in WIDTHS:
            for H, W in ((a, b), (b, a)):
                p = plan(shim, H, W)
                rp = R.resize_plan(H, W)
                l, r, t, bt = R.pad_amounts(rp["new_h"], rp["new_w"])
                want = dict(H=H, W=W, C=3, h=rp["new_h"], w=rp["new_w"], Hp=rp["new_h"] + t + bt, Wp=rp["new_w"] + l + r, pl=l, pt=t,
                            blur=int(rp["blur"]), ky=rp["ky"], kx=rp["kx"], sy=f32(rp["sigma_y"]), sx=f32(rp["sigma_x"]))
                assert {k: p[k] for k in want} == want, (H, W)
                sizes.setdefault((p["h"], p["w"], p["ky"], p["kx"]), (H, W))
                if p["h"] >= 8 and p["w"] >= 8:
                    max_taps = max(max_taps, p["kx"], p["ky"])
                n += 1
    assert n == len(HEIGHTS) * len(WIDTHS) * 2
    return sizes, max_taps


def _legal(sizes):
    return {k: HW for k, HW in sizes.items() if k[0] >= 8 and k[1] >= 8}


def test_shape_constants_are_the_kernels(shim):
    assert constants(shim) == dict(AL_LONG_SIDE=1024, AL_PAD_DIV=32, MAX_FRAMES=16, B1_SW=30, B2_SW=30, DCN3_CS=1, DCN4_CS=4,
                                   AGG_PRE=13, ST_W=32, ST_H=8, NHALO=10, NW_R=48, NW_OW=44, NW_OH=28, HBINS=4096, COLLECT_PPT=16,
                                   SEL_CAP=8192, EDGE_CAP=2048, CAND_CAP=1024 * 1024, REFINE_KPB=32, SDDH_KSPLIT=4)
    assert shim.al_dims_bytes() == 9 * 4          # nine ints, by value into the kernels


def test_dims_equal_the_oracle_over_the_whole_sweep(sweep):
    sizes, max_taps = sweep                        # (the comparison itself runs in the fixture, once)
    assert len(sizes) == 3623 and len(_legal(sizes)) == 3583 and max_taps == 15


# every launch of al_enqueue whose grid depends on the frame: the plan fields (or None = 1) it builds its dim3 from
GRIDS = dict(reset=("F", None, None), to_float=("to_float_gx", "H", "F"), resize_pad=("pad_gx", "Hp", "F"),
             block1=("b1_strips", "b1_nb", "F"), block2=("b2_gx", None, None), pool3=("pool3_gx", "F", None),
             off3=("off3_gx", "H3", "F"), dcn3=("dcn3_gx", "H3", "F"), pool4=("pool4_gx", "F", None), off4=("off4_gx", "H4", "F"),
             dcn4=("dcn4_gx", "H4", "F"), gate2=("gate2_gx", "F", None), gate34=("gate34_gx", "F", None),
             agg_pre=("agg_pre_gx", "F", None), aggregate=("pad_gx", "Hp", "F"), score_tail=("tail_gx", "tail_gy", "F"),
             nms=("nms_gx", "F", None), collect=("collect_gx", "F", None), select=("F", None, None), kpt_gemm=(None, None, "KF"))


def test_splits_equal_the_parent_rules_for_every_legal_size_and_batch(shim, sweep):
    legal = _legal(sweep[0])
    n = 0
    for H, W in legal.values():
        for F in range(1, 17):
            got, want = plan(shim, H, W, 3, F), parent_plan(H, W, 3, F)
            assert set(want) == set(INTS) | set(FLOATS)
            assert got == want, (H, W, F, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
            # what the old code only implied: both row splits cover their level, with no empty block ...
            for rows, hs, nb, floor in ((got["Hp"], got["b1_hs"], got["b1_nb"], 4), (got["H2"], got["b2_hs"], got["b2_nb"], 3)):
                assert nb * hs >= rows > (nb - 1) * hs and hs >= floor, (H, W, F)
            assert got["b2_waves"] == got["b2_strips"] * got["b2_nb"] * F and 4 * got["b2_gx"] >= got["b2_waves"], (H, W, F)
            assert got["b1_strips"] * 30 >= got["Wp"] and got["b2_strips"] * 30 >= got["W2"], (H, W, F)
            # ... the NMS tiles cover the score map and their partial sums fit al_nms_wave_kernel's `bsum`
            assert got["nbx"] * 44 >= got["w"] and got["nby"] * 28 >= got["h"] and got["n_tiles"] <= 4096, (H, W, F)
            # ... and every grid is one the device takes
            for name, dims in GRIDS.items():
                x, y, z = (1 if f is None else got[f] for f in dims)
                assert 1 <= x < 2 ** 31 and 1 <= y <= 65535 and 1 <= z <= 65535, (name, H, W, F)
            n += 1
    assert n == 3583 * 16


def test_refusals_are_the_parents(shim, sweep):
    sizes = sweep[0]
    refused = 0
    for (h, w, _, _), (H, W) in sizes.items():     # an instance as sslam_aliked_create_batched builds it
        got = refusal(shim, H, W)
        assert got == parent_refusal(parent_plan(H, W, 3, 1), CAP, CAP, 16), (H, W)
        assert (got[0] != NONE) == (h < 8 or w < 8), (H, W)
        refused += got[0] != NONE
    assert refused == 3623 - 3583
    assert refusal(shim, 16, 2064) == (SIZE, "sslam_aliked: network size 32x1024 outside the instance capacity 1056x1056")
    assert plan(shim, 16, 2064)["h"] == 7 and refusal(shim, 16, 2048) == (NONE, "")
    assert refusal(shim, 2064, 16)[0] == SIZE and refusal(shim, 2048, 16)[0] == NONE
    for H, W in ((376, 1241), (16, 2048), (16, 2064), (1024, 1024), (1023, 1024)):
        q = parent_plan(H, W, 3, 1)
        for caps in ((CAP, CAP), (q["Hp"], q["Wp"]), (q["Hp"] - 1, CAP), (CAP, q["Wp"] - 1)):      # size over capacity
            for F, mf in ((0, 1), (1, 1), (2, 1), (16, 16), (17, 16), (5, 4), (-1, 16)):           # F outside [1, max_frames]
                for kx, ky in ((-1, -1), (31, 31), (33, 3), (3, 33)):                              # blur taps over 31
                    q = parent_plan(H, W, 3, F)
                    if kx >= 0:
                        q["kx"], q["ky"] = kx, ky
                    assert refusal(shim, H, W, F, kx, ky, caps[0], caps[1], mf) == parent_refusal(q, caps[0], caps[1], mf), (H, W, caps, F, mf, kx, ky)
    assert refusal(shim, 376, 1241, 17, 33, 3)[0] == FRAMES and refusal(shim, 376, 1241, 16, 33, 3) == (
        BLUR, "sslam_aliked: blur kernel too large (33,3)")
    assert refusal(shim, 376, 1241, 3, max_frames=2) == (FRAMES, "sslam_aliked: 3 frames, instance capacity 2")


def test_extents_are_the_parents_and_debug_read_stays_inside_them(shim, sweep):
    for max_h, max_w, NK in ((16, 16, 1), (376, 1241, 2048), (1200, 2048, 4000), (8192, 8192, 8192), (16, 2064, 1024)):
        carved = extents(shim, CAP * CAP, max_h * max_w, NK)
        assert carved == parent_extents(CAP * CAP, max_h * max_w, NK), (max_h, max_w, NK)
    NK = 1024
    carved = extents(shim, CAP * CAP, 8192 * 8192, NK)
    for H, W in _legal(sweep[0]).values():
        q = plan(shim, H, W)
        got, want = debug_cap(shim, q, NK), parent_debug_cap(q, NK)
        assert got == want, (H, W)
        for which, (name, cap) in got.items():
            assert cap <= carved[name] * 4, (H, W, which)
    assert set(parent_debug_cap(q, NK)) == set(range(21)) - {2}


def test_keypoint_grids_equal_the_parent_rules(shim):
    for NK in (1, 3, 31, 32, 33, 63, 64, 65, 1000, 1024, 2048, 4000, 4096, 8191, 8192):
        out = (ctypes.c_longlong * len(KPT))()
        shim.al_kpt_shim(NK, out)
        # al_enqueue: al_refine, al_patch, al_offsets, al_sample, al_finalize; the row counts of the three GEMMs; `plane`
        want = dict(NK=NK, refine_gx=cdiv(NK, 32), patch_gx=cdiv(NK * 3, 4), offsets_gx=cdiv(NK * 32, 256), sample_gx=cdiv(NK * 16, 4),
                    finalize_gx=cdiv(NK, 4), rows_x16=NK * 16, rows64=cdiv(NK, 64), rows64_x16=cdiv(NK * 16, 64),
                    plane=(NK * 16 + 64) * 128)
        assert dict(zip(KPT, out)) == want
        assert all(1 <= v < 2 ** 31 for k, v in want.items() if k != "plane") and want["rows64"] <= 65535 and want["rows64_x16"] <= 65535
        assert 2 * want["plane"] * 2 == parent_extents(0, 0, NK)["sampled"] * 4       # (hi, lo) fp16 planes fill the fp32 buffer


def test_worked_rows(shim):
    """By hand from the rules."""
    p = plan(shim, 376, 1241)                  # KITTI: 1024 / (1241 / 376) = 310.2...; 320 - 310 = 10 rows of padding, 5 on top
    assert (p["h"], p["w"], p["Hp"], p["Wp"], p["pt"], p["pl"]) == (310, 1024, 320, 1024, 5, 0)
    # F = 1: block1 35 strips (1024 / 30 = 34.1...), min(320 / 4 = 80, 3072 // 35 = 87) = 80 blocks of 4 rows; block2 on 160 x 512:
    # 18 strips, min(ceil(160 / 3) = 54, 1024 // 18 = 56) = 54 -> 3 rows, 54 blocks, 972 waves in 243 workgroups
    assert (p["b1_strips"], p["b1_nblk"], p["b1_hs"], p["b1_nb"]) == (35, 80, 4, 80)
    assert (p["b2_strips"], p["b2_nblk"], p["b2_hs"], p["b2_nb"], p["b2_waves"], p["b2_gx"]) == (18, 54, 3, 54, 972, 243)
    assert (p["nbx"], p["nby"], p["n_tiles"], p["nms_gx"], p["npx"], p["collect_gx"]) == (24, 12, 288, 72, 317440, 78)
    assert (p["H3"], p["W3"], p["H4"], p["W4"], p["off3_gx"], p["dcn4_gx"]) == (40, 128, 10, 32, 4, 4)
    assert (p["mo3"], p["mo4"], p["mo"], p["agg_tile"]) == (32.0, 8.0, 256.0, T64x64)
    assert p["sy2"] == f32(159) / f32(319) and p["sx32"] == f32(31) / f32(1023) and p["scale_y"] == f32(310) / f32(376)
    # F = 16: 3072 // (35 * 16) = 5 blocks of 64 rows; 1024 // (18 * 16) = 3 blocks of 54 rows (the last one 52), 864 waves
    p = plan(shim, 376, 1241, 3, 16)
    assert (p["b1_strips"], p["b1_nblk"], p["b1_hs"], p["b1_nb"]) == (35, 5, 64, 5)
    assert (p["b2_strips"], p["b2_nblk"], p["b2_hs"], p["b2_nb"], p["b2_waves"], p["b2_gx"]) == (18, 3, 54, 3, 864, 216)
    assert (p["KF"], p["agg_tile"]) == (64, T64x128) and plan(shim, 376, 1241, 3, 3)["agg_tile"] == T64x64
    assert plan(shim, 376, 1241, 3, 4)["agg_tile"] == T64x128
    p = plan(shim, 16, 2048)                   # 1024 / 128 = 8 rows, 24 of padding
    assert (p["h"], p["w"], p["Hp"], p["Wp"], p["pt"], p["pl"]) == (8, 1024, 32, 1024, 12, 0)
    assert (p["b1_nblk"], p["b1_hs"], p["b1_nb"], p["b2_nblk"], p["b2_hs"], p["b2_nb"]) == (8, 4, 8, 6, 3, 6)
    assert (p["H4"], p["nby"], p["sy32"]) == (1, 1, 0.0)
    p = plan(shim, 20, 640)                    # 1024 / 32 = 32 rows: no padding
    assert (p["h"], p["w"], p["Hp"], p["Wp"], p["pt"], p["pl"]) == (32, 1024, 32, 1024, 0, 0)
    p = plan(shim, 640, 24)                    # the transpose of 24 x 640: 38 columns in 64, 13 on the left
    assert (p["h"], p["w"], p["Hp"], p["Wp"], p["pt"], p["pl"]) == (1024, 38, 1024, 64, 0, 13)
    assert (p["b1_strips"], p["b2_strips"], p["nbx"], p["off4_gx"], p["dcn4_gx"]) == (3, 2, 1, 1, 4)
