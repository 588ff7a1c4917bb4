"""The LightGlue launch plan (csrc/lg_plan.hpp) on the CPU.  Every hooked kernel form gives bit-identical results, so the GPU
suite cannot see a wrong SELECTION - only the speed would move.  This test compiles the header (plain C++17, no HIP) behind a
small extern "C" shim with the host compiler and compares lg_plan with `parent_plan` below: a Python restatement of the rules
as the host code spelled them before the plan existed (attn_key_split, launch_attention, launch_attention_h, lg_layer_h,
lg_enqueue of the commit before lg_plan.hpp), NOT a transcription of the header."""
import ctypes
import itertools
import shutil
import subprocess

import pytest

from conftest import PKG_NAME, ROOT

SHIM = r"""
#include "lg_plan.hpp"
extern "C" int lg_plan_shim(int precision, int sim_exact, int layers, int self_only, int key_split, int big_gemm, int study,
                            int Kc, int NI, int want_heads, int* o) {
    sslam::LGHooks h;
    h.precision = precision; h.sim_exact = sim_exact != 0; h.layers = layers; h.self_only = self_only != 0;
    h.key_split = key_split; h.big_gemm = big_gemm; h.study = study;
    const sslam::LGPlan p = sslam::lg_plan(h, Kc, NI, want_heads != 0);
    const int v[] = {p.split, p.proj_split, (int)p.attn, p.p_single, p.ks, (int)p.merge, (int)p.linears, (int)p.ffn_tile,
                     p.heads_in_ffn, p.layers, p.self_only_last, sslam::lg_ks_max(Kc)};
    for (int i = 0; i < 12; ++i) o[i] = v[i];
    return sslam::LG_NH * 1000000 + sslam::LG_NL * 10000 + sslam::LG_AQ * 10 + sslam::LG_AK / 64;
}
"""
FIELDS = ("split", "proj_split", "attn", "p_single", "ks", "merge", "linears", "ffn_tile", "heads_in_ffn", "layers",
          "self_only_last", "ks_max")
F32, FOUR_WAVE, ASM = 0, 1, 2           # enum LGAttn
NONE, LAUNCH, IN_FFN = 0, 1, 2          # enum LGMerge
RING, BIG = 0, 1                        # enum LGLinears
T64, T32 = 0, 1                         # enum LGFfnTile

KEY_SPLITS = (-5, -4, -3, -1, 0, 1, 2, 4, 101, 102, 104)      # every value sslam_lightglue_debug_key_split accepts
BIG_GEMMS = (-1, 0, 1, 2, 3, 5)                                # ... and sslam_lightglue_debug_big_gemm
PRECISIONS = (0, 1, 2)
STUDIES = (0, 0x04, 0x10)
KCS = (128, 256, 512, 1024, 2048, 4096, 8192)
NIS = (2, 4, 8, 16, 32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("lg_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "lg_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    fn = ctypes.CDLL(str(so)).lg_plan_shim
    fn.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int)]
    fn.restype = ctypes.c_int
    return fn


def plan(fn, key_split=0, big_gemm=-1, precision=2, study=0, Kc=2048, NI=2, want_heads=True, sim_exact=False, layers=9,
         self_only=False):
    out = (ctypes.c_int * 12)()
    fn(precision, int(sim_exact), layers, int(self_only), key_split, big_gemm, study, Kc, NI, int(want_heads), out)
    return dict(zip(FIELDS, out))


def parent_plan(key_split=0, big_gemm=-1, precision=2, study=0, Kc=2048, NI=2, want_heads=True, sim_exact=False, layers=9,
                self_only=False):
    """What the host code before lg_plan.hpp launched, rule by rule as it was written there."""
    # sslam_lightglue_create_batched: g->KSmax
    ks_max = 4 if Kc >= 1024 else (2 if Kc >= 512 else 1)
    # attn_key_split
    ks = 1
    if key_split > 100:
        ks = key_split - 100
    elif key_split > 0:
        ks = key_split
    elif key_split < 0 and key_split > -4:
        ks = 1
    else:
        units = NI * 4 * (Kc // 128)
        while ks < 4 and units * ks < 256 and Kc // 64 >= 2 * ks * 4:
            ks *= 2
    ks = ks_max if ks > ks_max else ks
    # sslam_lightglue_set_precision: precision = mode == 0 ? 0 : 1, p_single = mode == 2
    split = precision != 0
    p = dict(split=int(split), proj_split=int(split and not sim_exact), ks=ks, ks_max=ks_max, layers=layers,
             self_only_last=int(self_only))
    if not split:
        # lg_enqueue's fp32 branch: launch_attention = lg_attention_kernel + lg_attn_merge_kernel at every ks, fp32 linears,
        # heads_done stays false
        p.update(attn=F32, merge=LAUNCH, heads_in_ffn=0)
        return p
    # launch_attention_h
    asm = not (study & 0x04) and (key_split == 0 or key_split == -3 or key_split == -5 or key_split > 100)
    p_single = bool(study & 0x04) or precision == 2
    # lg_layer_h
    big = (big_gemm != 0) if big_gemm >= 0 else (NI * Kc >= 4096 and Kc % 128 == 0)
    small_tiles = big_gemm == 3 or (big_gemm != 2 and NI * (Kc // 64) <= 128)
    fold = big and small_tiles and ks > 1 and study == 0 and (key_split == 0 or key_split > 100)
    # launch_attention_h: `if (KS == 1 || merge_in_ffn) return;` in front of the merge launch
    merge = NONE if ks == 1 else (IN_FFN if fold else LAUNCH)
    # lg_enqueue: heads = want_heads && big_gemm != 5; lg_layer_h returns big && heads
    p.update(attn=ASM if asm else FOUR_WAVE, p_single=int(p_single), merge=merge, linears=BIG if big else RING,
             ffn_tile=T32 if small_tiles else T64, heads_in_ffn=int(big and want_heads and big_gemm != 5))
    return p


def test_shape_constants_are_the_kernels(shim):
    out = (ctypes.c_int * 12)()
    assert shim(2, 0, 9, 0, 0, -1, 0, 2048, 2, 1, out) == 4 * 1000000 + 9 * 10000 + 128 * 10 + 1      # NH 4, NL 9, AQ 128, AK 64


def test_plan_equals_the_parent_rules_over_the_full_sweep(shim):
    n = 0
    for ks, bg, pr, st, Kc, NI in itertools.product(KEY_SPLITS, BIG_GEMMS, PRECISIONS, STUDIES, KCS, NIS):
        for want_heads in (True, False):
            kw = dict(key_split=ks, big_gemm=bg, precision=pr, study=st, Kc=Kc, NI=NI, want_heads=want_heads)
            got, want = plan(shim, **kw), parent_plan(**kw)
            # (fields the fp32 path never reads - p_single, linears, ffn_tile - are absent from `want` there)
            assert {k: got[k] for k in want} == want, kw
            # what the old code only implied
            assert got["ks"] in (1, 2, 4) and got["ks"] <= got["ks_max"], kw
            if got["merge"] == IN_FFN:
                assert got["attn"] == ASM and got["linears"] == BIG and got["ffn_tile"] == T32 and got["ks"] > 1, kw
            if got["merge"] == NONE:
                assert got["ks"] == 1 and got["split"], kw
            if got["heads_in_ffn"]:
                assert got["split"] and got["linears"] == BIG, kw
            assert (got["attn"] == F32) == (pr == 0), kw
            n += 1
    assert n == 11 * 6 * 3 * 3 * 7 * 5 * 2


def test_layers_self_only_and_sim_exact_pass_through(shim):
    for layers, self_only, sim_exact, pr in itertools.product((1, 3, 9), (False, True), (False, True), PRECISIONS):
        kw = dict(layers=layers, self_only=self_only, sim_exact=sim_exact, precision=pr)
        got, want = plan(shim, **kw), parent_plan(**kw)
        assert {k: got[k] for k in want} == want, kw
        assert got["layers"] == layers and got["self_only_last"] == int(self_only)
        assert got["proj_split"] == int(pr != 0 and not sim_exact)


def test_default_hooks_worked_rows(shim):
    """The shipped selection at the sizes the measurements of DESIGN section 3 were taken at, by hand from the rules."""
    p = plan(shim, Kc=2048, NI=2)             # one 2048-keypoint pair: the drop-in path
    assert (p["ks"], p["attn"], p["merge"], p["linears"], p["ffn_tile"]) == (2, ASM, IN_FFN, BIG, T32)
    assert p["split"] and p["proj_split"] and p["p_single"] and p["heads_in_ffn"] and p["layers"] == 9 and not p["self_only_last"]
    p = plan(shim, Kc=2048, NI=16)            # eight pairs: the benchmark's batch
    assert (p["ks"], p["attn"], p["merge"], p["linears"], p["ffn_tile"]) == (1, ASM, NONE, BIG, T64)
    p = plan(shim, Kc=1024, NI=2)
    assert (p["ks"], p["attn"], p["merge"], p["linears"]) == (4, ASM, LAUNCH, RING)
    assert not p["heads_in_ffn"]
    assert plan(shim, Kc=1024, NI=4)["linears"] == BIG
    assert plan(shim, Kc=512, NI=2)["ks"] == 2
    assert plan(shim, Kc=128, NI=2)["ks"] == 1
    assert plan(shim, Kc=4096, NI=2)["ks"] == 1


def test_hooks_select_what_their_documentation_says(shim):
    one = dict(Kc=2048, NI=2)
    assert plan(shim, key_split=-5, **one)["merge"] == LAUNCH and plan(shim, key_split=-5, **one)["attn"] == ASM
    assert plan(shim, key_split=-4, **one)["attn"] == FOUR_WAVE and plan(shim, key_split=-4, **one)["ks"] == 2
    assert plan(shim, key_split=-3, **one)["ks"] == 1 and plan(shim, key_split=-3, **one)["attn"] == ASM
    assert plan(shim, key_split=-1, **one)["ks"] == 1 and plan(shim, key_split=-1, **one)["attn"] == FOUR_WAVE
    assert plan(shim, key_split=4, **one)["ks"] == 4 and plan(shim, key_split=4, **one)["attn"] == FOUR_WAVE
    assert plan(shim, key_split=104, **one)["ks"] == 4 and plan(shim, key_split=104, **one)["merge"] == IN_FFN
    assert plan(shim, key_split=104, Kc=512, NI=2)["ks"] == 2            # capped by the partial buffers
    assert plan(shim, big_gemm=0, **one)["linears"] == RING and plan(shim, big_gemm=0, **one)["merge"] == LAUNCH
    assert plan(shim, big_gemm=2, **one)["ffn_tile"] == T64 and plan(shim, big_gemm=2, **one)["merge"] == LAUNCH
    assert plan(shim, big_gemm=3, Kc=2048, NI=16)["ffn_tile"] == T32
    assert not plan(shim, big_gemm=5, **one)["heads_in_ffn"] and plan(shim, big_gemm=5, **one)["linears"] == BIG
    assert plan(shim, study=0x04, **one)["attn"] == FOUR_WAVE and plan(shim, study=0x04, precision=1, **one)["p_single"]
    assert plan(shim, study=0x10, **one)["merge"] == LAUNCH and plan(shim, study=0x10, **one)["attn"] == ASM
    assert not plan(shim, precision=1, **one)["p_single"]
    p = plan(shim, precision=0, Kc=2048, NI=16)
    assert (p["attn"], p["ks"], p["merge"], p["proj_split"], p["heads_in_ffn"]) == (F32, 1, LAUNCH, 0, 0)
