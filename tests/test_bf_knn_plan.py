"""The k-NN matcher's host plan (csrc/bf_knn_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small
extern "C" shim with the host compiler and swept over the sizes - the list length, the splits (chosen, requested, refused),
the split ranges, which must tile the train tiles exactly once, and the scratch formula."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

SHIM = r"""
#include "bf_knn_plan.hpp"
using namespace sslam;
// out: K, row_tiles, tiles, S;  begin: S + 1 entries (cap of them at most);  returns the scratch bytes, -1 when refused
extern "C" long long bfk_plan_shim(int M, int N, int k, int splits, int* out, int* begin, int cap, char* msg, int n) {
    if (bfk_check_k("who", k, msg, (size_t)n) || bfk_check_splits("who", splits, N, msg, (size_t)n)) return -1;
    const BfKnnPlan p = bfk_plan(M, N, k, splits);
    out[0] = p.K; out[1] = p.row_tiles; out[2] = p.tiles; out[3] = p.S;
    for (int s = 0; s <= p.S && s < cap; ++s) begin[s] = p.begin(s);
    return (long long)p.scratch_bytes;
}
extern "C" void bfk_consts_shim(int* c) { c[0] = BFK_TILE; c[1] = BFK_MIN_K; c[2] = BFK_MAX_K; c[3] = BFK_TARGET_WORKGROUPS; }
"""

SIZES = (1, 63, 64, 65, 257, 2048, 4000, 65536)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("bf_knn_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "bf_knn_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    i, vp = ctypes.c_int, ctypes.c_void_p
    lib.bfk_plan_shim.argtypes = [i, i, i, i, vp, vp, i, ctypes.c_char_p, i]
    lib.bfk_plan_shim.restype = ctypes.c_longlong
    lib.bfk_consts_shim.argtypes = [vp]
    lib.bfk_consts_shim.restype = None
    return lib


def plan(lib, M, N, k, splits=0):
    out, begin, msg = np.zeros(4, np.int32), np.full(1026, -1, np.int32), ctypes.create_string_buffer(200)
    b = lib.bfk_plan_shim(M, N, k, splits, out.ctypes.data, begin.ctypes.data, len(begin), msg, 200)
    if b < 0:
        return None, msg.value.decode()
    K, row_tiles, tiles, S = out.tolist()
    return dict(K=K, row_tiles=row_tiles, tiles=tiles, S=S, begin=begin[:S + 1].tolist(), scratch=b), ""


def _tiles_exactly_once(P):
    b = P["begin"]
    assert b[0] == 0 and b[-1] == P["tiles"] and len(b) == P["S"] + 1
    sizes = np.diff(b)
    assert (sizes >= 1).all() and sizes.max() - sizes.min() <= 1            # none empty, uneven by one at most


def test_constants(shim):
    c = np.zeros(4, np.int32)
    shim.bfk_consts_shim(c.ctypes.data)
    assert c.tolist() == [64, 1, 8, 512]


def test_sweep_list_length_splits_ranges_and_scratch(shim):
    for M in SIZES:
        for N in SIZES:
            tiles, row_tiles = -(-N // 64), -(-M // 64)
            for k in range(1, 9):
                P, _ = plan(shim, M, N, k)
                K = 2 if k <= 2 else 4 if k <= 4 else 8
                assert (P["K"], P["row_tiles"], P["tiles"]) == (K, row_tiles, tiles), (M, N, k)
                assert 1 <= P["S"] <= tiles
                assert P["S"] == min(max(-(-512 // row_tiles), 1), tiles)   # the grid fills 256 compute units about twice
                assert P["scratch"] == 8 * P["S"] * M * K
                assert P["scratch"] <= 8 * 2 ** 20                          # a few MB whatever the size
                _tiles_exactly_once(P)
    assert plan(shim, 2048, 2048, 2)[0]["S"] == 16 and plan(shim, 2048, 2048, 2)[0]["begin"] == list(range(0, 33, 2))
    assert plan(shim, 65536, 65536, 8)[0]["S"] == 1
    assert plan(shim, 64, 65536, 8)[0]["S"] == 512


def test_a_requested_split_count_is_honoured(shim):
    for M, N in ((257, 191), (1025, 2049), (64, 65536), (1, 1)):
        tiles = -(-N // 64)
        for S in sorted({1, 2, 3, tiles // 2, tiles - 1, tiles} & set(range(1, tiles + 1))):
            for k in (1, 3, 8):
                P, _ = plan(shim, M, N, k, S)
                assert P["S"] == S and P["scratch"] == 8 * S * M * P["K"]
                _tiles_exactly_once(P)
    P, _ = plan(shim, 300, 1000, 2, 16)                                      # 16 tiles, one each
    assert P["begin"] == list(range(17))
    P, _ = plan(shim, 300, 5 * 64, 2, 3)                                     # 5 tiles over 3 splits: 1 + 2 + 2
    assert P["begin"] == [0, 1, 3, 5]


def test_illegal_values_are_refused_with_a_message(shim):
    for k in (0, -1, 9, 100):
        assert plan(shim, 10, 10, k) == (None, f"who: k {k} outside 1..8")
    for N, S in ((191, 4), (191, -1), (64, 2), (65536, 1025), (1, 2)):
        P, msg = plan(shim, 10, N, 2, S)
        assert P is None and msg.startswith(f"who: splits {S} outside 0..{-(-N // 64)} ") and f"N = {N}" in msg


def test_no_train_rows_need_no_launch(shim):
    P, _ = plan(shim, 10, 0, 2)
    assert (P["S"], P["tiles"], P["scratch"]) == (0, 0, 0)
    assert plan(shim, 10, 0, 2, 1)[0] is None
