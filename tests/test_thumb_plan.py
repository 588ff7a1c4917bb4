"""The thumbnail host plan (csrc/thumb_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a small
extern "C" shim with the host compiler and compared with tests/thumb_ref.py - the quantisation tables per quality, the DCT matrix,
the zigzag order, the Huffman codes, the MCU and block geometry, the dummy-block predicate and the block a dummy copies, the resize
taps, the capacity, the header bytes and every refusal with its message."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import thumb_ref as R
from conftest import PKG_NAME, ROOT

SHIM = r"""
#include "thumb_plan.hpp"
#include <cstring>
using namespace sslam;
// dct int32[64]; quant uint16[2][64]; zz uint8[64]; dc uint16[2][12][2] (code, len); ac uint16[2][256][2]
extern "C" void th_tables_shim(int quality, int* dct, unsigned short* quant, unsigned char* zz, unsigned short* dc, unsigned short* ac) {
    const ThumbTables T = thumb_tables(quality);
    std::memcpy(dct, T.dct, sizeof T.dct);
    std::memcpy(quant, T.quant, sizeof T.quant);
    std::memcpy(zz, T.zigzag_pos, sizeof T.zigzag_pos);
    for (int t = 0; t < 2; ++t) {
        for (int i = 0; i < 12; ++i) { dc[(t * 12 + i) * 2] = T.dc_code[t][i]; dc[(t * 12 + i) * 2 + 1] = T.dc_len[t][i]; }
        for (int i = 0; i < 256; ++i) { ac[(t * 256 + i) * 2] = T.ac_code[t][i]; ac[(t * 256 + i) * 2 + 1] = T.ac_len[t][i]; }
    }
}
// g: w h ncomp mcux mcuy yw yh cw ch bw bh blocks
extern "C" void th_geom_shim(int w, int h, int c, int* g) {
    const ThumbGeom G = thumb_geom(w, h, c);
    const int v[] = {G.w, G.h, G.ncomp, G.mcux, G.mcuy, G.yw, G.yh, G.cw, G.ch, G.bw, G.bh, G.blocks};
    for (int i = 0; i < 12; ++i) g[i] = v[i];
}
// per block: comp bx by dummy sx sy prev
extern "C" void th_blocks_shim(int w, int h, int c, int* out) {
    const ThumbGeom G = thumb_geom(w, h, c);
    for (int b = 0; b < G.blocks; ++b) {
        const ThumbBlock k = thumb_block(G, b);
        const int v[] = {k.comp, k.bx, k.by, k.dummy, k.sx, k.sy, k.prev};
        for (int i = 0; i < 7; ++i) out[7 * b + i] = v[i];
    }
}
extern "C" int th_dummy_shim(int w, int h, int bx, int by) { return thumb_is_dummy(thumb_geom(w, h, 3), bx, by) ? 1 : 0; }
extern "C" void th_taps_shim(int dst, int src, int* out) {
    for (int d = 0; d < dst; ++d) thumb_tap(d, dst, src, out + 4 * d, out + 4 * d + 1, out + 4 * d + 2, out + 4 * d + 3);
}
extern "C" long long th_capacity_shim(int w, int h) { return (long long)thumb_capacity(w, h); }
extern "C" long long th_chunks_shim(int blocks) { return (long long)thumb_chunks(blocks); }
extern "C" int th_header_shim(int w, int h, int ncomp, int quality, unsigned char* out, int cap) {
    const std::vector<uint8_t> v = thumb_header(w, h, ncomp, quality);
    if ((int)v.size() > cap) return -1;
    std::memcpy(out, v.data(), v.size());
    return (int)v.size();
}
extern "C" void th_consts_shim(int* c) {
    const int v[] = {THUMB_MAX_DST, THUMB_MAX_SRC, THUMB_BLOCK_BITS, THUMB_BLOCK_WORDS, THUMB_BLOCK_BYTES, THUMB_CHUNK, THUMB_STAGE_RESIZED, THUMB_STAGE_Y,
                     THUMB_STAGE_CB, THUMB_STAGE_CR, THUMB_STAGE_COEF, THUMB_STAGE_BITOFF};
    for (int i = 0; i < 12; ++i) c[i] = v[i];
}
extern "C" int th_create_shim(int mw, int mh, int w, int h, int q, char* msg, int n) { return thumb_check_create(mw, mh, w, h, q, msg, (size_t)n); }
extern "C" int th_image_shim(int ws, int hs, int c, int mw, int mh, char* msg, int n) { return thumb_check_image(ws, hs, c, mw, mh, msg, (size_t)n); }
"""

SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (17, 16), (40, 24), (24, 40), (33, 17), (50, 30), (23, 19), (640, 360), (4096, 4096)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("thumb_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "thumb_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    i, vp = ctypes.c_int, ctypes.c_void_p
    lib.th_tables_shim.argtypes = [i, vp, vp, vp, vp, vp]
    lib.th_geom_shim.argtypes = [i, i, i, vp]
    lib.th_blocks_shim.argtypes = [i, i, i, vp]
    lib.th_dummy_shim.argtypes = [i, i, i, i]
    lib.th_taps_shim.argtypes = [i, i, vp]
    lib.th_capacity_shim.argtypes = [i, i]
    lib.th_capacity_shim.restype = ctypes.c_longlong
    lib.th_chunks_shim.argtypes = [i]
    lib.th_chunks_shim.restype = ctypes.c_longlong
    lib.th_header_shim.argtypes = [i, i, i, i, vp, i]
    lib.th_consts_shim.argtypes = [vp]
    lib.th_create_shim.argtypes = [i] * 5 + [ctypes.c_char_p, i]
    lib.th_image_shim.argtypes = [i] * 5 + [ctypes.c_char_p, i]
    return lib


def _tables(lib, q):
    dct, quant, zz = np.zeros(64, np.int32), np.zeros((2, 64), np.uint16), np.zeros(64, np.uint8)
    dc, ac = np.zeros((2, 12, 2), np.uint16), np.zeros((2, 256, 2), np.uint16)
    lib.th_tables_shim(q, dct.ctypes.data, quant.ctypes.data, zz.ctypes.data, dc.ctypes.data, ac.ctypes.data)
    return dct, quant, zz, dc, ac


def test_tables_per_quality_equal_the_restatement(shim):
    for q in (1, 2, 10, 25, 49, 50, 51, 70, 75, 95, 99, 100):
        dct, quant, zz, dc, ac = _tables(shim, q)
        ql, qc = R.quant_tables(q)
        assert quant[0].tolist() == ql.tolist() and quant[1].tolist() == qc.tolist(), q
        assert quant.min() >= 1 and quant.max() <= 255
    assert _tables(shim, 100)[1].max() == 1 and _tables(shim, 1)[1].min() == 255
    assert _tables(shim, 50)[1][0].tolist() == R.LUMA_Q.tolist()
    assert dct.tolist() == R.dct_matrix().reshape(64).tolist()
    assert dct[:8].tolist() == [2896] * 8 and dct[8:16].tolist() == [4017, 3406, 2276, 799, -799, -2276, -3406, -4017]
    assert zz[R.ZIGZAG].tolist() == list(range(64)) and sorted(R.ZIGZAG.tolist()) == list(range(64))
    for t in range(2):
        for sym in range(12):
            assert tuple(dc[t, sym].tolist()) == R.DC_CODES[t][sym]
        for sym in range(256):
            assert tuple(ac[t, sym].tolist()) == R.AC_CODES[t].get(sym, (0, 0)), (t, sym)
        assert len(R.AC_CODES[t]) == 162 and max(ln for _, ln in R.AC_CODES[t].values()) == 16
        assert max(ln for _, ln in R.DC_CODES[t].values()) <= 11 - 2 * (1 - t)          # 9 bits luma, 11 chroma


def test_geometry_blocks_and_the_dummy_rule_equal_the_restatement(shim):
    names = ("w", "h", "ncomp", "mcux", "mcuy", "yw", "yh", "cw", "ch", "bw", "bh", "blocks")
    for w, h in SIZES:
        for c in (1, 3, 4):
            g = np.zeros(12, np.int32)
            shim.th_geom_shim(w, h, c, g.ctypes.data)
            ref = R.geometry(w, h, c)
            assert dict(zip(names, g.tolist())) == {k: ref[k] for k in names}, (w, h, c)
            if ref["blocks"] > 20000:
                continue
            out = np.zeros((ref["blocks"], 7), np.int32)
            shim.th_blocks_shim(w, h, c, out.ctypes.data)
            want = [[int(v) for v in R.block_info(ref, b)] for b in range(ref["blocks"])]
            assert out.tolist() == want, (w, h, c)
            # every plane position is covered exactly once, and a dummy copies a real Y block of its own MCU
            for comp in range(ref["ncomp"]):
                pos = [(r[1], r[2]) for r in want if r[0] == comp]
                pw = (ref["yw"] if comp == 0 else ref["cw"]) // 8
                ph = (ref["yh"] if comp == 0 else ref["ch"]) // 8
                assert sorted(pos) == sorted((x, y) for y in range(ph) for x in range(pw))
            for r in want:
                if r[3]:
                    assert r[0] == 0 and not R.is_dummy(ref, r[4], r[5]) and (r[4] // 2, r[5] // 2) == (r[1] // 2, r[2] // 2)
    # 640 x 360: the whole 46th block row of the 16-pixel MCU grid is dummy, no column is
    assert [shim.th_dummy_shim(640, 360, bx, 45) for bx in (0, 79)] == [1, 1]
    assert [shim.th_dummy_shim(640, 360, bx, 44) for bx in (0, 79)] == [0, 0]
    assert shim.th_dummy_shim(40, 24, 4, 3) == 1 and shim.th_dummy_shim(24, 40, 3, 4) == 1 and shim.th_dummy_shim(24, 40, 2, 4) == 0
    g = R.geometry(640, 360, 3)
    assert sum(R.block_info(g, b)[3] for b in range(g["blocks"])) == 80 and g["blocks"] == 40 * 23 * 6


def test_resize_taps_equal_the_restatement(shim):
    for dst, src in ((1, 1), (8, 8), (9, 9), (50, 100), (30, 60), (640, 1241), (360, 376), (23, 5), (19, 4), (7, 1), (1, 7), (4096, 16384), (100, 3)):
        out = np.zeros((dst, 4), np.int32)
        shim.th_taps_shim(dst, src, out.ctypes.data)
        s0, s1, a0, a1 = R.resize_coords(dst, src)
        assert out[:, 0].tolist() == s0.tolist() and out[:, 1].tolist() == s1.tolist(), (dst, src)
        assert out[:, 2].tolist() == a0.tolist() and out[:, 3].tolist() == a1.tolist(), (dst, src)
        assert out[:, :2].min() >= 0 and out[:, :2].max() <= src - 1                    # every tap inside the source


def test_constants_capacity_and_chunks(shim):
    c = np.zeros(12, np.int32)
    shim.th_consts_shim(c.ctypes.data)
    assert c.tolist() == [R.MAX_DST, R.MAX_SRC, 20 + 63 * 26, 52, R.BLOCK_BYTES, 16] + [R.STAGES[k] for k in ("resized", "y", "cb", "cr", "coef", "bitoff")]
    assert 52 * 32 >= 20 + 63 * 26 and R.BLOCK_BYTES == 2 * 52 * 4
    for w, h in SIZES:
        assert shim.th_capacity_shim(w, h) == R.capacity(w, h)
    assert shim.th_capacity_shim(640, 360) == 623 + 416 * 5520 + 2
    for blocks in (1, 6, 7, 5520):
        assert shim.th_chunks_shim(blocks) == 13 * blocks


def test_header_bytes_equal_the_restatement(shim):
    buf = np.zeros(1024, np.uint8)
    for w, h, ncomp, q in ((640, 360, 3, 70), (640, 360, 1, 70), (1, 1, 3, 1), (4096, 4096, 3, 100), (33, 17, 1, 95), (300, 258, 3, 50)):
        n = shim.th_header_shim(w, h, ncomp, q, buf.ctypes.data, len(buf))
        assert bytes(buf[:n]) == R.header(w, h, ncomp, q), (w, h, ncomp, q)
    assert shim.th_header_shim(640, 360, 3, 70, buf.ctypes.data, len(buf)) == 623


REFUSALS = [
    (dict(q=0), "quality 0 outside 1..100"),
    (dict(q=101), "quality 101 outside 1..100"),
    (dict(q=-5), "quality -5 outside 1..100"),
    (dict(w=0), "thumbnail size 0x30 outside 1..4096"),
    (dict(w=4097), "thumbnail size 4097x30 outside 1..4096"),
    (dict(h=0), "thumbnail size 50x0 outside 1..4096"),
    (dict(h=4097), "thumbnail size 50x4097 outside 1..4096"),
    (dict(mw=0), "source size 0x60 outside 1..16384"),
    (dict(mw=16385), "source size 16385x60 outside 1..16384"),
    (dict(mh=0), "source size 100x0 outside 1..16384"),
    (dict(mh=16385), "source size 100x16385 outside 1..16384"),
]


def test_every_refusal_with_its_message(shim):
    base = dict(mw=100, mh=60, w=50, h=30, q=70)
    msg = ctypes.create_string_buffer(200)

    def create(**kw):
        a = dict(base, **kw)
        msg.value = b""
        rc = shim.th_create_shim(a["mw"], a["mh"], a["w"], a["h"], a["q"], msg, 200)
        return rc, msg.value.decode()
    assert create() == (0, "")
    assert create(q=1)[0] == 0 and create(q=100)[0] == 0 and create(w=4096, h=4096, mw=16384, mh=16384)[0] == 0 and create(w=1, h=1, mw=1, mh=1)[0] == 0
    for kw, text in REFUSALS:
        rc, got = create(**kw)
        a = dict(base, **kw)
        assert rc != 0 and got == text == R.check_create(a["mw"], a["mh"], a["w"], a["h"], a["q"]), (kw, got)
    for (ws, hs, c), text in (((10, 10, 2), "2 channels (want 1, 3 or 4)"), ((10, 10, 0), "0 channels (want 1, 3 or 4)"),
                              ((0, 10, 1), "source size 0x10 outside 1..16384"), ((10, 16385, 3), "source size 10x16385 outside 1..16384"),
                              ((101, 60, 1), "source 101x60 is larger than the instance's 100x60"),
                              ((100, 61, 3), "source 100x61 is larger than the instance's 100x60")):
        msg.value = b""
        assert shim.th_image_shim(ws, hs, c, 100, 60, msg, 200) != 0 and msg.value.decode() == text == R.check_image(ws, hs, c, 100, 60)
    for c in (1, 3, 4):
        assert shim.th_image_shim(100, 60, c, 100, 60, msg, 200) == 0 and R.check_image(100, 60, c, 100, 60) is None
