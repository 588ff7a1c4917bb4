"""The slab and the RANSAC chunk schedule (csrc/geom_slab.hpp) on the CPU.  Every geometry entry lays its pieces of the
context's scratch slab out with Slab::take<T>(count), once to measure and once bound to the slab - and every instance its own
memory, through the same rule (OwnedSlab in common.hpp) - and the four RANSAC entries take their sample-loop chunks from
ransac_chunk_bounds.  This test compiles the header (plain C++17, no HIP) behind a small extern "C" shim with the host compiler
and compares it with `carver` below: a Python restatement of the byte-offset rule the entries and the ORB / SIFT / KLT
instances used before they took typed pieces (a `carve(bytes)` per piece, since deleted), NOT a transcription of the header."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT

SHIM = r"""
#include <cstdint>
#include "geom_slab.hpp"
using namespace sslam;
struct E12 { int32_t v[3]; };
struct E40 { double v[5]; };
struct Ctrl { int a, b, c; unsigned long long s; double F[9]; };      // a control block: padded to 96 bytes
extern "C" int ctrl_bytes() { return (int)sizeof(Ctrl); }
// kind[i] indexes {1, 4, 8, 12, 40, sizeof(Ctrl)}.  off[i]: where piece i starts - the returned pointer minus `base`, or (measuring,
// base == 0) the total before the take, which must return null.  Returns the total; ~0 if a pointer is not what the mode promises.
extern "C" unsigned long long slab_shim(unsigned long long base, int n, const unsigned long long* count, const int* kind,
                                        unsigned long long* off) {
    Slab sl;
    sl.base = reinterpret_cast<char*>((uintptr_t)base);
    for (int i = 0; i < n; ++i) {
        const size_t before = sl.bytes, c = (size_t)count[i];
        char* p = nullptr;
        switch (kind[i]) {
            case 0: p = reinterpret_cast<char*>(sl.take<unsigned char>(c)); break;
            case 1: p = reinterpret_cast<char*>(sl.take<float>(c)); break;
            case 2: p = reinterpret_cast<char*>(sl.take<double>(c)); break;
            case 3: p = reinterpret_cast<char*>(sl.take<E12>(c)); break;
            case 4: p = reinterpret_cast<char*>(sl.take<E40>(c)); break;
            default: p = reinterpret_cast<char*>(sl.take<Ctrl>(c)); break;
        }
        if ((p == nullptr) != (base == 0)) return ~0ull;
        off[i] = base ? (unsigned long long)(p - sl.base) : (unsigned long long)before;
    }
    return (unsigned long long)sl.bytes;
}
extern "C" void bounds_shim(int max_iters, int mid, int* o) {
    const auto b = ransac_chunk_bounds(max_iters, mid);
    for (int i = 0; i < 4; ++i) o[i] = b[i];
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the slab header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("geom_slab")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "geom_slab_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    u64p = ctypes.POINTER(ctypes.c_ulonglong)
    lib.slab_shim.argtypes = [ctypes.c_ulonglong, ctypes.c_int, u64p, ctypes.POINTER(ctypes.c_int), u64p]
    lib.slab_shim.restype = ctypes.c_ulonglong
    lib.bounds_shim.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.bounds_shim.restype = None
    return lib


def carver(nbytes):
    """The parent's rule: a piece starts at the total so far; the total then is align_up(total + n + 8, 256)."""
    offs, total = [], 0
    for n in nbytes:
        offs.append(total)
        total = (total + n + 8 + 255) // 256 * 256
    return offs, total


def take_all(lib, base, counts, kinds):
    n = len(counts)
    c = (ctypes.c_ulonglong * n)(*counts)
    k = (ctypes.c_int * n)(*kinds)
    off = (ctypes.c_ulonglong * n)()
    total = lib.slab_shim(base, n, c, k, off)
    assert total != 2 ** 64 - 1, "a take returned a pointer while measuring, or null while bound"
    return list(off), total


def test_placement_is_the_parents_byte_rule(shim):
    sizes = (1, 4, 8, 12, 40, shim.ctrl_bytes())
    assert sizes[5] == 96
    rng = np.random.default_rng(20)
    arena = ctypes.create_string_buffer(4 << 20)
    base = (ctypes.addressof(arena) + 255) // 256 * 256
    for seq in range(3000):
        n = int(rng.integers(1, 14))
        kinds = [int(k) for k in rng.integers(0, 6, n)]
        # mostly small, a fifth empty, now and then a piece that ends just below / on / above a 256-byte boundary
        counts = [0 if rng.random() < 0.2 else int(rng.integers(1, 700)) for _ in range(n)]
        for i in range(n):
            if rng.random() < 0.15:
                counts[i] = (256 * int(rng.integers(1, 8)) - 8 + int(rng.integers(-2, 3))) // sizes[kinds[i]]
        nbytes = [c * sizes[k] for c, k in zip(counts, kinds)]
        want_offs, want_total = carver(nbytes)
        assert want_total <= (4 << 20) - 256
        m_offs, m_total = take_all(shim, 0, counts, kinds)
        b_offs, b_total = take_all(shim, base, counts, kinds)
        assert m_offs == want_offs and b_offs == want_offs, (seq, counts, kinds)
        assert m_total == b_total == want_total, (seq, counts, kinds)
        assert all(o % 256 == 0 for o in b_offs)
        assert all(b_offs[i + 1] - (b_offs[i] + nbytes[i]) >= 8 for i in range(n - 1))
        assert b_total - (b_offs[-1] + nbytes[-1]) >= 8


def test_a_piece_above_4_gib_is_measured_in_size_t(shim):
    # BA's dense Schur operands: [Po][Q][18] doubles reach 32 GB
    sizes = (1, 4, 8, 12, 40, 96)
    for big_kind, big_count in ((2, 600_000_000), (4, 2 ** 30), (1, 2 ** 31 + 5), (0, 2 ** 32 + 1)):
        counts, kinds = [7, big_count, 0, 300, big_count // 3], [1, big_kind, 5, 3, big_kind]
        nbytes = [c * sizes[k] for c, k in zip(counts, kinds)]
        assert nbytes[1] > 2 ** 32
        offs, total = take_all(shim, 0, counts, kinds)
        assert (offs, total) == carver(nbytes)
        assert all(o % 256 == 0 for o in offs)


def test_chunk_bounds(shim):
    o = (ctypes.c_int * 4)()
    for mid in (64, 128):
        for mi in list(range(1, 2001)) + [100000]:
            shim.bounds_shim(mi, mid, o)
            got = list(o)
            assert got == [0, min(8, mi), min(mid, mi), mi], (mi, mid)
            assert all(got[i] <= got[i + 1] for i in range(3))
