"""Which images of one LightGlue enqueue are the same frame (csrc/lg_plan.hpp `lg_alias`), on the CPU.  The header is plain
C++17 with no HIP include; it is compiled behind a small extern "C" shim with the host compiler, as tests/test_lg_plan.py does.
The rule: image j is an alias of the EARLIEST image i < j with equal keypoint, descriptor and count pointers, equal bound and
equal image size; rep[j] == j means "computed".  The expected tables below are written by hand from that rule."""
import ctypes
import shutil
import subprocess

import pytest

from conftest import PKG_NAME, ROOT

SHIM = r"""
#include <cstdint>
#include "lg_plan.hpp"
extern "C" int lg_alias_shim(int NI, const uintptr_t* xy, const uintptr_t* desc, const uintptr_t* cnt, const int* bound,
                             const float* size_w, const float* size_h, int* rep) {
    return sslam::lg_alias(NI, xy, desc, cnt, bound, size_w, size_h, rep);
}
extern "C" int lg_share_shim(int precision, int share_frames) {
    sslam::LGHooks h;
    const bool dflt = h.share_frames;
    h.precision = precision; h.share_frames = share_frames != 0;
    return (dflt ? 2 : 0) | (sslam::lg_plan(h, 2048, 16, true).share_frames ? 1 : 0);
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    d = tmp_path_factory.mktemp("lg_alias")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "lg_alias_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(ROOT / PKG_NAME / "csrc"),
                    str(d / "shim.cpp"), "-o", str(so)], check=True, capture_output=True, text=True)
    return ctypes.CDLL(str(so))


class Frame:
    """The source entries of one image.  Distinct frames get distinct pointers."""

    def __init__(self, k, bound=2048, cnt=True, size=(0.0, 0.0)):
        self.xy, self.desc = 0x10000 * (k + 1), 0x10000 * (k + 1) + 0x4000
        self.cnt = 0x10000 * (k + 1) + 0x8000 if cnt else 0
        self.bound, self.size = bound, size

    def but(self, **kw):
        f = Frame(0)
        f.__dict__.update(self.__dict__)
        f.__dict__.update(kw)
        return f


def alias(shim, images):
    n = len(images)
    up, ip, fp = ctypes.c_size_t * n, ctypes.c_int * n, ctypes.c_float * n
    rep = ip(*([-7] * n))
    distinct = shim.lg_alias_shim(n, up(*[f.xy for f in images]), up(*[f.desc for f in images]), up(*[f.cnt for f in images]),
                                  ip(*[f.bound for f in images]), fp(*[f.size[0] for f in images]),
                                  fp(*[f.size[1] for f in images]), rep)
    return list(rep), distinct


def chain(frames):
    """The frame pipeline's batch: pairs (f0, f1), (f1, f2), ... as the image list 2p, 2p + 1."""
    return [f for a, b in zip(frames[:-1], frames[1:]) for f in (a, b)]


def test_a_chain_of_eight_pairs_holds_nine_distinct_frames(shim):
    rep, distinct = alias(shim, chain([Frame(k) for k in range(9)]))
    # images: f0 f1 | f1 f2 | f2 f3 | ... | f7 f8 ; image 2p (p >= 1) is frame p, first seen as image 2p - 1
    assert rep == [0, 1, 1, 3, 3, 5, 5, 7, 7, 9, 9, 11, 11, 13, 13, 15]
    assert distinct == 9


def test_no_sharing(shim):
    rep, distinct = alias(shim, [Frame(k) for k in range(6)])
    assert rep == [0, 1, 2, 3, 4, 5] and distinct == 6


def test_one_frame_in_three_pairs_and_the_alias_of_an_alias_resolves_to_the_earliest(shim):
    a, b, c, d = (Frame(k) for k in range(4))
    rep, distinct = alias(shim, [a, b, b, c, b, d])                # (A,B), (B,C), (B,D): B is images 1, 2 and 4
    assert rep == [0, 1, 1, 3, 1, 5] and distinct == 4            # image 4 names image 1, not its fellow alias 2
    rep, distinct = alias(shim, [b, a, c, b, d, b, b, b])          # the keyframe on either side
    assert rep == [0, 1, 2, 0, 4, 0, 0, 0] and distinct == 4


def test_a_pair_of_one_frame_with_itself(shim):
    a = Frame(0)
    assert alias(shim, [a, a]) == ([0, 0], 1)
    assert alias(shim, [a, a, a, a]) == ([0, 0, 0, 0], 1)


@pytest.mark.parametrize("change", [dict(bound=2047), dict(cnt=0), dict(cnt=0x77000), dict(size=(1241.0, 376.0)),
                                    dict(size=(0.0, 376.0)), dict(xy=0x990000), dict(desc=0x990000)])
def test_equal_pointers_with_another_bound_count_or_size_are_not_an_alias(shim, change):
    a, b = Frame(0), Frame(1)
    rep, distinct = alias(shim, [a, b, a.but(**change), b])
    assert rep == [0, 1, 2, 1] and distinct == 3
    # ... and two images that share the changed entry are aliases of each other again
    rep, distinct = alias(shim, [a, a.but(**change), a, a.but(**change)])
    assert rep == [0, 1, 0, 1] and distinct == 2


def test_the_plan_shares_on_the_split_paths_only_and_by_default(shim):
    """LGHooks::share_frames defaults to on; the plan takes the shared form in precision 1 and 2, never on the fp32 path."""
    assert [shim.lg_share_shim(p, 1) for p in (0, 1, 2)] == [2, 3, 3]
    assert [shim.lg_share_shim(p, 0) for p in (0, 1, 2)] == [2, 2, 2]
