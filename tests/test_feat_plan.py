"""The host side the feature detectors share (csrc/feat_plan.hpp) on the CPU: the header (plain C++17, no HIP) is compiled behind a
small extern "C" shim with the host compiler - fastAtan2's constants bit for bit against tests/orb_ref.py, cvRound at the halves,
the tile quotient, every refusal of the per-call image check with its message and code, and that sift_plan.hpp no longer pulls in
the ORB plan."""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest

import orb_ref as R
from conftest import PKG_NAME, ROOT

CSRC = ROOT / PKG_NAME / "csrc"

SHIM = r"""
#include "feat_plan.hpp"
using namespace sslam;
static_assert(feat_cdiv(64, 64) == 1 && feat_cdiv(65, 64) == 2 && feat_cdiv(1, 4) == 1 && feat_cdiv(0, 4) == 0, "the tile quotient");
extern "C" void feat_atan_shim(float* f) {
    const FastAtan k = fast_atan_consts();
    const float v[] = {k.p1, k.p3, k.p5, k.p7, k.eps, k.deg2rad};
    for (int i = 0; i < 6; ++i) f[i] = v[i];
}
extern "C" int feat_round_shim(double v) { return cv_round(v); }
extern "C" int feat_roundf_shim(float v) { return cv_roundf(v); }
extern "C" int feat_max_side_shim() { return FEAT_MAX_SIDE; }
extern "C" int feat_image_shim(int w, int h, int c, int max_w, int max_h, char* msg, int n) { return feat_check_image(w, h, c, max_w, max_h, msg, (size_t)n); }
"""


@pytest.fixture(scope="module")
def gxx():
    exe = shutil.which("g++")
    if exe is None:
        pytest.skip("no g++ on this machine: the plan header is tested where a host compiler exists")
    return exe


@pytest.fixture(scope="module")
def shim(gxx, tmp_path_factory):
    d = tmp_path_factory.mktemp("feat_plan")
    (d / "shim.cpp").write_text(SHIM)
    so = d / "feat_plan_shim.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", str(CSRC), str(d / "shim.cpp"), "-o", str(so)],
                   check=True, capture_output=True, text=True)
    lib = ctypes.CDLL(str(so))
    lib.feat_atan_shim.argtypes = [ctypes.c_void_p]
    lib.feat_round_shim.argtypes = [ctypes.c_double]
    lib.feat_roundf_shim.argtypes = [ctypes.c_float]
    lib.feat_image_shim.argtypes = [ctypes.c_int] * 5 + [ctypes.c_char_p, ctypes.c_int]
    return lib


def test_fast_atan_constants_equal_the_restatement_bit_for_bit(shim):
    f = np.zeros(6, np.float32)
    shim.feat_atan_shim(f.ctypes.data)
    want = np.array([*R.ATAN_P, R.EPS32, R.F32(np.pi / 180.0)], np.float32)
    assert f.tobytes() == want.tobytes(), (f, want)
    assert shim.feat_max_side_shim() == 16384


def test_cv_round_rounds_half_to_even(shim):
    for v, want in ((0.5, 0), (-0.5, 0), (1.5, 2), (-1.5, -2), (2.5, 2), (-2.5, -2), (2.4999, 2), (2.5001, 3), (-7.0, -7)):
        assert shim.feat_round_shim(v) == want, v
        assert shim.feat_roundf_shim(v) == want, v


def test_every_image_refusal_with_its_message(shim):
    msg = ctypes.create_string_buffer(200)

    def image(w, h, c, max_w=640, max_h=480):
        msg.value = b""
        return shim.feat_image_shim(w, h, c, max_w, max_h, msg, 200), msg.value.decode()
    for a in ((640, 480, 1), (1, 1, 3), (5, 5, 4)):
        assert image(*a) == (0, "")
    assert image(640, 480, 2) == (1, "2 channels (want 1, 3 or 4)")
    assert image(640, 480, 0) == (1, "0 channels (want 1, 3 or 4)")
    assert image(640, 480, 5) == (1, "5 channels (want 1, 3 or 4)")
    assert image(0, 480, 1) == (2, "frame size 0x480")
    assert image(640, 0, 3) == (2, "frame size 640x0")
    assert image(-1, -1, 1) == (2, "frame size -1x-1")
    assert image(641, 480, 1) == (3, "frame 641x480 is larger than the instance's 640x480")
    assert image(640, 481, 4) == (3, "frame 640x481 is larger than the instance's 640x480")
    assert image(0, 0, 2)[0] == 1                       # the channel count is checked first, the size before the instance's bound
    assert image(0, 481, 1)[0] == 2


def test_the_sift_plan_no_longer_pulls_in_the_orb_plan(gxx, tmp_path):
    src = tmp_path / "only_sift.cpp"
    src.write_text('#include "sift_plan.hpp"\nint main() { return sslam::sift_consts().atan.p1 > 0 ? 0 : 1; }\n')
    out = subprocess.run([gxx, "-std=c++17", "-E", "-I", str(CSRC), str(src)], check=True, capture_output=True, text=True).stdout
    assert "SiftPlan" in out and "FastAtan" in out
    assert "OrbPlan" not in out and "orb_plan" not in out
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(CSRC), str(src)], check=True, capture_output=True, text=True)
