"""Pyramidal Lucas-Kanade surface without a GPU: the C-ABI header declares the entries, the binding and the library export
them, the library refuses bad arguments with a code and a message before it touches the device, and the Python module
refuses them (and answers N == 0) without touching the library."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

ENTRIES = ("sslam_klt_create", "sslam_klt_destroy", "sslam_klt_push_host", "sslam_klt_push_dev", "sslam_klt_gray_host",
           "sslam_klt_track_host", "sslam_klt_track_dev", "sslam_klt_track_fb_host", "sslam_klt_track_fb_dev", "sslam_klt_info",
           "sslam_klt_levels_read")


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sslam_hip.h").read_text(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_header_binding_and_library_carry_the_entry(name):
    assert re.search(rf"\bint\s+{name}\s*\(", _header()), name
    native = load_pkg("_native")
    assert name in native.declared_symbols()
    assert hasattr(native.lib(), name)


def test_abi_version_is_unchanged():
    assert load_pkg("_native").lib().sslam_abi_version() == 1


def _refused(rc, *words):
    msg = load_pkg("_native").lib().sslam_last_error().decode()
    assert rc != 0, "accepted"
    for w in words:
        assert w in msg, msg
    return msg


def test_create_refuses_bad_arguments_before_touching_the_device():
    """No device is needed (or present): every refusal comes before the first HIP call.  `ctx` is a block of zeros that a
    refusing call never reads."""
    lib = load_pkg("_native").lib()
    fake_ctx = C.create_string_buffer(256)
    ctx = C.cast(fake_ctx, C.c_void_p)
    out = C.c_void_p()
    ok = dict(max_w=64, max_h=48, max_points=100, win_w=21, win_h=21, max_level=3)

    def create(ctx_=ctx, out_=C.byref(out), **kw):
        a = {**ok, **kw}
        return lib.sslam_klt_create(ctx_, a["max_w"], a["max_h"], a["max_points"], a["win_w"], a["win_h"], a["max_level"], out_)
    _refused(create(ctx_=None), "NULL")
    _refused(create(out_=None), "NULL")
    for kw in (dict(max_w=0), dict(max_h=0), dict(max_w=16385), dict(max_h=16385), dict(max_w=-3)):
        _refused(create(**kw), "outside 1..16384")
    for kw in (dict(win_w=20), dict(win_h=8), dict(win_w=0)):
        _refused(create(**kw), "even side")
    for kw in (dict(win_w=1), dict(win_h=33), dict(win_w=-5), dict(win_w=63)):
        _refused(create(**kw), "outside 3..31")
    for kw in (dict(max_points=0), dict(max_points=(1 << 20) + 1)):
        _refused(create(**kw), "points")
    for kw in (dict(max_level=-1), dict(max_level=11)):
        _refused(create(**kw), "maxLevel")
    assert out.value is None


def test_entries_refuse_a_null_instance():
    lib = load_pkg("_native").lib()
    buf = np.zeros(64, np.uint8)
    p = load_pkg("_native").ptr(buf)
    _refused(lib.sslam_klt_push_host(None, p, 4, 4, 1), "NULL")
    _refused(lib.sslam_klt_push_dev(None, p, 4, 4, 1), "NULL")
    _refused(lib.sslam_klt_track_host(None, 0, 1, p, None, 0, 3, 30, 0.01, 1e-4, p, p, p), "NULL")
    _refused(lib.sslam_klt_track_dev(None, 0, 1, p, None, 0, 3, 30, 0.01, 1e-4, p, p, p), "NULL")
    _refused(lib.sslam_klt_track_fb_host(None, 1, p, 3, 30, 0.01, 1e-4, 12.0, 1.5, None, p, p, p, None), "NULL")
    _refused(lib.sslam_klt_track_fb_dev(None, 1, p, 3, 30, 0.01, 1e-4, 12.0, 1.5, None, p, p, p, None), "NULL")
    _refused(lib.sslam_klt_levels_read(None, 0, 0, p, None, None), "NULL")
    _refused(lib.sslam_klt_info(None, 0, None, None, None), "NULL")
    _refused(lib.sslam_klt_gray_host(None, p, 4, 4, 3, p), "NULL")
    assert lib.sslam_klt_destroy(None) == 0


def test_gray_host_refuses_sizes_and_channels_before_touching_the_device():
    lib = load_pkg("_native").lib()
    fake_ctx = C.create_string_buffer(256)
    ctx = C.cast(fake_ctx, C.c_void_p)
    p = load_pkg("_native").ptr(np.zeros(64, np.uint8))
    _refused(lib.sslam_klt_gray_host(ctx, p, 4, 4, 2, p), "channels")
    _refused(lib.sslam_klt_gray_host(ctx, p, 0, 4, 3, p), "outside 1..16384")
    _refused(lib.sslam_klt_gray_host(ctx, p, 4, 16385, 3, p), "outside 1..16384")
    _refused(lib.sslam_klt_gray_host(ctx, None, 4, 4, 3, p), "NULL")


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal, and the answer to N == 0, must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


def test_module_names_and_defaults():
    import inspect
    O = load_pkg("optical_flow")
    sig = inspect.signature(O.calc_optical_flow_pyr_lk)
    assert list(sig.parameters) == ["prev_img", "next_img", "prev_pts", "next_pts", "winSize", "maxLevel", "criteria", "flags",
                                    "minEigThreshold", "ctx"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["winSize"], d["maxLevel"], d["criteria"], d["flags"], d["minEigThreshold"]) == ((21, 21), 3, (3, 30, 0.01), 0, 1e-4)
    sig = inspect.signature(O.KLTTracker.__init__)
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["winSize"], d["maxLevel"], d["criteria"], d["minEigThreshold"], d["err_thresh"], d["fb_thresh"]) == \
        ((21, 21), 3, (3, 30, 1e-3), 1e-4, 12.0, 1.5)                    # main4.py:242-252
    for name in ("push", "track", "close"):
        assert callable(getattr(O.KLTTracker, name))
    assert callable(O.bgr_to_gray)
    assert (O.OPTFLOW_USE_INITIAL_FLOW, O.OPTFLOW_LK_GET_MIN_EIGENVALS) == (4, 8)


def test_no_points_are_answered_without_the_library(no_library):
    O = load_pkg("optical_flow")
    img = np.zeros((48, 64), np.uint8)
    for pts in (np.empty((0, 2), np.float32), np.empty((0, 1, 2), np.float32), []):
        nxt, st, err = O.calc_optical_flow_pyr_lk(img, img, pts)
        assert nxt.shape == (0, 1, 2) and nxt.dtype == np.float32
        assert st.shape == (0, 1) and st.dtype == np.uint8
        assert err.shape == (0, 1) and err.dtype == np.float32


def test_python_refuses_bad_arguments_without_the_library(no_library):
    O = load_pkg("optical_flow")
    img = np.zeros((48, 64), np.uint8)
    pts = np.ones((3, 2), np.float32)
    with pytest.raises(TypeError):
        O.calc_optical_flow_pyr_lk(img.astype(np.uint16), img, pts)        # 16-bit images are out of scope
    with pytest.raises(TypeError):
        O.calc_optical_flow_pyr_lk(img, img.astype(np.float32), pts)
    with pytest.raises(ValueError, match="channels"):
        O.calc_optical_flow_pyr_lk(np.zeros((48, 64, 2), np.uint8), img, pts)
    with pytest.raises(ValueError, match="differ in size"):
        O.calc_optical_flow_pyr_lk(img, np.zeros((48, 65), np.uint8), pts)
    with pytest.raises(ValueError, match="outside 1..16384"):
        O.calc_optical_flow_pyr_lk(np.zeros((1, 16385), np.uint8), np.zeros((1, 16385), np.uint8), pts)
    for win in ((20, 21), (21, 4)):
        with pytest.raises(ValueError, match="even side"):
            O.calc_optical_flow_pyr_lk(img, img, pts, winSize=win)
    for win in ((1, 21), (21, 33), (63, 63)):
        with pytest.raises(ValueError, match="outside 3..31"):
            O.calc_optical_flow_pyr_lk(img, img, pts, winSize=win)
    for lv in (-1, 11):
        with pytest.raises(ValueError, match="maxLevel"):
            O.calc_optical_flow_pyr_lk(img, img, pts, maxLevel=lv)
    with pytest.raises(ValueError, match=r"\[N,2\]"):
        O.calc_optical_flow_pyr_lk(img, img, np.ones((3, 3), np.float32))
    with pytest.raises(ValueError, match="flags"):
        O.calc_optical_flow_pyr_lk(img, img, pts, flags=1)
    with pytest.raises(ValueError, match="next_pts"):
        O.calc_optical_flow_pyr_lk(img, img, pts, flags=O.OPTFLOW_USE_INITIAL_FLOW)
    with pytest.raises(ValueError, match="next_pts"):
        O.calc_optical_flow_pyr_lk(img, img, pts, np.ones((2, 2), np.float32), flags=O.OPTFLOW_USE_INITIAL_FLOW)
    with pytest.raises(ValueError, match="not finite"):
        O.calc_optical_flow_pyr_lk(img, img, pts, criteria=(3, 30, float("nan")))
    with pytest.raises(ValueError):
        O.KLTTracker((0, 48))
    with pytest.raises(ValueError, match="even side"):
        O.KLTTracker((64, 48), winSize=(10, 10))
    with pytest.raises(ValueError, match="capacity"):
        O.KLTTracker((64, 48), max_points=0)
    assert O.bgr_to_gray(img) is img                                      # 2-D passes through, no library


def test_tracker_refuses_more_points_than_its_capacity_and_tracking_too_early(no_library):
    O = load_pkg("optical_flow")
    t = O.KLTTracker.__new__(O.KLTTracker)                                # an instance is not needed to refuse
    t.handle, t.max_points, t.pushes, t.size, t.ctx = C.c_void_p(1), 10, 2, (64, 48), object()
    t.criteria, t.min_eig, t.err_thresh, t.fb_thresh = (3, 30, 1e-3), 1e-4, 12.0, 1.5
    with pytest.raises(ValueError, match="capacity"):
        t.track(np.ones((11, 2), np.float32))
    t.pushes = 1
    with pytest.raises(RuntimeError, match="two pushed frames"):
        t.track(np.ones((5, 2), np.float32))
    with pytest.raises(ValueError, match="tracker's"):
        t.push(np.zeros((48, 65), np.uint8))
    t.handle = None                                                       # (nothing for __del__ to destroy)


def test_product_imports_no_cv2_and_nothing_under_tests():
    src = (ROOT / "opencv-simpleslam_amd" / "optical_flow.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(cv2|tests|oracle|klt_ref|klt_scenes)\b", src, flags=re.M)
