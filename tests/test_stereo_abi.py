"""The stereo surface without a GPU: the C-ABI header declares the seven entries, the binding and the library export them, the
module offers cv2's constructor and the prototype's four names, arguments outside the backend's scope are refused before the
library is touched, and the module imports nothing of cv2, tests or oracle."""
import inspect
import re

import numpy as np
import pytest

import stereo_ref as R
from conftest import PKG_NAME, ROOT, load_pkg

ENTRIES = ("sslam_sgbm_create", "sslam_sgbm_destroy", "sslam_sgbm_compute_host", "sslam_sgbm_compute_dev", "sslam_sgbm_stage_read",
           "sslam_stereo_lift_host", "sslam_stereo_lift_dev")


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sslam_hip.h").read_text(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_stereo_entry(name):
    assert re.search(rf"\bint\s+{name}\s*\(", _header()), name


@pytest.mark.parametrize("name", ENTRIES)
def test_library_and_binding_export_stereo_entry(name):
    native = load_pkg("_native")
    assert name in native.declared_symbols()
    assert hasattr(native.lib(), name)


def test_create_takes_cv2s_positional_order_and_defaults():
    S = load_pkg("stereo")
    p = inspect.signature(S.StereoSGBM_create).parameters
    assert list(p)[:11] == ["minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio",
                            "speckleWindowSize", "speckleRange", "mode"]
    assert [p[k].default for k in list(p)[:11]] == [0, 16, 3, 0, 0, 0, 0, 0, 0, 0, 0]
    assert (S.MODE_SGBM, S.MODE_HH, S.MODE_SGBM_3WAY, S.MODE_HH4) == (0, 1, 2, 3)
    assert S.STAGES == R.STAGES and (S.MAX_SIDE, S.MAX_COST, S.MAX_WORKSPACE) == (R.MAX_SIDE, R.MAX_COST, R.MAX_WORKSPACE)
    assert list(inspect.signature(S.compute_stereo_disparity).parameters) == ["img_l", "img_r", "stereo"]
    assert list(inspect.signature(S.apply_disparity_check).parameters) == ["q", "disp", "min_disp", "max_disp"]
    q = inspect.signature(S.calculate_right_features).parameters
    assert list(q)[:6] == ["q1", "q2", "disparity1", "disparity2", "min_disp", "max_disp"] and (q["min_disp"].default, q["max_disp"].default) == (0.0, 100.0)
    assert list(inspect.signature(S.get_stereo_3d_pts).parameters)[:6] == ["q1_l", "q1_r", "q2_l", "q2_r", "Proj", "Proj_r"]
    for name in ("compute", "compute_dev", "stage_read"):
        assert callable(getattr(S.StereoSGBM, name))
    for args in ((0, 32, 11, 968, 3872, 0, 0, 0), (5, 32, 3, 10, 4, -1, 20, -3), (0, 16, 3, 0, 0, 3, 63, 15)):
        p, n = R.Params(*args), S.normalise(*args)
        assert n == dict(minD=p.minD, D=p.D, bs=p.bs, P1=p.P1, P2=p.P2, d12=p.d12, uniq=p.uniq, ftzero=p.ftzero, maxD=p.maxD, invalid=p.invalid)
    for w, h, maxD, D in ((1241, 376, 32, 32), (20, 5, 32, 32), (300, 12, 256, 256)):
        assert S.workspace_bytes(w, h, maxD, D) == R.workspace_bytes(w, h, maxD, D)


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


def test_bad_parameters_raise_without_the_library(no_library):
    S = load_pkg("stereo")
    for kw, exc in ((dict(mode=S.MODE_HH), NotImplementedError), (dict(mode=S.MODE_SGBM_3WAY), NotImplementedError), (dict(mode=S.MODE_HH4), NotImplementedError),
                    (dict(speckleWindowSize=100, speckleRange=2), NotImplementedError), (dict(minDisparity=-1), ValueError),
                    (dict(numDisparities=24), ValueError), (dict(numDisparities=272), ValueError), (dict(blockSize=4), ValueError),
                    (dict(blockSize=13), ValueError), (dict(preFilterCap=64), ValueError), (dict(uniquenessRatio=101), ValueError),
                    (dict(blockSize=11, preFilterCap=63, P2=30000), ValueError)):
        a = dict(dict(minDisparity=0, numDisparities=32, blockSize=5), **kw)
        with pytest.raises(exc) as e:
            S.StereoSGBM_create(**a)
        p = dict(dict(P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=0), **a)
        ref = R.check_create(100, 60, **p)
        assert ref is not None and (ref in str(e.value) or ref.split(" is not built")[0] in str(e.value)), (kw, str(e.value), ref)
    S.StereoSGBM_create(0, 32, 11, 8 * 121, 32 * 121)               # the prototype's call: accepted, no device yet


def test_bad_images_raise_without_the_library(no_library):
    S = load_pkg("stereo")
    sg = S.StereoSGBM_create(0, 32, 11, 968, 3872)
    g = np.zeros((6, 50), np.uint8)
    with pytest.raises(ValueError, match="compute_stereo_disparity"):
        sg.compute(np.zeros((6, 50, 3), np.uint8), np.zeros((6, 50, 3), np.uint8))
    with pytest.raises(TypeError):
        sg.compute(g.astype(np.float32), g.astype(np.float32))
    with pytest.raises(TypeError):
        sg.compute(g.astype(np.uint16), g.astype(np.uint16))
    with pytest.raises(ValueError, match="differ in size"):
        sg.compute(g, np.zeros((6, 51), np.uint8))
    with pytest.raises(ValueError):
        sg.compute(np.zeros(50, np.uint8), np.zeros(50, np.uint8))
    with pytest.raises(ValueError, match="image size 0x6"):
        sg.compute(np.zeros((6, 0), np.uint8), np.zeros((6, 0), np.uint8))
    with pytest.raises(ValueError, match="2 channels|unsupported image shape"):
        S.compute_stereo_disparity(np.zeros((6, 50, 2), np.uint8), np.zeros((6, 50, 2), np.uint8), sg)
    with pytest.raises(ValueError, match="no compute yet"):
        sg.stage_read("S")
    big = S.StereoSGBM_create(0, 256, 3)
    with pytest.raises(ValueError, match=f"workspace of {R.workspace_bytes(4096, 2048, 256, 256)} bytes"):
        S._check_size(4096, 2048, big.params)


def test_contiguous_copies_of_views_live_across_the_library_call(monkeypatch):
    """a sliced view is copied for the library; the copy must be referenced until the call returns (the binding's pointer keeps
    nothing alive)"""
    import ctypes as C
    import weakref
    S, native = load_pkg("stereo"), load_pkg("_native")
    seen = {}
    real = np.ascontiguousarray

    def tracking(a, *args, **kw):
        out = real(a, *args, **kw)
        if out is not a:
            seen.setdefault("refs", []).append(weakref.ref(out))
        return out

    class FakeLib:
        def sslam_sgbm_compute_host(self, handle, left, right, H, W, channels, out):
            seen["alive"] = [r() is not None for r in seen["refs"]]
            seen["rows"] = [C.string_at(p.value, W) for p in (left, right)]
            return 0
    monkeypatch.setattr(np, "ascontiguousarray", tracking)
    monkeypatch.setattr(native, "lib", lambda: FakeLib())
    inst = S._Instance.__new__(S._Instance)
    inst.handle, inst.max_wh, inst._last = C.c_void_p(1), (64, 8), None
    canvas = np.arange(8 * 80, dtype=np.uint8).reshape(8, 80)
    left, right = canvas[:, 3:53], canvas[:, 7:57]
    inst.compute(left, right)
    assert seen["alive"] == [True, True]
    assert seen["rows"] == [left[0].tobytes(), right[0].tobytes()]
    inst.handle = None                                                   # (nothing to destroy)


def test_apply_disparity_check_is_the_prototypes_expression(no_library):
    S = load_pkg("stereo")
    rng = np.random.default_rng(0)
    disp = rng.uniform(-1, 40, (9, 14)).astype(np.float32)
    q = np.column_stack([rng.uniform(0, 14, 30), rng.uniform(0, 9, 30)]).astype(np.float32)
    vals, mask = S.apply_disparity_check(q, disp, 0.0, 30.0)
    want = disp[q[:, 1].astype(int), q[:, 0].astype(int)]
    assert np.array_equal(vals, want) and np.array_equal(mask, (want > 0.0) & (want < 30.0))


def test_product_imports_no_cv2_and_nothing_under_tests():
    src = (ROOT / PKG_NAME / "stereo.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(cv2|tests|oracle|stereo_ref|stereo_scenes)\b", src, flags=re.M)
