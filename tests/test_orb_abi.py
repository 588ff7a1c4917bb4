"""The ORB surface without a GPU: the C-ABI header declares the entries, the binding and the library export them, the library
refuses bad arguments with a code and a message before it touches the device, `orb.py` refuses them without touching the
library, and `init_feature_pipeline` hands out the GPU ORB + brute-force pair on the cv2-less default branch (with the fake
device of tests/fake_device.py standing in for the context) and keeps raising for SIFT / AKAZE / FLANN."""
import ctypes as C
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest

import fake_device
from conftest import ROOT, load_pkg

ENTRIES = ("sslam_orb_create", "sslam_orb_destroy", "sslam_orb_capacity", "sslam_orb_default_pattern", "sslam_orb_detect_host",
           "sslam_orb_detect_dev", "sslam_orb_level_info", "sslam_orb_stage_read")


def _header():
    return (ROOT / "include" / "sslam_hip.h").read_text()


@pytest.mark.parametrize("name", ENTRIES)
def test_header_binding_and_library_carry_the_entry(name):
    assert re.search(rf"\bint\s+{name}\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)), name
    native = load_pkg("_native")
    assert name in native.declared_symbols()
    assert hasattr(native.lib(), name)


def _refused(rc, *words):
    msg = load_pkg("_native").lib().sslam_last_error().decode()
    assert rc != 0, "accepted"
    for w in words:
        assert w in msg, msg


def test_entries_refuse_bad_arguments_before_touching_the_device():
    """No device is needed (or present): every refusal comes before the first HIP call.  `ctx` is a block of zeros that a
    refusing call never reads."""
    native = load_pkg("_native")
    lib = native.lib()
    ctx = C.cast(C.create_string_buffer(256), C.c_void_p)
    h = C.c_void_p()

    def create(**kw):
        a = dict(ctx=ctx, max_w=640, max_h=480, nfeatures=500, sf=1.2, nlevels=8, edge=31, score=0, fast=20, pattern=None, out=C.byref(h))
        a.update(kw)
        return lib.sslam_orb_create(a["ctx"], a["max_w"], a["max_h"], a["nfeatures"], a["sf"], a["nlevels"], a["edge"], a["score"], a["fast"],
                                    native.ptr(a["pattern"]), a["out"])
    who = "sslam_orb_create"
    _refused(create(ctx=None), who, "NULL")
    _refused(create(out=None), who, "NULL")
    _refused(create(nfeatures=0), who, "nfeatures 0")
    _refused(create(sf=1.0), who, "scaleFactor")
    _refused(create(sf=2.5), who, "scaleFactor")
    _refused(create(nlevels=0), who, "nlevels 0")
    _refused(create(nlevels=17), who, "nlevels 17")
    _refused(create(edge=2), who, "edgeThreshold 2")
    _refused(create(score=2), who, "scoreType 2")
    _refused(create(fast=0), who, "fastThreshold 0")
    _refused(create(fast=255), who, "fastThreshold 255")
    _refused(create(max_w=0), who, "frame size")
    _refused(create(max_h=20000), who, "frame size")
    bad = np.zeros((512, 2), np.int8)
    bad[7, 0] = -16
    _refused(create(pattern=bad), who, "pattern point 7", "-16")
    assert h.value is None
    buf = native.ptr(np.zeros(64, np.uint8))
    n = C.c_int32(-7)
    _refused(lib.sslam_orb_detect_host(None, buf, 4, 4, 1, buf, buf, buf, C.byref(n)), "sslam_orb_detect_host", "instance is NULL")
    _refused(lib.sslam_orb_detect_dev(None, buf, 4, 4, 1, buf, buf, buf, buf), "sslam_orb_detect_dev", "instance is NULL")
    _refused(lib.sslam_orb_capacity(None, None), "sslam_orb_capacity", "NULL")
    _refused(lib.sslam_orb_level_info(None, 0, buf), "sslam_orb_level_info", "NULL")
    _refused(lib.sslam_orb_stage_read(None, 0, None, None, None, None, None), "sslam_orb_stage_read", "NULL")
    _refused(lib.sslam_orb_default_pattern(None), "sslam_orb_default_pattern", "NULL")
    assert n.value == -7
    assert lib.sslam_orb_destroy(None) == 0


def test_the_default_pattern_needs_no_device():
    O = load_pkg("orb")
    p = O.default_pattern()
    assert p.dtype == np.int8 and p.shape == (512, 2) and p.min() == -15 and p.max() == 15
    assert p[:4].tolist() == [[13, -15], [3, 4], [10, 6], [-5, -6]]


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


def test_module_names_and_defaults():
    O = load_pkg("orb")
    assert (O.HARRIS_SCORE, O.FAST_SCORE) == (0, 1)
    sig = inspect.signature(O.ORB_create)
    assert list(sig.parameters) == ["nfeatures", "scaleFactor", "nlevels", "edgeThreshold", "firstLevel", "WTA_K", "scoreType", "patchSize",
                                    "fastThreshold", "pattern", "max_h", "max_w", "ctx"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert [d[k] for k in list(sig.parameters)[:9]] == [500, 1.2, 8, 31, 0, 2, O.HARRIS_SCORE, 31, 20]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("pattern", "max_h", "max_w", "ctx"))
    for name in ("detectAndCompute", "detect_arrays", "detect_dev", "stage_read"):
        assert callable(getattr(O.ORB, name))


def test_python_refuses_bad_arguments_without_the_library(no_library):
    O = load_pkg("orb")
    for kw, word in ((dict(firstLevel=1), "firstLevel"), (dict(WTA_K=3), "WTA_K"), (dict(WTA_K=4), "WTA_K"), (dict(patchSize=21), "patchSize"),
                     (dict(nfeatures=0), "nfeatures"), (dict(scaleFactor=1.0), "scaleFactor"), (dict(scaleFactor=2.5), "scaleFactor"),
                     (dict(nlevels=0), "nlevels"), (dict(nlevels=17), "nlevels"), (dict(edgeThreshold=2), "edgeThreshold"),
                     (dict(scoreType=2), "scoreType"), (dict(fastThreshold=0), "fastThreshold"), (dict(fastThreshold=255), "fastThreshold"),
                     (dict(max_w=0), "max_w"), (dict(pattern=np.zeros((256, 4), np.int8)), "pattern"),
                     (dict(pattern=np.zeros((512, 2), np.int16)), "pattern"), (dict(pattern=np.full((512, 2), 16, np.int8)), "-15..15")):
        with pytest.raises(ValueError, match=word):
            O.ORB_create(**kw)
    o = O.ORB_create(100, max_h=48, max_w=64)                                # (a valid construction touches nothing either)
    img = np.zeros((48, 64), np.uint8)
    with pytest.raises(ValueError, match="mask"):
        o.detectAndCompute(img, np.ones((48, 64), np.uint8))
    with pytest.raises(TypeError, match="float32"):
        o.detectAndCompute(img.astype(np.float32))
    with pytest.raises(TypeError, match="uint16"):
        o.detect_arrays(img.astype(np.uint16))
    with pytest.raises(ValueError, match="larger than the instance's 64x48"):
        o.detectAndCompute(np.zeros((49, 64), np.uint8))
    with pytest.raises(ValueError, match="larger than the instance's 64x48"):
        o.detectAndCompute(np.zeros((48, 65, 3), np.uint8), None)
    with pytest.raises(ValueError, match="larger"):
        o.detect_dev(0x1000, 48, 65, 1, 0x1000, 0x1000, 0x1000, 0x1000)
    with pytest.raises(ValueError, match="shape"):
        o.detectAndCompute(np.zeros((48, 64, 2), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        o.detectAndCompute(np.zeros(48, np.uint8))


def _args(**kw):
    return SimpleNamespace(use_lightglue=False, **kw)


def test_init_feature_pipeline_hands_out_the_gpu_pair_without_cv2(monkeypatch):
    """with the fake device as the default context: nothing of the real library is needed to build the pair"""
    fu, types, O, B, native = (load_pkg("slam.core.features_utils"), load_pkg("slam.core.types"), load_pkg("orb"), load_pkg("bf_matcher"),
                               load_pkg("_native"))
    assert not types.HAVE_CV2
    fake = fake_device.FakeContext()
    monkeypatch.setattr(native, "default_context", lambda device=0: fake)
    for args, nfeat in ((_args(detector="orb", matcher="bf", max_features=1234), 1234), (_args(), 6000), (_args(detector="orb"), 6000)):
        det, m = fu.init_feature_pipeline(args)
        assert isinstance(det, O.ORB) and isinstance(m, B.BFMatcher)
        assert (det.nfeatures, det.scaleFactor, det.nlevels, det.edgeThreshold, det.scoreType, det.fastThreshold) == (nfeat, 1.2, 8, 31, 0, 20)
        assert (det.max_h, det.max_w) == (fu.MAX_IMAGE_H, fu.MAX_IMAGE_W) and det.handle is None
        assert (m.normType, m.crossCheck) == (B.NORM_HAMMING, True)
        with pytest.raises(ValueError, match="mask"):                        # argument handling needs no device
            det.detectAndCompute(np.zeros((8, 8), np.uint8), np.ones((8, 8), np.uint8))
        assert m.match([], np.zeros((3, 32), np.uint8)) == []


@pytest.mark.parametrize("kw", [dict(detector="sift"), dict(detector="akaze"), dict(detector="orb", matcher="flann"),
                                dict(detector="sift", matcher="flann")])
def test_init_feature_pipeline_keeps_raising_for_what_stays_opencv_only(kw):
    fu = load_pkg("slam.core.features_utils")
    with pytest.raises(ImportError, match="the OpenCV detector/matcher branch needs cv2; this backend accelerates the --use_lightglue path only"):
        fu.init_feature_pipeline(_args(**kw))


def test_feature_extractor_maps_no_descriptors_to_empty_lists():
    fu = load_pkg("slam.core.features_utils")
    det = SimpleNamespace(detectAndCompute=lambda img, mask: ([], None))
    assert fu.feature_extractor(_args(), np.zeros((8, 8), np.uint8), det) == ([], [])


def test_product_imports_no_cv2_and_nothing_under_tests():
    src = (ROOT / "opencv-simpleslam_amd" / "orb.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(cv2|tests|oracle|orb_ref|orb_scenes)\b", src, flags=re.M)
