"""The base class of the drop-in detectors (`_detector.py`) without a library: for ORB, SIFT and AKAZE alike the image refusals
- a mask, a dtype, a bad shape, 2 channels, an oversize image - come before the library is touched and carry the class's own
name, a [h, w] image becomes a contiguous [h, w, 1], `close()` on an object that never made its instance is a no-op, and only
the detectors with list capacities have `overflow()`."""
import numpy as np
import pytest

from conftest import load_pkg

DETECTORS = (("orb", "ORB", "ORB_create"), ("sift", "SIFT", "SIFT_create"), ("akaze", "AKAZE", "AKAZE_create"))


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


@pytest.fixture(params=DETECTORS, ids=[d[1] for d in DETECTORS])
def det(request, no_library):
    module, name, create = request.param
    M = load_pkg(module)
    o = getattr(M, create)(max_h=48, max_w=64)
    assert isinstance(o, load_pkg("_detector").Detector) and type(o) is getattr(M, name) and o.NAME == name and o.PREFIX == module
    return name, o


def test_image_refusals_carry_the_class_name(det):
    name, o = det
    who = f"{name}.detectAndCompute: "
    img = np.zeros((48, 64), np.uint8)
    cases = ((img, np.ones((48, 64), np.uint8), ValueError, who + "a mask is not supported"),
             (img.astype(np.float32), None, TypeError, who + "image is float32, want uint8"),
             (img.astype(np.uint16), None, TypeError, who + "image is uint16, want uint8"),
             (np.zeros(48, np.uint8), None, ValueError, who + "image must be [h, w] or [h, w, 1 | 3 | 4], got shape (48,)"),
             (np.zeros((48, 64, 3, 1), np.uint8), None, ValueError, who + "image must be [h, w] or [h, w, 1 | 3 | 4], got shape (48, 64, 3, 1)"),
             (np.zeros((48, 64, 2), np.uint8), None, ValueError, who + "image must be [h, w] or [h, w, 1 | 3 | 4], got shape (48, 64, 2)"),
             (np.zeros((0, 64), np.uint8), None, ValueError, who + "image must be [h, w] or [h, w, 1 | 3 | 4], got shape (0, 64, 1)"),
             (np.zeros((49, 64), np.uint8), None, ValueError, who + "image 64x49 is larger than the instance's 64x48 (max_w x max_h)"),
             (np.zeros((48, 65, 3), np.uint8), None, ValueError, who + "image 65x48 is larger than the instance's 64x48 (max_w x max_h)"))
    for image, mask, kind, text in cases:
        for call in (o._image, o.detect_arrays, o.detectAndCompute):
            with pytest.raises(kind) as e:
                call(image, mask)
            assert str(e.value) == text and type(e.value) is kind
    n_out = {"ORB": 3}.get(name, 4)
    with pytest.raises(ValueError) as e:
        o.detect_dev(0x1000, 48, 65, 1, *[0x1000] * (n_out + 1))
    assert str(e.value) == f"{name}.detect_dev: image 65x48 is larger than the instance's 64x48"
    with pytest.raises(ValueError, match=f"{name}.detect_dev: image 64x0 is larger"):
        o.detect_dev(0x1000, 0, 64, 1, *[0x1000] * (n_out + 1))


def test_accepted_images_become_contiguous_h_w_c(det):
    _, o = det
    grey = np.arange(48 * 64, dtype=np.uint8).reshape(48, 64)
    out = o._image(grey, None)
    assert out.shape == (48, 64, 1) and out.dtype == np.uint8 and out.flags.c_contiguous and np.array_equal(out[:, :, 0], grey)
    wide = np.arange(20 * 60 * 3, dtype=np.uint8).reshape(20, 60, 3)
    view = wide[:, ::2]                                  # not contiguous
    out = o._image(view, None)
    assert out.shape == (20, 30, 3) and out.flags.c_contiguous and np.array_equal(out, view)
    for c in (1, 3, 4):
        assert o._image(np.zeros((1, 1, c), np.uint8), None).shape == (1, 1, c)
    with pytest.raises(TypeError):                       # (a list of ints is int64: refused, never cast)
        o._image(grey.tolist(), None)


def test_close_without_an_instance_is_a_no_op(det):
    _, o = det
    assert o.handle is None and o.capacity == 0 and o._out is None
    o.close(); o.close()
    assert o.handle is None
    del o                                                # (__del__ closes again)


def test_only_the_detectors_with_capacities_have_overflow(no_library):
    D = load_pkg("_detector")
    orb, sift, akaze = load_pkg("orb").ORB, load_pkg("sift").SIFT, load_pkg("akaze").AKAZE
    assert not hasattr(orb, "overflow") and not issubclass(orb, D.CapacityDetector)
    assert not hasattr(orb(max_h=8, max_w=8), "candidate_capacity")
    for cls in (sift, akaze):
        assert issubclass(cls, D.CapacityDetector) and callable(cls.overflow) and cls(max_h=8, max_w=8).candidate_capacity == 0
    for cls in (orb, sift, akaze):
        assert isinstance(cls.chain_rows, property)
        for name in ("_instance", "close", "__del__", "_image", "_detect_host", "chain_rows"):
            assert name not in vars(cls), (cls, name)    # one copy, on the base
    # the public module attributes stay importable from their modules
    assert (load_pkg("orb").MAX_SIDE, load_pkg("sift").MAX_SIDE, load_pkg("akaze").MAX_SIDE) == (16384,) * 3
    assert (load_pkg("orb").HARRIS_SCORE, load_pkg("orb").FAST_SCORE, load_pkg("sift").CV_32F, load_pkg("akaze").DESC_BYTES) == (0, 1, 5, 61)
