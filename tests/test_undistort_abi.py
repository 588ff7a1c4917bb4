"""Lens-undistortion surface without a GPU: the C-ABI header declares the six entries, the binding and the library export them,
the module offers `Undistorter` / `remap` / `get_optimal_new_camera_matrix`, and arguments outside the backend's scope are
refused before the library is touched."""
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

ENTRIES = ("sslam_undistort_create", "sslam_undistort_create_from_maps", "sslam_undistort_destroy", "sslam_undistort_maps_read",
           "sslam_undistort_remap_host", "sslam_undistort_remap_dev")
K = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sslam_hip.h").read_text(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_undistort_entry(name):
    assert re.search(rf"\bint\s+{name}\s*\(", _header()), name


@pytest.mark.parametrize("name", ENTRIES)
def test_library_and_binding_export_undistort_entry(name):
    native = load_pkg("_native")
    assert name in native.declared_symbols()
    assert hasattr(native.lib(), name)


def test_module_names_are_importable():
    U = load_pkg("undistort")
    assert callable(U.Undistorter) and callable(U.remap) and callable(U.get_optimal_new_camera_matrix)
    assert callable(U.Undistorter.from_maps)
    for name in ("maps", "fixed_maps", "remap", "remap_dev", "close"):
        assert callable(getattr(U.Undistorter, name))


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


@pytest.mark.parametrize("n", [12, 14])
def test_thin_prism_and_tilt_coefficients_are_not_implemented(n, no_library):
    U = load_pkg("undistort")
    with pytest.raises(NotImplementedError, match="coefficients"):
        U.Undistorter(K, np.zeros(n), (640, 480))
    with pytest.raises(NotImplementedError, match="coefficients"):
        U.get_optimal_new_camera_matrix(K, np.zeros((1, n)), (640, 480))


def test_bad_coefficients_matrix_and_size_raise(no_library):
    U = load_pkg("undistort")
    with pytest.raises(ValueError):
        U.Undistorter(K, np.zeros(3), (640, 480))
    with pytest.raises(ValueError):
        U.Undistorter(K[:2], np.zeros(4), (640, 480))
    with pytest.raises(ValueError):
        U.Undistorter(K, np.zeros(4), (0, 480))
    with pytest.raises(ValueError):
        U.Undistorter(K, np.zeros(4), (640, 16385))


def test_bad_images_and_maps_raise_without_the_library(no_library):
    U = load_pkg("undistort")
    mx = np.zeros((4, 5), np.float32)
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(TypeError):
        U.remap(img.astype(np.float32), mx, mx)
    with pytest.raises(ValueError):
        U.remap(np.zeros((4, 5, 2), np.uint8), mx, mx)                   # two channels
    with pytest.raises(ValueError):
        U.remap(np.zeros((4,), np.uint8), mx, mx)
    with pytest.raises(ValueError):
        U.remap(np.zeros((2, 4, 5, 3), np.uint8), mx, mx)
    with pytest.raises(TypeError):
        U.remap(img, mx.astype(np.float64), mx)
    with pytest.raises(ValueError):
        U.remap(img, mx, np.zeros((5, 4), np.float32))
    with pytest.raises(ValueError):
        U.Undistorter.from_maps(np.zeros((4, 5, 1), np.float32), np.zeros((4, 5, 1), np.float32))
    und = U.Undistorter.__new__(U.Undistorter)                             # an instance is not needed to refuse an image
    und.handle = None
    with pytest.raises(TypeError):
        und.remap(img.astype(np.int16))
    with pytest.raises(ValueError):
        und.remap(np.zeros((4, 5, 5), np.uint8))


def test_all_zero_distortion_is_a_valid_model():
    U = load_pkg("undistort")
    newK, roi = U.get_optimal_new_camera_matrix(K, np.zeros(5), (640, 480))
    np.testing.assert_allclose(newK, K, rtol=1e-9)
    assert roi[2] > 0 and roi[3] > 0


def test_product_imports_no_cv2_and_nothing_under_tests():
    src = (ROOT / "opencv-simpleslam_amd" / "undistort.py").read_text()
    assert not re.search(r"^\s*(from|import)\s+(cv2|tests|oracle|undistort_ref|undistort_scenes)\b", src, flags=re.M)


def test_device_copy_is_only_the_last_returned_read_only_array():
    """`feature_ring.extract` asks `device_copy(img, ctx)`: None for any array no `Undistorter` returned (no library needed)."""
    U = load_pkg("undistort")
    img = np.zeros((4, 5, 3), np.uint8)
    assert U.device_copy(img, object()) is None
    img.setflags(write=False)
    assert U.device_copy(img, object()) is None
