"""Keyframe-thumbnail surface without a GPU: the C-ABI header declares the seven entries, the binding and the library export them,
the module offers `Thumbnailer` / `resize` / `imencode_jpg`, arguments outside the backend's scope are refused before the library
is touched, the overlay `slam.core.keyframe_utils` imports with `cv2` and `lz4` absent, and `is_new_keyframe` takes each gate."""
import importlib
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, load_pkg

ENTRIES = ("sslam_thumb_create", "sslam_thumb_destroy", "sslam_thumb_capacity", "sslam_thumb_encode_host", "sslam_thumb_encode_dev",
           "sslam_thumb_resize_host", "sslam_thumb_stage_read")


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sslam_hip.h").read_text(), flags=re.S)


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_thumb_entry(name):
    assert re.search(rf"\bint\s+{name}\s*\(", _header()), name


@pytest.mark.parametrize("name", ENTRIES)
def test_library_and_binding_export_thumb_entry(name):
    native = load_pkg("_native")
    assert name in native.declared_symbols()
    assert hasattr(native.lib(), name)


def test_module_names_are_importable():
    T = load_pkg("thumbnail")
    assert callable(T.Thumbnailer) and callable(T.resize) and callable(T.imencode_jpg) and callable(T.cached)
    for name in ("encode", "encode_dev", "resize", "stage_read", "close"):
        assert callable(getattr(T.Thumbnailer, name))
    import inspect
    sig = inspect.signature(T.Thumbnailer.__init__).parameters
    assert sig["thumb_wh"].default == (640, 360) and sig["quality"].default == 70 and sig["ctx"].default is None
    assert inspect.signature(T.imencode_jpg).parameters["quality"].default == 95         # cv2's default
    import thumb_ref as R
    assert T.STAGES == R.STAGES and (T.MAX_DST, T.MAX_SRC, T.BLOCK_BYTES) == (R.MAX_DST, R.MAX_SRC, R.BLOCK_BYTES)
    for w, h in ((1, 1), (33, 17), (640, 360)):
        for c in (1, 3, 4):
            g, ref = T.geometry(w, h, c), R.geometry(w, h, c)
            assert g == {k: ref[k] for k in g}


@pytest.fixture
def no_library(monkeypatch):
    """every way into the library raises: a refusal must come before it"""
    native = load_pkg("_native")

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(native, "lib", boom)
    monkeypatch.setattr(native, "default_context", boom)


def test_bad_sizes_and_quality_raise_without_the_library(no_library):
    T = load_pkg("thumbnail")
    for kw, text in ((dict(quality=0), "quality 0 outside 1..100"), (dict(quality=101), "quality 101 outside 1..100"),
                     (dict(thumb_wh=(0, 360)), "thumbnail size 0x360 outside 1..4096"), (dict(thumb_wh=(640, 4097)), "thumbnail size 640x4097 outside 1..4096"),
                     (dict(max_src_wh=(16385, 376)), "source size 16385x376 outside 1..16384"), (dict(max_src_wh=(1241, 0)), "source size 1241x0 outside 1..16384")):
        a = dict(dict(max_src_wh=(1241, 376)), **kw)
        with pytest.raises(ValueError, match=re.escape(text)):
            T.Thumbnailer(**a)
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match="quality 0"):
        T.imencode_jpg(img, 0)
    with pytest.raises(ValueError, match="thumbnail size 0x3"):
        T.resize(img, (0, 3))
    with pytest.raises(ValueError, match="thumbnail size 4097x4"):
        T.imencode_jpg(np.zeros((4, 4097), np.uint8))


def test_bad_images_raise_without_the_library(no_library):
    T = load_pkg("thumbnail")
    img = np.zeros((4, 5, 3), np.uint8)
    for fn in (lambda a: T.resize(a, (3, 2)), lambda a: T.imencode_jpg(a, 70)):
        with pytest.raises(TypeError):
            fn(img.astype(np.float32))
        with pytest.raises(TypeError):
            fn(img.astype(np.uint16))
        with pytest.raises(ValueError, match="2 channels"):
            fn(np.zeros((4, 5, 2), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((4,), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 4, 5, 3), np.uint8))
        with pytest.raises(ValueError, match="source size"):
            fn(np.zeros((0, 5, 3), np.uint8))
    th = T.Thumbnailer.__new__(T.Thumbnailer)                  # an instance is not needed to refuse an image
    th.handle, th.max_src_wh, th.thumb_wh, th._last_c = None, (5, 4), (3, 2), 0
    with pytest.raises(TypeError):
        th.encode(img.astype(np.int16))
    with pytest.raises(ValueError, match="larger than the instance's 5x4"):
        th.encode(np.zeros((5, 5, 3), np.uint8))
    with pytest.raises(ValueError, match="larger than the instance's 5x4"):
        th.resize(np.zeros((4, 6), np.uint8))
    with pytest.raises(ValueError, match="7 channels"):
        th.encode_dev(0, 4, 5, 7, 0, 0)
    with pytest.raises(ValueError, match="no encode yet"):
        th.stage_read("y")


def test_product_imports_no_cv2_and_nothing_under_tests():
    for rel in ("thumbnail.py", "slam/core/keyframe_utils.py"):
        src = (ROOT / PKG_NAME / rel).read_text()
        assert not re.search(r"^\s*(from|import)\s+(cv2|tests|oracle|thumb_ref|PIL)\b", src, flags=re.M), rel
    kf = (ROOT / PKG_NAME / "slam" / "core" / "keyframe_utils.py").read_text()
    assert re.search(r"try:[^\n]*\n\s+import lz4\.frame", kf)                         # lz4 only inside a try


@pytest.fixture
def kfu(monkeypatch):
    """the overlay imported afresh with `cv2` and `lz4` unimportable"""
    name = PKG_NAME + ".slam.core.keyframe_utils"
    for mod in ("cv2", "lz4", "lz4.frame"):
        monkeypatch.setitem(sys.modules, mod, None)            # `import cv2` raises ImportError
    monkeypatch.delitem(sys.modules, name, raising=False)
    mod = importlib.import_module(name)
    yield mod
    sys.modules.pop(name, None)


def test_overlay_imports_without_cv2_and_lz4_and_carries_the_references_names(kfu):
    import dataclasses
    import inspect
    assert kfu._lz4_frame is None
    assert [f.name for f in dataclasses.fields(kfu.Keyframe)] == ["idx", "frame_idx", "path", "kps", "desc", "pose", "thumb"]
    assert inspect.signature(kfu.make_thumb).parameters["hw"].default == (640, 360)
    p = inspect.signature(kfu.is_new_keyframe).parameters
    assert list(p) == ["frame_no", "matches_to_kf", "kp_curr", "kp_kf", "Tcw_prev_kf", "Tcw_curr", "kf_cooldown", "kf_min_inliers", "kf_min_ratio",
                       "kf_max_disp", "kf_min_rot_deg", "last_kf_frame_no"]
    assert [p[k].default for k in list(p)[6:]] == [5, 125, 0.35, 30.0, 8.0, -999]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    assert list(inspect.signature(kfu.select_keyframe).parameters) == ["args", "seq", "frame_idx", "img2", "kp2", "des2", "Tcw_curr", "matcher", "kfs",
                                                                      "last_kf_frame_no"]
    fu = load_pkg("slam.core.features_utils")
    assert kfu.feature_matcher is fu.feature_matcher and kfu.filter_matches_ransac is fu.filter_matches_ransac
    with pytest.raises(TypeError):
        kfu.make_thumb(np.zeros((4, 4, 3), np.float32))


def _rot_y(deg):
    T = np.eye(4)
    a = np.radians(deg)
    T[0, 0] = T[2, 2] = np.cos(a)
    T[0, 2], T[2, 0] = np.sin(a), -np.sin(a)
    return T


def test_is_new_keyframe_takes_each_gate(kfu):
    types = load_pkg("slam.core.types")
    n = 200
    rng = np.random.default_rng(0)
    xy = rng.uniform(0, 600, (n, 2)).astype(np.float32)
    kp_kf = types.keypoints_from_xy(xy)

    def matches(k):
        return types.matches_from_ij(np.stack([np.arange(k), np.arange(k)], 1))

    def moved(d):
        return types.keypoints_from_xy(xy + np.float32([d, 0]))
    kw = dict(last_kf_frame_no=10)
    still = (matches(150), moved(3.0), kp_kf, np.eye(4), _rot_y(1.0))
    assert kfu.is_new_keyframe(12, *still, **kw) is False                              # none of the gates
    assert kfu.is_new_keyframe(15, *still, **kw) is False                              # age == cooldown: not yet
    assert kfu.is_new_keyframe(16, *still, **kw) is True                               # age over the cooldown
    assert kfu.is_new_keyframe(12, *still, kf_cooldown=1, **kw) is True
    assert kfu.is_new_keyframe(12, matches(124), *still[1:], **kw) is True             # few inliers
    assert kfu.is_new_keyframe(12, matches(125), *still[1:], **kw) is False
    many = types.keypoints_from_xy(np.concatenate([xy, xy, xy]))                      # 600 reference keypoints: 150 / 600 < 0.35
    assert kfu.is_new_keyframe(12, still[0], still[1], many, *still[3:], **kw) is True  # low ratio
    assert kfu.is_new_keyframe(12, still[0], still[1], many, *still[3:], kf_min_ratio=0.25, **kw) is False
    assert kfu.is_new_keyframe(12, matches(150), moved(31.0), *still[2:], **kw) is True  # median displacement
    assert kfu.is_new_keyframe(12, matches(150), moved(29.0), *still[2:], **kw) is False
    # the MEDIAN, not the mean: 70 of 150 matches far away leave the median small
    far = xy + np.float32([3, 0])
    far[:70] += np.float32([500, 0])
    assert kfu.is_new_keyframe(12, matches(150), types.keypoints_from_xy(far), *still[2:], **kw) is False
    assert kfu.is_new_keyframe(12, *still[:4], _rot_y(9.0), **kw) is True              # rotation
    assert kfu.is_new_keyframe(12, *still[:3], None, None, **kw) is False              # no poses: no rotation signal
    assert kfu.is_new_keyframe(12, [], moved(0), kp_kf, None, None, kf_min_inliers=0, kf_min_ratio=0.0, **kw) is False     # no matches at all
    assert abs(kfu._rot_deg_from_Tcw(np.eye(4), _rot_y(9.0)) - 9.0) < 1e-9
    # the indices are read from the matches (a shuffled, partial set)
    perm = rng.permutation(n)[:150]
    shuffled = types.matches_from_ij(np.stack([perm, perm], 1))
    assert kfu.is_new_keyframe(12, shuffled, moved(31.0), *still[2:], **kw) is True
    assert kfu.is_new_keyframe(12, shuffled, moved(3.0), *still[2:], **kw) is False


def test_select_keyframe_skips_the_matching_inside_the_cooldown(kfu, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("matched inside the cooldown")
    monkeypatch.setattr(kfu, "feature_matcher", boom)
    args = SimpleNamespace(kf_cooldown=5, kf_min_rot_deg=8.0)
    kf = kfu.Keyframe(0, 0, "", [], np.zeros((0, 128), np.float32), np.eye(4), b"")
    kfs, last = kfu.select_keyframe(args, [None] * 8, 2, None, [], None, _rot_y(1.0), None, [kf], 0)
    assert len(kfs) == 1 and last == 0
    assert kfu.select_keyframe(args, [None] * 8, 2, None, [], None, None, None, [], 0) == ([], 0)
