"""`feature_extractor(args, und.remap(img), det)`: the extractor reads the undistorted frame where the remap kernel left it on
the device (no second upload) when it is handed exactly the array `Undistorter.remap` returned last; a copy of it takes the
upload path - with the same keypoints and descriptors, bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest

import frames
import undistort_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

SD_L = dict(seed=1, match_gain=4.0, match_bias=3.0)      # random-init weights that produce matches (not vacuous)
SIZE = (161, 97)


@pytest.fixture(scope="module")
def fu():
    return load_pkg("slam.core.features_utils")


@pytest.fixture(scope="module")
def pipeline(fu, gpu_ctx):
    """init_feature_pipeline(args) on seeded random weights, as tests/test_dropin_names_gpu.py sets it up"""
    W = load_pkg("weights")
    sd = W.random_lightglue_state_dict(SD_L["seed"], match_gain=SD_L["match_gain"], match_bias=SD_L["match_bias"])
    mp = pytest.MonkeyPatch()
    mp.setattr(fu._weights, "random_lightglue_state_dict", lambda seed=0: sd)
    mp.setenv(fu.ENV_ALLOW_RANDOM, "1")
    mp.delenv(fu.ENV_ALIKED, raising=False); mp.delenv(fu.ENV_LIGHTGLUE, raising=False)
    args = SimpleNamespace(use_lightglue=True, min_conf=0.05)
    det, mat = fu.init_feature_pipeline(args)
    mp.undo()
    yield args, det, mat
    det.close(); mat.close()


@pytest.fixture(scope="module")
def und(pipeline):
    U = load_pkg("undistort")
    K, D = S.camera("tum_fr1", SIZE)
    u = U.Undistorter(K, D, SIZE, ctx=pipeline[1].ctx)
    yield u
    u.close()


def _xy(kps):
    return np.array([k.pt for k in kps], np.float32).reshape(-1, 2)


def test_extractor_takes_the_device_copy_three_frames_in_a_row(fu, pipeline, und):
    args, det, _ = pipeline
    ring = fu._ring_of(det)
    for idx in range(3):
        img = frames.structured_frame(idx, h=SIZE[1], w=SIZE[0])
        out = und.remap(img)
        assert not out.flags.writeable
        with pytest.raises(ValueError):
            out[0, 0, 0] = 1
        skipped = ring.stats["upload_skipped"]
        kp_a, des_a = fu.feature_extractor(args, out, det)
        assert ring.stats["upload_skipped"] == skipped + 1               # exactly the returned array: no upload
        kp_b, des_b = fu.feature_extractor(args, np.array(out), det)
        assert ring.stats["upload_skipped"] == skipped + 1               # a copy: uploaded
        assert len(kp_a) == len(kp_b) > 0
        np.testing.assert_array_equal(_xy(kp_a), _xy(kp_b))
        np.testing.assert_array_equal(des_a, des_b)


def test_an_older_frame_a_slice_and_another_context_take_the_upload_path(fu, pipeline, und, native):
    args, det, _ = pipeline
    ring = fu._ring_of(det)
    img0 = frames.structured_frame(5, h=SIZE[1], w=SIZE[0])
    img1 = frames.structured_frame(6, h=SIZE[1], w=SIZE[0])
    old = und.remap(img0)
    new = und.remap(img1)
    skipped = ring.stats["upload_skipped"]
    kp_o, des_o = fu.feature_extractor(args, old, det)                   # not the last one any more
    assert ring.stats["upload_skipped"] == skipped
    kp_r, des_r = fu.feature_extractor(args, np.array(old), det)
    np.testing.assert_array_equal(_xy(kp_o), _xy(kp_r)); np.testing.assert_array_equal(des_o, des_r)
    fu.feature_extractor(args, new[:], det)                              # a view of the last one: another object
    assert ring.stats["upload_skipped"] == skipped
    kp_n, des_n = fu.feature_extractor(args, new, det)                   # the last one, after other extractions: still in place
    assert ring.stats["upload_skipped"] == skipped + 1
    kp_c, des_c = fu.feature_extractor(args, np.array(new), det)
    np.testing.assert_array_equal(_xy(kp_n), _xy(kp_c)); np.testing.assert_array_equal(des_n, des_c)
    # the returned array made writable again (it owns its data): the read-only guarantee is gone, so it is uploaded
    loose = und.remap(img1)
    loose.setflags(write=True)
    loose[0, 0, 0] ^= 255
    kp_w, des_w = fu.feature_extractor(args, loose, det)
    assert ring.stats["upload_skipped"] == skipped + 1
    kp_v, des_v = fu.feature_extractor(args, loose.copy(), det)
    np.testing.assert_array_equal(_xy(kp_w), _xy(kp_v)); np.testing.assert_array_equal(des_w, des_v)
    # an Undistorter of another context: its device copy lives behind another stream, so the image is uploaded
    other = native.Context(det.ctx.device)
    U = load_pkg("undistort")
    K, D = S.camera("tum_fr1", SIZE)
    u2 = U.Undistorter(K, D, SIZE, ctx=other)
    try:
        out2 = u2.remap(img1)
        np.testing.assert_array_equal(out2, new)
        fu.feature_extractor(args, out2, det)
        assert ring.stats["upload_skipped"] == skipped + 1
    finally:
        u2.close(); other.close()
