"""The overlay `slam.core.keyframe_utils` on the GPU with cv2 (and lz4) absent: `make_thumb` on a KITTI-sized frame returns a JPEG
that Pillow opens at 640 x 360, and `select_keyframe`, driven as the reference's frame loop drives it on a short synthetic
sequence (the default ORB + BF branch), promotes a keyframe whose thumbnail decodes and is as close to the resized frame as
Pillow's own encode of it, within the bound of tests/thumb_ref.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import orb_scenes as S
import thumb_ref as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu


def _jpeg(kfu, thumb):
    """what the reference's reader does: the lz4 frame where there is one, else the bytes as they are"""
    return kfu._lz4_frame.decompress(thumb) if kfu._lz4_frame is not None else thumb


def test_make_thumb_on_a_kitti_frame_is_a_jpeg_of_640_by_360(gpu_ctx):
    kfu = load_pkg("slam.core.keyframe_utils")
    frame = R.natural(376, 1241, 3, seed=4)
    thumb = kfu.make_thumb(frame)
    assert isinstance(thumb, bytes)
    jpeg = _jpeg(kfu, thumb)
    im = R.decode(jpeg)
    assert im.size == (640, 360) and im.mode == "RGB"
    assert jpeg == R.encode(frame, (640, 360), 70)["jpeg"]
    grey = kfu.make_thumb(frame[:, :, 1])                      # KITTI's grey frames: one component
    im = R.decode(_jpeg(kfu, grey))
    assert im.size == (640, 360) and im.mode == "L"
    T = load_pkg("thumbnail")
    assert kfu.make_thumb(frame) == thumb and (id(gpu_ctx), 1241, 376, 640, 360, 70) in T._instances     # one cached instance serves all three


def test_select_keyframe_promotes_a_keyframe_with_a_thumbnail(gpu_ctx):
    kfu, fu = load_pkg("slam.core.keyframe_utils"), load_pkg("slam.core.features_utils")
    args = SimpleNamespace(use_lightglue=False, detector="orb", matcher="bf", max_features=2000, ransac_thresh=1.0, kf_cooldown=5,
                           kf_min_inliers=125, kf_max_disp=30.0, kf_thumb_hw=(64, 48))
    detector, matcher = fu.init_feature_pipeline(args)
    h, w, n, dx = 120, 160, 8, 2
    big = S.mosaic(h, w + n * dx, seed=5, channels=3)
    seq = [np.ascontiguousarray(big[:, k * dx:k * dx + w]) for k in range(n)]          # the camera slides 2 px per frame
    try:
        kp, des = fu.feature_extractor(args, seq[0], detector)
        kfs = [kfu.Keyframe(0, 0, "", kp, des, np.eye(4), kfu.make_thumb(seq[0], (64, 48)))]
        last, promoted_at = 0, []
        for i in range(n - 1):
            kp2, des2 = fu.feature_extractor(args, seq[i + 1], detector)
            before = len(kfs)
            kfs, last = kfu.select_keyframe(args, seq, i, seq[i + 1], kp2, des2, np.eye(4), matcher, kfs, last)
            if len(kfs) > before:
                promoted_at.append(i + 1)
    finally:
        detector.close()
    assert promoted_at == [6] and last == 6                    # inside the cooldown nothing, then the pessimistic cooldown's promotion
    kf = kfs[-1]
    assert (kf.idx, kf.frame_idx, kf.path) == (1, 6, "") and len(kf.kps) > 100 and len(kf.desc) == len(kf.kps)
    jpeg = _jpeg(kfu, kf.thumb)
    im = R.decode(jpeg)
    assert im.size == (64, 48) and im.mode == "RGB"
    small = R.resize(seq[6], (64, 48))
    d_db, d_scan, ours_db = R.gaps(jpeg, small, 70)
    print(f"keyframe thumbnail: PSNR {ours_db:.3f} dB, Pillow's minus ours {d_db:+.3f} dB, scan bytes over Pillow's {100 * d_scan:+.2f} %")
    assert d_db <= R.GAP_PSNR_DB
    assert jpeg == R.encode(seq[6], (64, 48), 70)["jpeg"]
