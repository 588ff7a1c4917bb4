"""Lens-undistortion timing at 640 x 480 x 3 and 1241 x 376 x 3 (the TUM fr1 calibration scaled to the size), median of `reps`
warm calls after a warm-up, between two timing events on the context stream:
  * `remap_dev` alone (device to device), also as GB/s of (6 + 2 C) H W bytes: 6 B of record, C gathered, C written per pixel;
  * `und.remap(img)` host to host (upload, kernel, read-back into a fresh array), and its wall clock;
  * the drop-in frame `feature_extractor(args, und.remap(img), det)` against `feature_extractor(args, img, det)` on the same
    build: what undistortion adds to a frame (wall clock; both calls end synchronised), and the same with a COPY of the
    undistorted frame (the upload path) to show what taking the device copy saves.
Needs SSLAM_ALLOW_RANDOM_WEIGHTS=1 (no checkpoint: the extractor's time does not depend on the weights)."""
import importlib, sys, time
from pathlib import Path
from types import SimpleNamespace
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import undistort_scenes as S
U = importlib.import_module("opencv-simpleslam_amd.undistort")
FU = importlib.import_module("opencv-simpleslam_amd.slam.core.features_utils")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
args = SimpleNamespace(use_lightglue=True, min_conf=0.05, max_features=2048)
det, mat = FU.init_feature_pipeline(args)
ctx = det.ctx
e0, e1 = ctx.timing_event(), ctx.timing_event()


def timed(fn):
    for _ in range(10):
        fn()
    ctx.sync()
    ev, wall = [], []
    for _ in range(reps):
        ctx.record(e0); t0 = time.perf_counter()
        fn()
        ctx.record(e1); ctx.sync(); wall.append(time.perf_counter() - t0)
        ev.append(ctx.elapsed_ms(e0, e1))
    return np.median(ev) * 1e3, np.median(wall) * 1e3


for size in ((640, 480), (1241, 376)):
    W, H = size
    K, D = S.camera("tum_fr1", size)
    und = U.Undistorter(K, D, size, ctx=ctx)
    rng = np.random.default_rng(W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for C in (1, 3, 4):
        src_h = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        src, dst = ctx.upload(src_h), ctx.malloc(H * W * C)
        ev, _ = timed(lambda: und.remap_dev(src, H, W, C, dst))
        print(f"{W}x{H}x{C} remap_dev: {ev:.1f} us between events, {(6 + 2 * C) * H * W / (ev * 1e-6) / 1e9:.0f} GB/s of (6 + 2C) H W bytes", flush=True)
        ctx.sync(); ctx.free(src); ctx.free(dst)
    ev, wall = timed(lambda: und.remap(img))
    print(f"{W}x{H}x3 und.remap(img) host to host: {ev:.1f} us between events, {wall:.3f} ms wall", flush=True)
    _, plain = timed(lambda: FU.feature_extractor(args, img, det))
    _, with_und = timed(lambda: FU.feature_extractor(args, und.remap(img), det))
    _, with_copy = timed(lambda: FU.feature_extractor(args, np.array(und.remap(img)), det))
    print(f"{W}x{H}x3 feature_extractor(img): {plain:.3f} ms; feature_extractor(und.remap(img)): {with_und:.3f} ms "
          f"(+{with_und - plain:.3f}); with a copy of the undistorted frame (uploaded again): {with_copy:.3f} ms", flush=True)
    und.close()
det.close(); mat.close()
