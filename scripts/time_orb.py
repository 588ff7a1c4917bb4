"""ORB timing: `sslam_orb_detect_dev` (timing events around `reps` back-to-back enqueues on the context stream after a warm-up,
five windows; the memset and every kernel of a frame are inside, nothing is read back) on a structured 1241 x 376 frame at
nfeatures 2048 and 6000 (the reference's default for this branch), the host entry (upload + call + download, wall clock), and
the keypoint count checked against the host entry.  `time_orb.py REPS [NFEATURES]`; under `rocprofv3 --kernel-trace --stats`
with a small REPS and one NFEATURES it gives the per-kernel split and the launch count of a frame (a run of its own)."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import orb_scenes
O = importlib.import_module("opencv-simpleslam_amd.orb")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
features = [int(sys.argv[2])] if len(sys.argv) > 2 else [2048, 6000]
H, W = 376, 1241
ctx = N.default_context(0)
img = orb_scenes.mosaic(H, W, seed=11, block=9)
for nf in features:
    o = O.ORB_create(nf, max_h=H, max_w=W, ctx=ctx)
    xy, aux, desc = o.detect_arrays(img)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); o.detect_arrays(img); ts.append(time.perf_counter() - t0)
    cap = o.capacity
    d = [ctx.upload(img), ctx.malloc(cap * 8), ctx.malloc(cap * 16), ctx.malloc(cap * 32), ctx.malloc(4)]
    run = lambda: o.detect_dev(d[0], H, W, 1, d[1], d[2], d[3], d[4])
    for _ in range(min(20, reps)):
        run()
    ctx.sync()
    e0, e1 = ctx.timing_event(), ctx.timing_event()
    per = []
    for _ in range(5):
        ctx.record(e0)
        for _ in range(reps):
            run()
        ctx.record(e1); ctx.sync()
        per.append(ctx.elapsed_ms(e0, e1) / reps * 1e3)
    n = np.zeros(1, np.int32); ctx.d2h(n, d[4])
    assert n[0] == len(xy)
    levels = [int((aux[:, 3] == l).sum()) for l in range(8)]
    for p in d:
        ctx.free(p)
    o.close()
    print(f"orb {W} x {H}, nfeatures {nf}: device entry {np.median(per):.1f} us per frame (min {min(per):.1f}, max {max(per):.1f} over 5 x {reps}); "
          f"host entry {np.median(ts) * 1e3:.3f} ms; {len(xy)} keypoints, per level {levels}; capacity {cap} rows", flush=True)
