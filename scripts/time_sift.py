"""SIFT timing: `sslam_sift_detect_dev` (timing events around `reps` back-to-back enqueues on the context stream after a
warm-up, five windows; the memset and every kernel of a frame are inside, nothing is read back) on a structured 1241 x 376 frame
at nfeatures 2048 and 6000 (the reference's default for this branch), the host entry (upload + call + download, wall clock), and
the keypoint count checked against the host entry.  `time_sift.py REPS [NFEATURES]`; under `rocprofv3 --kernel-trace --stats`
with a small REPS and one NFEATURES it gives the per-kernel split and the launch count of a frame (a run of its own)."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import orb_scenes
T = importlib.import_module("opencv-simpleslam_amd.sift")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
features = [int(sys.argv[2])] if len(sys.argv) > 2 else [2048, 6000]
H, W = 376, 1241
ctx = N.default_context(0)
img = orb_scenes.mosaic(H, W, seed=11, block=9)
for nf in features:
    o = T.SIFT_create(nf, max_h=H, max_w=W, ctx=ctx)
    xy, aux, octave, desc = o.detect_arrays(img)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); o.detect_arrays(img); ts.append(time.perf_counter() - t0)
    cap = o.capacity
    d = [ctx.upload(img), ctx.malloc(cap * 8), ctx.malloc(cap * 12), ctx.malloc(cap * 4), ctx.malloc(cap * 512), ctx.malloc(4)]
    run = lambda: o.detect_dev(d[0], H, W, 1, d[1], d[2], d[3], d[4], d[5])
    for _ in range(min(10, reps)):
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
    n = np.zeros(1, np.int32); ctx.d2h(n, d[5])
    assert n[0] == len(xy)
    counts = o.stage_read(0)["counts"].tolist()
    info = o.octave_info(0)
    octs = [int(((((octave & 255) + 1) & 255) == i).sum()) for i in range(info["octaves"])]
    px = [o.octave_info(i)["w"] * o.octave_info(i)["h"] for i in range(info["octaves"])]
    m = info["octaves"]                                        # the plan's tail_first: one launch computes the small octaves behind it
    while m > 1 and px[m - 1] <= 8192:
        m -= 1
    launches = 1 + 2 * (1 + m * (info["layers"] - 1)) + (m - 1) + (m < info["octaves"]) + 5
    for p in d:
        ctx.free(p)
    o.close()
    print(f"sift {W} x {H}, nfeatures {nf}: device entry {np.median(per):.1f} us per frame (min {min(per):.1f}, max {max(per):.1f} over 5 x {reps}); "
          f"host entry {np.median(ts) * 1e3:.3f} ms; {counts[0]} extrema, {counts[1]} keypoints before the quota, {len(xy)} rows, per octave {octs}; "
          f"{info['octaves']} octaves, {launches} launches and a memset; capacity {cap} rows", flush=True)
