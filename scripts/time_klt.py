"""Pyramidal Lucas-Kanade timing (csrc/klt_kernels.hip) at 1241 x 376 on `frames.structured_frame` (BGR, 3 px shift per frame),
main4's parameters (21 x 21, maxLevel 3, 30 iterations, epsilon 1e-3), between two timing events on the context stream, median
of REPS warm calls:
  push_dev     grey + pyramid + derivatives of a frame that is already on the device (8 launches at four levels)
  push_host    the same from a host array (upload included; the call returns synchronised)
  track_fb_dev forward + backward + gate (3 launches) on device-resident points, nothing read back, for 2048 and 4000 points (and 256:
               the floor one point's chain of levels and iterations sets)
  track_host   `KLTTracker.track`: upload of the points, the same three launches, read-back of the kept pairs
Prints one JSON line.  There is no bar to hold it against: the parent commit has no such entry and cv2 is not installed here,
so neither can be timed beside it.  usage: python scripts/time_klt.py [REPS]"""
import importlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
from frames import structured_frame

N = importlib.import_module("opencv-simpleslam_amd._native")
O = importlib.import_module("opencv-simpleslam_amd.optical_flow")
B = importlib.import_module("opencv-simpleslam_amd.build")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
H, W = 376, 1241
ctx = N.default_context()
e0, e1 = ctx.timing_event(), ctx.timing_event()


def timed(fn, warm=5):
    for _ in range(warm):
        fn()
    ctx.sync()
    out = []
    for _ in range(REPS):
        ctx.record(e0)
        fn()
        ctx.record(e1); ctx.sync()
        out.append(ctx.elapsed_ms(e0, e1) * 1e3)
    return round(float(np.median(out)), 1)


frames = [structured_frame(i, H, W, 3) for i in range(2)]
dev = [ctx.upload(f) for f in frames]
klt = O.KLTTracker((W, H), ctx=ctx)
res = {"what": "KLT at 1241x376x3, winSize 21x21, maxLevel 3, criteria (30, 1e-3); HIP-event microseconds, median of REPS", "reps": REPS,
       "csrc_digest": B.source_digest(), "levels": None}
turn = [0]


def push_dev():
    turn[0] ^= 1
    klt.push_dev(dev[turn[0]], H, W, 3)


def push_host():
    turn[0] ^= 1
    O._Instance.push(klt, frames[turn[0]])


res["push_dev_us"] = timed(push_dev)
res["push_host_us"] = timed(push_host)
klt.push_dev(dev[0], H, W, 3); klt.push_dev(dev[1], H, W, 3); ctx.sync()
res["levels"] = klt.info()[0] + 1
for n in (256, 2048, 4000):
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1).astype(np.float32)
    d_pts, d_p0, d_p1, d_cnt = ctx.upload(pts), ctx.malloc(n * 8), ctx.malloc(n * 8), ctx.malloc(32)
    args = (klt.criteria, klt.min_eig, klt.err_thresh, klt.fb_thresh)
    res[f"track_fb_dev_{n}_us"] = timed(lambda: klt.flow_fb_dev(n, d_pts, *args, d_p0, d_p1, d_cnt))
    res[f"track_host_{n}_us"] = timed(lambda: klt.track(pts))
    res[f"counts_{n}"] = list(klt.track(pts)[2])
    ctx.sync()
    for d in (d_pts, d_p0, d_p1, d_cnt):
        ctx.free(d)
klt.close()
print(json.dumps(res))
