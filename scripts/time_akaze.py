"""AKAZE timing: `sslam_akaze_detect_dev` (timing events around `reps` back-to-back enqueues on the context stream after a
warm-up, five windows; the memset and every kernel of a frame are inside, nothing is read back) on a structured 1241 x 376 frame
with cv2's defaults, the host entry (upload + call + download, wall clock), the keypoint count checked against the host entry,
the launch count of a frame from the level table, and the bytes the diffusion steps move at 12 bytes per pixel per step (two
reads, one write) split by form.  `time_akaze.py REPS`; under `rocprofv3 --kernel-trace --stats` with a small REPS it gives
the per-kernel split (a run of its own)."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import orb_scenes
A = importlib.import_module("opencv-simpleslam_amd.akaze")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
H, W = 376, 1241
ctx = N.default_context(0)
img = orb_scenes.mosaic(H, W, seed=11, block=9)
o = A.AKAZE_create(max_h=H, max_w=W, ctx=ctx)
xy, aux, lvl, desc = o.detect_arrays(img)
ts = []
for _ in range(10):
    t0 = time.perf_counter(); o.detect_arrays(img); ts.append(time.perf_counter() - t0)
cap = o.capacity
d = [ctx.upload(img), ctx.malloc(cap * 8), ctx.malloc(cap * 12), ctx.malloc(cap * 8), ctx.malloc(cap * 61), ctx.malloc(4)]
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
levels = [o.level_info(i) for i in range(o.level_info(0)["levels"])]
launches = 1 + 4 + 3                                        # grey, two blurs of two passes, the three kcontrast kernels
step_launches = wg_steps = 0
bytes_launch = bytes_wg = 0
for i, L in enumerate(levels):
    if i > 0:
        launches += int(L["octave"] != levels[i - 1]["octave"])                     # the halving
        if L["one_workgroup"]:
            launches += 1; wg_steps += L["fed_steps"]; bytes_wg += 12 * L["w"] * L["h"] * L["fed_steps"]
        else:
            launches += 3 + L["fed_steps"]; step_launches += L["fed_steps"]; bytes_launch += 12 * L["w"] * L["h"] * L["fed_steps"]
    launches += 4                                            # the response: a blur of two passes, the derivatives, the determinant
launches += 5
per_level = [int((lvl[:, 1] == i).sum()) for i in range(len(levels))]
for p in d:
    ctx.free(p)
o.close()
print(f"akaze {W} x {H}, defaults: device entry {np.median(per):.1f} us per frame (min {min(per):.1f}, max {max(per):.1f} over 5 x {reps}); "
      f"host entry {np.median(ts) * 1e3:.3f} ms; {counts[0]} candidates, {counts[1]} keypoints before the quota, {len(xy)} rows, per level {per_level}; "
      f"{len(levels)} levels, {launches} launches and a memset, of them {step_launches} diffusion steps as launches ({bytes_launch / 1e6:.1f} MB at 12 B "
      f"per pixel per step) and {wg_steps} steps inside one-workgroup launches ({bytes_wg / 1e6:.1f} MB equivalent, in LDS); capacity {cap} rows", flush=True)
