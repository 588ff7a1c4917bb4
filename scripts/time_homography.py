"""Homography RANSAC timing: the host entry (upload, head + per-chunk launches + tail, read-back) between two timing events
on the context stream, median of `reps` calls after a warm-up, the wall clock of the same calls, and the numpy restatement
on the same box - at n = 600 and 4096, for a planted scene at 80 % inliers (the budget collapses to about ten iterations)
and at 35 % (about 350 iterations: all three chunks)."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import homography_ref as R, homography_scenes as S
H = importlib.import_module("opencv-simpleslam_amd.homography")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
ctx = N.default_context(0)
e0, e1 = ctx.timing_event(), ctx.timing_event()


def timed(fn):
    for _ in range(10):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        ctx.record(e0); t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0); ctx.record(e1); ctx.sync()
        ev.append(ctx.elapsed_ms(e0, e1))
    return np.median(ev) * 1e3, np.median(wall) * 1e3


for n in (600, 4096):
    for frac in (0.8, 0.35):
        p1, p2 = S._draw(n, 900 + n, frac, 0.2, "plane")
        fn = lambda: H.find_homography_ransac(p1, p2, S.THRESH, ctx=ctx)
        got = fn()[2]
        ev, wall = timed(fn)
        t0 = time.perf_counter(); ref = R.find_homography_ransac(p1, p2, S.THRESH)[2]; tr = time.perf_counter() - t0
        print(f"n={n}, {int(frac * 100)} % inliers: {ev:.1f} us between events ({wall:.3f} ms wall), {got['iterations']} iterations, "
              f"{got['inliers']} inliers (restatement {ref['iterations']} / {ref['inliers']}), numpy restatement {tr * 1e3:.1f} ms")
