"""Essential-matrix RANSAC timing: the host entry (upload, normalise + head + per-chunk launches + tail, read-back) between
two timing events on the context stream, median of `reps` warm calls after a warm-up, and the wall clock of the same calls -
at n = 600 and 2048, for a clean scene (96 % planted: the budget collapses inside the first chunk) and a 30 % scene (the
loop runs about its full 1000 samples).  Beside it `sslam_homography_ransac_host` on the same point counts and shares in the
same process (planar scenes of tests/homography_scenes.py), the yardstick a reader already knows."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import essential_scenes as S, homography_scenes as HS
E = importlib.import_module("opencv-simpleslam_amd.essential")
H = importlib.import_module("opencv-simpleslam_amd.homography")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ctx = N.default_context(0)
e0, e1 = ctx.timing_event(), ctx.timing_event()


def timed(fn):
    for _ in range(5):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        ctx.record(e0); t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0); ctx.record(e1); ctx.sync()
        ev.append(ctx.elapsed_ms(e0, e1))
    return np.median(ev) * 1e3, np.median(wall) * 1e3


for n in (600, 2048):
    for frac in (0.96, 0.3):
        p1, p2, _ = S._draw(n, 700 + n, frac, "forward")
        fn = lambda: E.find_essential_mat_ransac(p1, p2, S.K, S.PROB, S.THRESH, ctx=ctx)
        got = fn()[2]
        ev, wall = timed(fn)
        print(f"E n={n}, {int(frac * 100)} % inliers: {ev:.1f} us between events ({wall:.3f} ms wall), {got['iterations']} iterations, "
              f"{got['inliers']} inliers", flush=True)
        q1, q2 = HS._draw(n, 900 + n, frac, 0.2, "plane")
        fh = lambda: H.find_homography_ransac(q1, q2, HS.THRESH, ctx=ctx)
        goth = fh()[2]
        ev, wall = timed(fh)
        print(f"H n={n}, {int(frac * 100)} % inliers: {ev:.1f} us between events ({wall:.3f} ms wall), {goth['iterations']} iterations, "
              f"{goth['inliers']} inliers", flush=True)
