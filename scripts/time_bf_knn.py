"""k-NN / ratio matcher timing: `sslam_bf_ratio_match_dev` and `sslam_bf_knn_match_dev` at k = 8 (timing events around `reps`
back-to-back enqueues on the context stream, after a warm-up, five windows; both kernels of a call are inside) at the sizes of
DESIGN.md's table, and IN THE SAME RUN `sslam_bf_match_dev` with cross-check off and on at those shapes - the yardstick: it
performs the same distance arithmetic.  Prints the ratio of every variant to `match` (cross-check off), the splits the plan
chose, and checks the kept count against the host entry."""
import importlib, sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
B = importlib.import_module("opencv-simpleslam_amd.bf_matcher")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ctx = N.default_context(0)
CASES = (("hamming", B.NORM_HAMMING, 2048, 32), ("hamming", B.NORM_HAMMING, 4000, 61), ("l2", B.NORM_L2, 2048, 128), ("l2", B.NORM_L2, 4000, 128))


def timed(run):
    for _ in range(20):
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
    return float(np.median(per)), min(per), max(per)


for what, norm, n, D in CASES:
    rng = np.random.default_rng(n + D)
    if norm == B.NORM_HAMMING:
        q = rng.integers(0, 256, (n, D), dtype=np.uint8); t = rng.integers(0, 256, (n, D), dtype=np.uint8)
    else:
        q = rng.standard_normal((n, D)); t = rng.standard_normal((n, D))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32); t = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
    ratio = 0.95
    kept_host = len(B.BFMatcher(norm, ctx=ctx).ratio_match_arrays(q, t, ratio)[0])
    d = [ctx.upload(q), ctx.upload(t)]
    o = [ctx.malloc(n * 8 * 4), ctx.malloc(n * 8 * 4), ctx.malloc(n * 4), ctx.malloc(16)]       # the largest outputs: idx / dist [n, 8]
    off, on = B.BFMatcher(norm, crossCheck=False), B.BFMatcher(norm, crossCheck=True)
    info = np.empty(4, np.int32)
    rows = []
    variants = (("match, cross-check off", lambda: off.match_dev(ctx, D, d[0], n, d[1], n, o[0], o[1], o[3])),
                ("match, cross-check on", lambda: on.match_dev(ctx, D, d[0], n, d[1], n, o[0], o[1], o[3])),
                ("ratio_match_dev (k = 2)", lambda: off.ratio_match_dev(ctx, D, d[0], n, d[1], n, o[0], o[1], o[3], ratio=ratio)),
                ("knn_match_dev k = 8", lambda: off.knn_match_dev(ctx, D, d[0], n, d[1], n, 8, o[0], o[1], o[2], o[3])))
    for name, run in variants:
        us, lo, hi = timed(run)
        ctx.d2h(info, o[3])
        rows.append((name, us, lo, hi, info.tolist()))
    for p in d + o:
        ctx.free(p)
    assert rows[2][4] == [kept_host, n, n, 0], (rows[2][4], kept_host)
    assert rows[3][4][:3] == [n, n, 8]
    base = rows[0][1]
    print(f"{what} {n} x {n} x {D}{' B' if norm == B.NORM_HAMMING else ''}:", flush=True)
    for name, us, lo, hi, inf in rows:
        extra = f", {inf[0]} kept at ratio {ratio}" if name.startswith("ratio") else f", {inf[3]} splits" if name.startswith("knn") else f", {inf[0]} pairs"
        print(f"    {name:26s} {us:8.1f} us per call (min {lo:.1f}, max {hi:.1f} over 5 x {reps}), {us / base:5.2f} x match{extra}", flush=True)
