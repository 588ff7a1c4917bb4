"""Brute-force matcher timing, cross-check on: `sslam_bf_match_dev` (timing events around `reps` back-to-back enqueues on the
context stream, after a warm-up; the memset and both kernels of a call are inside) at the sizes of DESIGN.md's table, the
host entry (upload + call + download, wall clock) and the match count checked against the host entry."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
B = importlib.import_module("opencv-simpleslam_amd.bf_matcher")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ctx = N.default_context(0)
CASES = (("hamming", B.NORM_HAMMING, 2048, 32), ("hamming", B.NORM_HAMMING, 4000, 32), ("hamming", B.NORM_HAMMING, 4000, 61),
         ("l2", B.NORM_L2, 2048, 128), ("l2", B.NORM_L2, 4000, 128))
for what, norm, n, D in CASES:
    rng = np.random.default_rng(n + D)
    if norm == B.NORM_HAMMING:
        q = rng.integers(0, 256, (n, D), dtype=np.uint8); t = rng.integers(0, 256, (n, D), dtype=np.uint8)
        ops = 2.0 * n * n * ((D + 3) // 4)                 # xor, popcount-accumulate per 4-byte word
    else:
        q = rng.standard_normal((n, D)); t = rng.standard_normal((n, D))
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32); t = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
        ops = 2.0 * n * n * D                              # subtract, fma per element
    m = B.BFMatcher(norm, crossCheck=True, ctx=ctx)
    m.match_arrays(q, t)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); ij, dist = m.match_arrays(q, t); ts.append(time.perf_counter() - t0)
    d = [ctx.upload(q), ctx.upload(t)]
    o = [ctx.malloc(n * 8), ctx.malloc(n * 4), ctx.malloc(16)]
    run = lambda: m.match_dev(ctx, D, d[0], n, d[1], n, o[0], o[1], o[2])
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
    info = np.empty(4, np.int32); ctx.d2h(info, o[2])
    assert info.tolist() == [len(ij), n, n, 0]
    for p in d + o:
        ctx.free(p)
    us = float(np.median(per))
    print(f"{what} {n} x {n} x {D}{' B' if norm == B.NORM_HAMMING else ''}: device entry {us:.1f} us per call (min {min(per):.1f}, max {max(per):.1f} "
          f"over 5 x {reps}), {ops / us / 1e6:.2f} T lane-ops/s; host entry {np.median(ts) * 1e3:.3f} ms; {len(ij)} mutual pairs", flush=True)
