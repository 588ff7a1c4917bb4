"""Thumbnail timing: `sslam_thumb_encode_dev` (timing events around `reps` back-to-back enqueues on the context stream after a
warm-up, five windows; all eight kernels of an encode are inside, nothing is read back) on a 1241 x 376 frame -> 640 x 360 at
quality 70, colour and grey; the host entry (upload + encode + count + stream download, wall clock); and beside them Pillow's
`resize` + `save(quality=70)` of the same frame on this machine's CPU, the stated stand-in for the `cv2.resize` + `cv2.imencode`
it replaces (cv2 is not installed here).  The stream is checked against the host entry's.  `time_thumb.py REPS`; under
`rocprofv3 --kernel-trace --stats` with a small REPS it gives the per-kernel split (a run of its own)."""
import importlib, io, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import thumb_ref
T = importlib.import_module("opencv-simpleslam_amd.thumbnail")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
H, W, WH, Q = 376, 1241, (640, 360), 70
ctx = N.default_context(0)
th = T.Thumbnailer((W, H), WH, Q, ctx=ctx)
for c in (3, 1):
    img = thumb_ref.natural(H, W, c, seed=4)
    want = th.encode(img)
    ts = []
    for _ in range(20):
        t0 = time.perf_counter(); th.encode(img); ts.append(time.perf_counter() - t0)
    d = [ctx.upload(img), ctx.malloc(th.capacity), ctx.malloc(4)]
    run = lambda: th.encode_dev(d[0], H, W, c, d[1], d[2])
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
    n = np.zeros(1, np.int32); ctx.d2h(n, d[2])
    got = np.empty(int(n[0]), np.uint8); ctx.d2h(got, d[1])
    assert got.tobytes() == want
    for p in d:
        ctx.free(p)
    cpu = None
    try:
        from PIL import Image
        rgb = img if c == 1 else np.ascontiguousarray(img[:, :, ::-1])
        tc = []
        for _ in range(20):
            t0 = time.perf_counter()
            buf = io.BytesIO(); Image.fromarray(rgb).resize(WH, Image.BILINEAR).save(buf, "JPEG", quality=Q); tc.append(time.perf_counter() - t0)
        cpu = f"Pillow resize + save on the CPU {np.median(tc) * 1e3:.3f} ms ({len(buf.getvalue())} bytes)"
    except ImportError:
        cpu = "Pillow is not installed: no CPU figure"
    g = T.geometry(*WH, c)
    print(f"thumbnail {W} x {H} x {c} -> {WH[0]} x {WH[1]}, quality {Q}: device entry {np.median(per):.1f} us per encode (min {min(per):.1f}, max "
          f"{max(per):.1f} over 5 x {reps}), 8 launches, {g['blocks']} blocks, {len(want)} bytes of {th.capacity}; host entry "
          f"{np.median(ts) * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}); {cpu}", flush=True)
th.close()
