"""Semi-global stereo timing: `sslam_sgbm_compute_dev` (timing events around `reps` back-to-back enqueues on the context stream
after a warm-up, five windows; every kernel of a compute is inside, nothing is read back) on a 1241 x 376 grey pair, with the
prototype's configuration (D = 32, blockSize 11) and with D = 128, blockSize 5; the host entry (two uploads + compute + download,
wall clock) beside it.  The device result is checked against the host entry's.  There is no CPU figure: the project has no
other SGBM to run.  `time_sgbm.py [REPS [D BLOCKSIZE]]`: a window of the default 400 computes lasts about a second; with D and
BLOCKSIZE only that configuration runs, so that under `rocprofv3 --kernel-trace --stats` with a small REPS the per-kernel
split belongs to one configuration (a run of its own).  Per kernel the bytes it must move are printed with the time they take at the HBM rate SURVEY.md 8(d)
measured (6.29 TB/s)."""
import importlib, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
S = importlib.import_module("opencv-simpleslam_amd.stereo")
N = importlib.import_module("opencv-simpleslam_amd._native")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
configs = [(int(sys.argv[2]), int(sys.argv[3]))] if len(sys.argv) > 3 else [(32, 11), (128, 5)]
HBM = 6.29e12
H, W = 376, 1241
ctx = N.default_context(0)


def textured_pair(shift, seed):
    """a smooth texture with a little noise, the right image the left shifted by `shift` columns"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W + shift]
    T = np.clip(120 + 60 * np.sin(xx / 5.0 + yy / 9.0) + 30 * np.cos(xx / 2.3 - yy / 3.1) + rng.integers(-6, 7, (H, W + shift)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(T[:, :W]), np.ascontiguousarray(T[:, shift:shift + W])


for D, bs in configs:
    left, right = textured_pair(17, D)
    sg = S.StereoSGBM_create(0, D, bs, 8 * bs * bs, 32 * bs * bs, ctx=ctx)
    want = sg.compute(left, right)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); sg.compute(left, right); ts.append(time.perf_counter() - t0)
    d = [ctx.upload(left), ctx.upload(right), ctx.malloc(H * W * 2)]
    run = lambda: sg.compute_dev(d[0], d[1], H, W, d[2])
    for _ in range(min(5, reps)):
        run()
    ctx.sync()
    e0, e1 = ctx.timing_event(), ctx.timing_event()
    per = []
    for _ in range(5):
        ctx.record(e0)
        for _ in range(reps):
            run()
        ctx.record(e1); ctx.sync()
        per.append(ctx.elapsed_ms(e0, e1) / reps)
    got = np.empty((H, W), np.int16); ctx.d2h(got, d[2])
    assert np.array_equal(got, want)
    for p in d:
        ctx.free(p)
    px, vol = H * W, H * (W - D) * D * 2
    floors = {"sg_prefilter_kernel": 4 * px, "sg_rowsum_kernel": 4 * px + vol, "sg_colsum_kernel": 2 * vol, "sg_path_kernel (first)": 2 * vol,
              "sg_path_kernel (each of four more)": 3 * vol, "sg_select_kernel": vol + 6 * H * (W - D), "sg_right_kernel": 4 * H * (W - D) + 2 * px,
              "sg_check_kernel": 6 * px, "sg_median_kernel": 4 * px}
    total = sum(v * (4 if "four" in k else 1) for k, v in floors.items())
    print(f"sgbm {W} x {H}, D {D}, blockSize {bs}: device entry {np.median(per):.3f} ms per compute (min {min(per):.3f}, max {max(per):.3f} over 5 x {reps}), "
          f"12 launches, cost volume {vol / 1e6:.1f} MB, instance {S.workspace_bytes(W, H, D, D) / 1e6:.1f} MB; host entry {np.median(ts) * 1e3:.3f} ms "
          f"(min {min(ts) * 1e3:.3f}); valid {float((want[:, D:] >= 0).mean()):.3f}", flush=True)
    for k, v in floors.items():
        print(f"    floor {k}: {v / 1e6:.1f} MB = {v / HBM * 1e6:.1f} us at 6.29 TB/s")
    print(f"    floor of a compute: {total / 1e6:.1f} MB = {total / HBM * 1e6:.1f} us", flush=True)
