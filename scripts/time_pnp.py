"""PnP-RANSAC timing (csrc/pnp_kernels.hip): per-call device time from HIP events after warm-up, median over REPS calls.
  host entry   sslam_pnp_ransac_host: upload + 8 launches + download (the drop-in's solve_pnp_ransac)
  device chain sslam_reproject_match_dev (SoA map) + sslam_pnp_ransac_dev on its output, nothing read back
  PnP alone    sslam_pnp_ransac_dev on a device-resident association
and the numpy restatement (oracle/pnp_ref.py) beside them for scale.  usage: python scripts/time_pnp.py [REPS]"""
import ctypes as C
import importlib
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import pnp_scenes as S
from oracle import pnp_ref as O

N = importlib.import_module("opencv-simpleslam_amd._native")
PN = importlib.import_module("opencv-simpleslam_amd.pnp")
L = importlib.import_module("opencv-simpleslam_amd.slam.core.landmark_utils")
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
lib = N.lib()
ctx = N.default_context()


def event():
    e = C.c_void_p()
    N.check(lib.sslam_timing_event_create(ctx.handle, C.byref(e)), "event")
    return e


def timed(fn, reps=REPS, warm=10):
    for _ in range(warm):
        fn()
    ctx.sync()
    a, b, ms = event(), event(), C.c_float()
    out = []
    for _ in range(reps):
        lib.sslam_event_record(ctx.handle, a)
        fn()
        lib.sslam_event_record(ctx.handle, b)
        ctx.sync()
        N.check(lib.sslam_event_elapsed_ms(a, b, C.byref(ms)), "elapsed")
        out.append(ms.value * 1e3)
    lib.sslam_event_destroy(a); lib.sslam_event_destroy(b)
    return float(np.median(out))


def map_scene(n, frac, seed):
    """A SoA map of 3n points of which n project onto keypoints of the frame (frac of them far off), the association's
    inputs: the map on the device, the frame's keypoints and descriptors, the predicted pose."""
    sc = S.make_scene(seed, 3 * n, 0.0, "kitti")
    rng = np.random.default_rng(seed)
    Q = 3 * n
    des_map = rng.standard_normal((Q, 128)).astype(np.float32)
    des_map /= np.linalg.norm(des_map, axis=1, keepdims=True)
    m = L.Map()
    ids = m.add_points(sc["pts3d"].astype(np.float64))
    for i, pid in enumerate(ids):
        m.points[pid].add_observation(0, i, des_map[i])
    pick = rng.choice(Q, n, replace=False)
    kp = sc["pts2d"][pick].copy()
    out = rng.choice(n, int(frac * n), replace=False)
    kp[out] += rng.uniform(3, 10, (len(out), 2)) * rng.choice([-1, 1], (len(out), 2))      # within the radius, off the model
    return m, sc, kp.astype(np.float32), des_map[pick].copy()


P = importlib.import_module("opencv-simpleslam_amd.slam.core.pnp_utils")
print(f"PnP-RANSAC per call, median of {REPS} after warm-up (HIP events), ransac_px {S.RANSAC_PX}, conf {S.CONF}, iters {S.ITERS}")
for n, frac in ((600, 0.3), (2000, 0.3)):
    # host entry (the drop-in)
    sc = S.make_scene(50 + n, n, frac, "kitti")
    ok, T, mask, info = PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS, use_guess=True)
    t_host = timed(lambda: PN.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, S.CONF, S.ITERS, use_guess=True))
    t0 = time.perf_counter()
    O.solve_pnp_ransac(sc["pts3d"], sc["pts2d"], sc["K"], S.RANSAC_PX, True, S.ITERS, S.CONF)
    t_np = (time.perf_counter() - t0) * 1e6
    print(f"n={n} outliers={frac}: host entry {t_host:.1f} us (inliers {info['inliers']}, samples {info['samples']}, "
          f"LM iterations {info['lm_iters']}); numpy restatement {t_np / 1e3:.1f} ms")
    # device chain: association + PnP on its device output
    m, msc, kp, des = map_scene(n, frac, 60 + n)
    K = msc["K"]; Tcw = msc["Tcw"]
    r = P.reproject_and_match_2d3d(m, K, Tcw, kp, des, 1241, 376, radius_px=12.0, max_l2=0.8, ctx=ctx)
    d_pos, d_cnt, d_desc = m.device_arrays(ctx)
    Q = len(m.soa()[0])
    scr = ctx.scratch["reproject"]
    Kd = np.ascontiguousarray(K, np.float64).reshape(9); Td = np.ascontiguousarray(Tcw, np.float64).reshape(16)
    d_T, d_info, d_n = ctx.malloc(128), ctx.malloc(16), ctx.malloc(4)
    Pp = N.ptr

    def assoc():
        N.check(lib.sslam_reproject_match_dev(ctx.handle, Q, Pp(d_pos), Pp(d_cnt), Pp(d_desc), Pp(Kd), Pp(Td), len(kp),
                                              Pp(scr["kp"]), Pp(scr["des"]), 1241, 376, 12.0, 0.8, Pp(scr["out"]), None,
                                              Pp(scr["info"])), "assoc")

    def pnp():
        PN.solve_pnp_ransac_dev(ctx, Q, scr["out"], d_pos, scr["kp"], K, d_T, d_info, S.RANSAC_PX, S.CONF, S.ITERS,
                                use_guess=True, n_out_dev=d_n)
    t_chain = timed(lambda: (assoc(), pnp()))
    t_pnp = timed(pnp)
    info4 = np.empty(4, np.int32); nn = np.empty(1, np.int32)
    ctx.d2h(info4, d_info); ctx.d2h(nn, d_n)
    print(f"n={n} outliers={frac}: device chain (association + PnP) {t_chain:.1f} us; PnP alone {t_pnp:.1f} us "
          f"({nn[0]} correspondences of {Q} map points, inliers {info4[0]}, samples {info4[1]}, LM iterations {info4[3]})")
    for d in (d_T, d_info, d_n):
        ctx.free(d)
