"""2D-3D association on the device at the C2 size (5000 landmarks x 2048 keypoints), per call by HIP events: the Hamming
form (`sslam_reproject_match_hamming_dev`, 32-byte rows) and the float form (`sslam_reproject_match_dev`, 128 floats) on
scenes of the same geometry, alternating call by call.  A call = the K / Tcw uploads, the info memset, the pair kernel and
the serial greedy pass; inputs are device resident.  Prints the byte bound of each pair kernel beside the time; the split
between the two kernels comes from a profiler run of this script (rocprofv3 --kernel-trace --stats).

    python scripts/time_reproject_hamming.py [calls per form, default 300]"""
import importlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import reproject_hamming_scenes as HS                              # noqa: E402
import reproject_scenes as RS                                      # noqa: E402

native = importlib.import_module("opencv-simpleslam_amd._native")
L = importlib.import_module("opencv-simpleslam_amd.slam.core.landmark_utils")
Q, N, B, RADIUS = 5000, 2048, 32, 12.0
HBM = 6.29e12                                                      # bytes/s, measured float4 copy on the MI355X
calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
ctx = native.default_context()
lib, P = native.lib(), native.ptr

hs = HS.make_case(11, Q, N, RADIUS, B, 64)
fs = RS.make_case(11, Q, N, RADIUS, 0.8, False)
hm, fm = L.Map.from_reference(hs["wmap"]), L.Map.from_reference(fs["wmap"])
h_pos, h_cnt, h_rows = hm.device_arrays_binary(ctx)
f_pos, f_cnt, f_desc = fm.device_arrays(ctx)
h_kp, h_des = ctx.upload(hs["kp"]), ctx.upload(hs["des"])
f_kp, f_des = ctx.upload(fs["kp"]), ctx.upload(fs["des"])
d_out, d_info = ctx.malloc(4 * Q), ctx.malloc(16)
Kd = np.ascontiguousarray(hs["K"], np.float64).reshape(9)
hT, fT = (np.ascontiguousarray(s["Tcw"], np.float64).reshape(16) for s in (hs, fs))


def hamming():
    native.check(lib.sslam_reproject_match_hamming_dev(ctx.handle, Q, P(h_pos), P(h_cnt), P(h_rows), P(Kd), P(hT), N, P(h_kp),
                                                       P(h_des), B, HS.W, HS.H, RADIUS, 64.0, P(d_out), None, P(d_info), None))


def floats():
    native.check(lib.sslam_reproject_match_dev(ctx.handle, Q, P(f_pos), P(f_cnt), P(f_desc), P(Kd), P(fT), N, P(f_kp), P(f_des),
                                               RS.W, RS.H, RADIUS, 0.8, P(d_out), None, P(d_info)))


def info():
    ctx.sync()
    i4 = np.empty(4, np.int32)
    ctx.d2h(i4, d_info)
    return [int(x) for x in i4]


res = {}
for name, fn in (("hamming", hamming), ("float", floats)):
    for _ in range(20):
        fn()
    res[name] = {"info_matches_overflow_candidates": info()[:3], "ms": []}
for _ in range(calls):                                             # alternating: both forms see the same machine
    for name, fn in (("hamming", hamming), ("float", floats)):
        ctx.timer_start(); fn(); res[name]["ms"].append(ctx.timer_stop())
for name, cand_rows, row_bytes, frame_bytes in (("hamming", hm.soa_binary()[2], 64, N * B), ("float", fm.soa()[2], 512, N * 128 * 4)):
    ms = np.array(res[name].pop("ms"))
    bound_bytes = Q * 6 * row_bytes + frame_bytes                  # every stored row slot once + the frame rows once
    res[name].update(calls=calls, median_ms=round(float(np.median(ms)), 4), p10_ms=round(float(np.percentile(ms, 10)), 4),
                     p90_ms=round(float(np.percentile(ms, 90)), 4), pair_kernel_bound_bytes=bound_bytes,
                     pair_kernel_bound_us=round(bound_bytes / HBM * 1e6, 3), stored_rows=int(cand_rows.sum()))
print(json.dumps({"Q": Q, "N": N, "B": B, "radius_px": RADIUS, **res}))
