"""Device-side timing of the batched LightGlue entry on a CHAIN of frames, the frame pipeline's call shape: B pairs (f, f + 1) over
B + 1 device-resident frames, so that image 2p + 1 of pair p and image 2p of pair p + 1 name the same pointers (HIP events).
usage: time_lightglue_chain.py [N=2048] [B=8] [iters=20] [share=1]   (share: sslam_lightglue_debug_share_frames, where the library has it)"""
import importlib, sys
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import lg_inputs
N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
share = int(sys.argv[4]) if len(sys.argv) > 4 else 1
pkg = importlib.import_module("opencv-simpleslam_amd")
W = importlib.import_module("opencv-simpleslam_amd.weights")
LG = importlib.import_module("opencv-simpleslam_amd.lightglue").LightGlueHIP
ctx = pkg._native.default_context()
lg = LG(W.random_lightglue_state_dict(2, match_gain=4.0, match_bias=3.0), max_kpts=N, max_pairs=B)
if hasattr(lg, "debug_share_frames"):
    lg.debug_share_frames(bool(share))
frames = [(ctx.upload(xy), ctx.upload(d)) for xy, d in lg_inputs.make_chain(B + 1, N, seed=11)]
pairs = [(frames[b][0], frames[b][1], N, frames[b + 1][0], frames[b + 1][1], N) for b in range(B)]
ij = ctx.malloc(B * N * 8); sc = ctx.malloc(B * N * 4); info = ctx.malloc(B * 16)
for _ in range(2):
    lg.match_batch_dev(pairs, ij, sc, info, N)
ctx.sync()
ctx.timer_start()
for _ in range(iters):
    lg.match_batch_dev(pairs, ij, sc, info, N)
ms = ctx.timer_stop() / iters
inf = np.empty((B, 4), np.int32); ctx.d2h(inf, info)
what = lg.debug_share_info() if hasattr(lg, "debug_share_info") else "(no shared form in this library)"
print(f"N={N} B={B} chain, share={share} {what}: batch {ms:.4f} ms = {ms/B:.4f} ms/pair  matches {inf[:, 0].tolist()}")
