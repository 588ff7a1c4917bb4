"""sha1 of the aggregation's stage buffers (debug_read 10..18: g1, rnorm, g2..g4, pre2..pre4, s8) and of the score map (0), with
the keypoints and descriptors, on the frames of tests/test_aliked_pre_tail_gpu.py and of tests/test_aliked_gate_agg_gpu.py:
    python scripts/hash_aliked_gate_agg.py [TREE]
runs the library of TREE (default: this tree) on this tree's frames.  Run it on the parent's tree and on the head's and diff the
two printouts when a change to the gates, the pre-aggregation planes or the aggregate kernel claims bit-identical results."""
import hashlib, importlib, sys
from pathlib import Path
import numpy as np
HERE = Path(__file__).resolve().parent.parent
TREE = Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else HERE
sys.path.insert(0, str(HERE / "tests"))
import frames                                            # noqa: E402
import test_aliked_pre_tail_gpu as T                     # noqa: E402  (the frames only; its oracle is not called)
import test_aliked_gate_agg_gpu as G                     # noqa: E402  (the frame sizes only)
sys.path.insert(0, str(TREE))
W = importlib.import_module("opencv-simpleslam_amd.weights")
AL = importlib.import_module("opencv-simpleslam_amd.aliked").AlikedHIP
assert Path(importlib.import_module("opencv-simpleslam_amd")._native.LIB_PATH).resolve().is_relative_to(TREE), "the library is not TREE's"
sd = W.random_aliked_state_dict(0)
cases = [(name, T._image(name)) for name in T.CASES] + [("noise_%dx%d" % hw, frames.noise_frame(0, h=hw[0], w=hw[1])) for hw in G.FRAMES]
sha = lambda a: hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]      # noqa: E731
for name, image in cases:
    al = AL(sd, max_num_keypoints=256, max_h=image.shape[0], max_w=image.shape[1])
    xy, desc = al.extract(image, 256)
    d = al.debug_read(2, (8,), np.int32)
    h, w, Hp, Wp = (int(v) for v in d[:4])
    parts = ["score " + sha(al.debug_read(0, (h, w))), "g1 " + sha(al.debug_read(10, (Hp, Wp, 32))), "rnorm " + sha(al.debug_read(11, (Hp, Wp)))]
    for which, label, div, ch in ((12, "g2", 2, 32), (13, "g3", 8, 32), (14, "g4", 32, 32), (15, "pre2", 2, 13), (16, "pre3", 8, 13),
                                  (17, "pre4", 32, 13), (18, "s8", 1, 8)):
        parts.append(label + " " + sha(al.debug_read(which, (ch, Hp // div, Wp // div))))
    al.close()
    print(f"{name:24s} {h:4d} x {w:4d}  " + "  ".join(parts) + f"  keypoints+descriptors {hashlib.sha1(xy.tobytes() + desc.tobytes()).hexdigest()[:12]} n={len(xy)}")
