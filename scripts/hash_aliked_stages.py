"""sha1 of the padded image (debug_read 7) and the score map (debug_read 0) on the frames of tests/test_aliked_pre_tail_gpu.py:
    python scripts/hash_aliked_stages.py [TREE]
runs the library of TREE (default: this tree) on this tree's frames.  Run it on the parent's tree and on the head's and diff the
two printouts when a change to the pre-processing or the score tail claims bit-identical results."""
import hashlib, importlib, sys
from pathlib import Path
import numpy as np
HERE = Path(__file__).resolve().parent.parent
TREE = Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else HERE
sys.path.insert(0, str(HERE / "tests"))
import test_aliked_pre_tail_gpu as T                     # noqa: E402  (the frames only; its oracle is not called)
sys.path.insert(0, str(TREE))
W = importlib.import_module("opencv-simpleslam_amd.weights")
AL = importlib.import_module("opencv-simpleslam_amd.aliked").AlikedHIP
sd = W.random_aliked_state_dict(0)
for name, (H, Wd, C) in T.CASES.items():
    al = AL(sd, max_num_keypoints=256, max_h=H, max_w=Wd)
    xy, desc = al.extract(T._image(name), 256)
    d = al.debug_read(2, (8,), np.int32)
    h, w, Hp, Wp = (int(v) for v in d[:4])
    img, score = al.debug_read(7, (3, Hp, Wp)), al.debug_read(0, (h, w))
    al.close()
    out = hashlib.sha1(xy.tobytes() + desc.tobytes()).hexdigest()
    print(f"{name:20s} {h:4d} x {w:4d}  img {hashlib.sha1(img.tobytes()).hexdigest()}  score {hashlib.sha1(score.tobytes()).hexdigest()}  "
          f"keypoints+descriptors {out[:16]} n={len(xy)}")
