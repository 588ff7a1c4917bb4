"""Generate tests/golden/reproject_hamming.npz from the REFERENCE's own `slam.core.pnp_utils.reproject_and_match_2d3d`
(pnp_utils.py:224-304) on binary descriptors.

    python tests/golden/make_reproject_hamming_golden.py <directory of the reference checkout>

`pnp_utils` imports cv2 at module scope and its Hamming branch calls `cv2.norm(a, b, cv2.NORM_HAMMING)` (:97); cv2 is
not installed where this runs, so a stub of ours stands in: NORM_HAMMING = 6 and norm(a, b, t) = popcount(a ^ b), which
is what OpenCV defines for that norm type.  Everything else the function touches is numpy and scipy.spatial.cKDTree.
The scenes come from the seeded generator tests/reproject_hamming_scenes.py; the .npz holds the reference's outputs
plus a digest of the generated inputs (data only), so the tests notice if the generator ever drifts.

Hamming distances are integers: where two free keypoints tie at an ACCEPTED minimum, the reference takes the one
cKDTree's traversal meets first, and the fixture would pin SciPy's tree layout.  So this generator asserts that the
restatement (tests/reproject_hamming_ref.py) counts 0 such decisions on every scene - a scene that has one gets
another seed - and that the restatement then equals the reference exactly."""
import sys
import types
from pathlib import Path

import numpy as np

if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
cv2 = types.ModuleType("cv2")
cv2.NORM_HAMMING = 6


def _norm(a, b, norm_type):
    assert norm_type == cv2.NORM_HAMMING
    return float(_POP[np.asarray(a, np.uint8) ^ np.asarray(b, np.uint8)].sum())


cv2.norm = _norm
sys.modules["cv2"] = cv2
from slam.core.pnp_utils import reproject_and_match_2d3d          # noqa: E402
import reproject_hamming_ref as HR                                # noqa: E402
import reproject_hamming_scenes as HS                             # noqa: E402


def main(out=Path(__file__).resolve().parent / "reproject_hamming.npz"):
    blob = {"n_cases": len(HS.CASES)}
    for c, args in enumerate(HS.CASES):
        sc = HS.make_case(*args)
        m = reproject_and_match_2d3d(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"], sc["H"],
                                     radius_px=sc["radius"], max_hamm=sc["max_hamm"])
        p3, p2, kp, mp, ties, _ = HR.reproject_and_match_hamming(sc["wmap"], sc["K"], sc["Tcw"], sc["kp"], sc["des"], sc["W"],
                                                                 sc["H"], sc["radius"], sc["max_hamm"])
        print(f"case {c}: {len(m.kp_indices)} matches of {len(sc['wmap'].points)} points / {len(sc['kp'])} keypoints, "
              f"B = {sc['B']}, tied accepted decisions: {ties}")
        assert ties == 0, f"case {c}: an accepted decision is tied; the fixture would depend on cKDTree's order - change the seed"
        assert list(m.kp_indices) == list(kp) and list(m.mp_ids) == list(mp), f"case {c}: restatement != reference"
        assert np.array_equal(m.pts3d, p3) and np.array_equal(m.pts2d, p2)
        blob[f"digest{c}"] = sc["digest"]
        blob[f"kp{c}"] = np.asarray(m.kp_indices, np.int64)
        blob[f"mp{c}"] = np.asarray(m.mp_ids, np.int64)
        blob[f"pts3d{c}"] = m.pts3d
        blob[f"pts2d{c}"] = m.pts2d
    np.savez_compressed(out, **blob)


if __name__ == "__main__":
    main()
