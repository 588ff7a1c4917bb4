"""`sslam_homography_ransac_host` against the numpy restatement (tests/homography_ref.py) on every scene of
tests/homography_scenes.py.

The winning sample, the iteration count, the inlier count and the mask must be IDENTICAL.  That can only be asked of inputs
that are not coin tosses, so every scene was accepted (homography_scenes.make_scene) only after its LAPACK and Jacobi variants
agreed on all four and no match's error under the winning model lay within 1e-3 relative of the squared threshold; a draw
that failed was drawn again with another seed.  Each test asserts both again, and that the scene reaches its branch.

H is compared on H / H[2,2], relative to max |H|.  The tolerance is measured, not guessed: `H_FLOOR` is the largest
disagreement over all scenes between the restatement with LAPACK and the same restatement with the float64 ports of the
kernel's Jacobi and elimination - 1.95e-9 on the build machine, on the five-match scene (four exact constraints and one more:
the least-squares problem of the polish is nearly singular there; every other scene is below 8e-11).
`test_the_measured_floor_still_holds` re-measures it on the CPU part of every GPU run.  The GPU may differ from the
restatement by 100 x that, 2e-7, and in no case by more than 1e-6.
"""
import numpy as np
import pytest

import homography_ref as HR
import homography_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu

H_FLOOR = 2e-9
H_BAR = 100 * H_FLOOR
assert H_BAR <= 1e-6


@pytest.fixture(scope="module")
def scenes():
    return S.all_scenes()


@pytest.fixture(scope="module")
def hg():
    return load_pkg("homography")


NAMES = ["four_4", "four_degenerate_4", "five_5", "plane_63", "plane_64", "plane_65", "plane_255", "plane_1023", "plane_1024",
         "plane_1025", "plane_16384", "sparse_600", "clean_600", "mirror_400", "line_50"]


def _h_err(H, Href):
    return float(np.abs(H / H[2, 2] - Href / Href[2, 2]).max() / np.abs(Href / Href[2, 2]).max())


def test_the_scene_list_is_complete(scenes):
    assert sorted(scenes) == sorted(NAMES)


def test_the_measured_floor_still_holds(scenes):
    worst = 0.0
    for s in scenes.values():
        ok, rl, rj = S.not_a_coin_toss(s["pts1"], s["pts2"], s["thresh"], s["max_iters"])
        assert ok, s["name"]
        if rl[0] is not None:
            worst = max(worst, _h_err(rj[0], rl[0]))
    print(f"LAPACK against the Jacobi / elimination ports, all scenes: H {worst:.3e} of max |H| (floor {H_FLOOR:.1e})")
    assert worst <= H_FLOOR


def _assert_equal(name, got, ref):
    H, mask, info = got
    Hr, mask_r, info_r = ref
    e = _h_err(H, Hr) if H is not None and Hr is not None else 0.0
    print(f"{name}: sample {info['sample']} ({info_r['sample']}), iterations {info['iterations']} ({info_r['iterations']}), "
          f"inliers {info['inliers']} ({info_r['inliers']}), H {e:.3e} (bar {H_BAR:.1e})")
    assert (H is None) == (Hr is None) and (mask is None) == (mask_r is None)
    assert (info["sample"], info["iterations"], info["inliers"]) == (info_r["sample"], info_r["iterations"], info_r["inliers"])
    if Hr is not None:
        assert H.shape == (3, 3) and mask.dtype == np.bool_ and mask.shape == mask_r.shape
        np.testing.assert_array_equal(mask, mask_r)
        assert H[2, 2] == 1.0 and e <= H_BAR


@pytest.mark.parametrize("name", NAMES)
def test_homography_equals_the_restatement(hg, gpu_ctx, scenes, name):
    s = scenes[name]
    S.assert_reaches(s)
    for ref in (s["ref"], s["ref_jacobi"]):               # accepted because the two agree and nothing sits on the threshold
        i = ref[2]
        assert (i["sample"], i["iterations"], i["inliers"]) == tuple(s["ref"][2][k] for k in ("sample", "iterations", "inliers"))
        if i["err"] is not None:
            assert (np.abs(i["err"].astype(np.float64) - i["t"]) > S.MARGIN_REL * i["t"]).all()
    got = hg.find_homography_ransac(s["pts1"], s["pts2"], s["thresh"], max_iters=s["max_iters"], ctx=gpu_ctx)
    _assert_equal(name, got, s["ref"])
    # a second call: bit for bit
    again = hg.find_homography_ransac(s["pts1"], s["pts2"], s["thresh"], max_iters=s["max_iters"], ctx=gpu_ctx)
    assert again[2] == got[2]
    if got[0] is not None:
        assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()


def test_defaulted_parameters(hg, gpu_ctx, scenes):
    """thresh <= 0 is 3, a confidence outside (0, 1) is 0.995, max_iters is clamped to [1, 2000]"""
    s = scenes["plane_255"]
    want = hg.find_homography_ransac(s["pts1"], s["pts2"], 3.0, 0.995, 2000, ctx=gpu_ctx)
    for args in ((0.0, 0.995, 2000), (-1.0, 1.0, 2000), (3.0, 0.0, 5000), (3.0, 7.0, 2000)):
        got = hg.find_homography_ransac(s["pts1"], s["pts2"], *args, ctx=gpu_ctx)
        assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]), args
    one = hg.find_homography_ransac(s["pts1"], s["pts2"], s["thresh"], max_iters=0, ctx=gpu_ctx)
    ref = HR.find_homography_ransac(s["pts1"], s["pts2"], s["thresh"], max_iters=0)
    assert one[2]["iterations"] == ref[2]["iterations"] == 1 and one[2]["inliers"] == ref[2]["inliers"]


def test_a_slab_driven_large_then_small(hg, native, scenes):
    """one fresh context: the largest scene sizes its scratch slab, the small ones then run inside it"""
    ctx = native.Context(0)
    try:
        for name in ("plane_16384", "plane_63", "four_4", "sparse_600", "line_50", "plane_1025"):
            s = scenes[name]
            _assert_equal(name, hg.find_homography_ransac(s["pts1"], s["pts2"], s["thresh"], max_iters=s["max_iters"], ctx=ctx), s["ref"])
    finally:
        ctx.close()


def test_bad_arguments_are_errors(hg, gpu_ctx, native, scenes):
    s = scenes["plane_63"]
    with pytest.raises(ValueError):
        hg.find_homography_ransac(s["pts1"], s["pts2"][:-1], ctx=gpu_ctx)
    with pytest.raises(native.NativeError, match="at least 4"):
        hg.find_homography_ransac(s["pts1"][:3], s["pts2"][:3], ctx=gpu_ctx)
    big = np.zeros((16385, 2), np.float32)
    with pytest.raises(native.NativeError, match="16384"):
        hg.find_homography_ransac(big, big, ctx=gpu_ctx)
