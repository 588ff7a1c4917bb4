"""`optical_flow.KLTTracker` as the KLT front end of the reference's tracking loop (slam/monocular/main4.py:395-433): over
three pushed frames it returns, for both consecutive pairs, exactly what that code computes when its two cv2 calls are the
restatement (tests/klt_ref.py: `track_forward_backward` is that code) - the same kept pairs in the same order, the same five
counters; the pyramid a frame keeps between its two roles equals a rebuilt one; a frame that is already on the device is read
there."""
import numpy as np
import pytest

import klt_ref as R
import klt_scenes as S
from conftest import load_pkg

pytestmark = pytest.mark.gpu
H, W = 120, 160
N = 300


@pytest.fixture(scope="module")
def O(gpu_ctx):
    return load_pkg("optical_flow")


@pytest.fixture(scope="module")
def frames():
    out = [S.frame(i, H, W, 3) for i in range(3)]                          # BGR with distinct planes: the grey conversion is in the path
    for f in out:
        f.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def points():
    return S.points(H, W, N)


@pytest.fixture(scope="module")
def expected(frames, points):
    """main4's body on pairs (0, 1) and (1, 2), computed once"""
    pyr = [R.Pyramid(f) for f in frames]
    return [R.track_forward_backward(pyr[i], pyr[i + 1], points, **S.MAIN4) for i in range(2)]


def _same_pairs(got, want, what):
    for g, w, part in ((got[0], want[0], "pts0"), (got[1], want[1], "pts1")):
        assert g.shape == w.shape and g.dtype == np.float32, (what, part, g.shape, w.shape)
        np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32), err_msg=f"{what}: {part}")
    assert tuple(got[2]) == tuple(want[2]), (what, got[2], want[2])


def test_three_frames_give_main4s_pairs_and_counters(O, gpu_ctx, frames, points, expected):
    klt = O.KLTTracker((W, H), ctx=gpu_ctx)
    try:
        klt.push(frames[0])
        with pytest.raises(RuntimeError, match="two pushed frames"):
            klt.track(points)
        klt.push(frames[1])
        first = klt.track(points.reshape(-1, 1, 2))                        # main4 hands [N,1,2]
        _same_pairs(first, expected[0], "frames 0 -> 1")
        klt.push(frames[2])
        second = klt.track(points)
        _same_pairs(second, expected[1], "frames 1 -> 2")
        # the gate is doing something in these scenes: every counter differs from its neighbour somewhere
        raw, st1, err_ok, fb_ok, kept = expected[0][2]
        assert raw == N and raw > st1 > err_ok >= fb_ok == kept > N // 2
        # the second pair against a tracker that never saw frame 0: the pyramid kept from its time as "current" against a rebuilt one
        fresh = O.KLTTracker((W, H), ctx=gpu_ctx)
        try:
            fresh.push(frames[1]); fresh.push(frames[2])
            _same_pairs(fresh.track(points), second, "fresh tracker")
            a, b = klt.levels(previous=True), fresh.levels(previous=True)
            for key in ("levels", "dx", "dy"):
                for x, y in zip(a[key], b[key]):
                    np.testing.assert_array_equal(x, y)
        finally:
            fresh.close()
        # masks and next_pts of the fused stage against the two separate calls
        p0, p1, counts, nxt, mask = klt.track(points, with_masks=True)
        want = R.calc_optical_flow_pyr_lk(frames[1], frames[2], points, None, criteria=S.MAIN4["criteria"])
        np.testing.assert_array_equal(nxt.view(np.uint32), want[0].reshape(-1, 2).view(np.uint32))
        np.testing.assert_array_equal((mask & O.MASK_STATUS) != 0, want[1].reshape(-1) == 1)
        np.testing.assert_array_equal((mask & O.MASK_ERR) != 0, want[2].reshape(-1) < np.float32(12.0))
        kept_mask = (mask & O.MASK_KEPT) != 0
        assert kept_mask.sum() == counts[4] == len(p0)
        np.testing.assert_array_equal(p0, points[kept_mask])
        np.testing.assert_array_equal(p1, nxt[kept_mask])
        assert ((mask & 7) == 7).sum() == counts[3]
    finally:
        klt.close()
    klt.close()                                                            # twice is harmless
    with pytest.raises(RuntimeError, match="closed"):
        klt.track(points)


def test_no_points_and_one_point(O, gpu_ctx, frames):
    klt = O.KLTTracker((W, H), ctx=gpu_ctx)
    try:
        klt.push(frames[0]); klt.push(frames[1])
        p0, p1, counts = klt.track(np.empty((0, 1, 2), np.float32))
        assert p0.shape == p1.shape == (0, 2) and counts == (0, 0, 0, 0, 0)
        pt = np.array([[100.0, 80.0]], np.float32)
        _same_pairs(klt.track(pt), R.track_forward_backward(frames[0], frames[1], pt, **S.MAIN4), "one point")
        # nothing survives: every point far outside
        p0, p1, counts = klt.track(np.full((70, 2), 1e6, np.float32))
        assert len(p0) == len(p1) == 0 and counts == (70, 0, 0, 0, 0)
    finally:
        klt.close()


def test_device_forms_leave_the_same_results_on_the_device(O, gpu_ctx, frames, points, expected):
    """`sslam_klt_track_dev` / `sslam_klt_track_fb_dev`: device pointers in and out, enqueue only - what a later stage would read"""
    ctx = gpu_ctx
    klt = O.KLTTracker((W, H), ctx=ctx)
    bufs = {k: ctx.malloc(v) for k, v in dict(next=N * 8, st=N, err=N * 4, p0=N * 8, p1=N * 8, cnt=32, mask=N, fbnext=N * 8).items()}
    bufs["pts"] = ctx.upload(points)
    try:
        klt.push(frames[0]); klt.push(frames[1])
        crit = S.MAIN4["criteria"]
        klt.flow_dev(N, bufs["pts"], 0, crit, 0, 1e-4, bufs["next"], bufs["st"], bufs["err"])
        nxt, st, err = np.empty((N, 2), np.float32), np.empty(N, np.uint8), np.empty(N, np.float32)
        ctx.d2h(nxt, bufs["next"]); ctx.d2h(st, bufs["st"]); ctx.d2h(err, bufs["err"])
        want = klt.flow(points, None, crit, 0, 1e-4)
        np.testing.assert_array_equal(nxt.view(np.uint32), want[0].view(np.uint32))
        np.testing.assert_array_equal(st, want[1])
        np.testing.assert_array_equal(err.view(np.uint32), want[2].view(np.uint32))
        # backward from the device-resident forward result
        klt.flow_dev(N, bufs["next"], 0, crit, 0, 1e-4, bufs["fbnext"], bufs["st"], bufs["err"], reverse=True)
        back = np.empty((N, 2), np.float32)
        ctx.d2h(back, bufs["fbnext"])
        np.testing.assert_array_equal(back.view(np.uint32), klt.flow(nxt, None, crit, 0, 1e-4, reverse=True)[0].view(np.uint32))
        klt.flow_fb_dev(N, bufs["pts"], crit, 1e-4, 12.0, 1.5, bufs["p0"], bufs["p1"], bufs["cnt"], bufs["fbnext"], bufs["mask"])
        cnt, p0, p1, mask = np.empty(5, np.int32), np.empty((N, 2), np.float32), np.empty((N, 2), np.float32), np.empty(N, np.uint8)
        ctx.d2h(cnt, bufs["cnt"]); ctx.d2h(p0, bufs["p0"]); ctx.d2h(p1, bufs["p1"]); ctx.d2h(mask, bufs["mask"]); ctx.d2h(back, bufs["fbnext"])
        kept = int(cnt[4])
        _same_pairs((p0[:kept], p1[:kept], cnt.tolist()), expected[0], "track_fb_dev")
        np.testing.assert_array_equal(back.view(np.uint32), nxt.view(np.uint32))
        assert ((mask & O.MASK_KEPT) != 0).sum() == kept
    finally:
        klt.close()
        for d in bufs.values():
            ctx.free(d)


def test_a_frame_that_is_already_on_the_device_is_read_there(O, gpu_ctx, frames, points, expected, monkeypatch):
    """`Undistorter.remap` leaves its result on the device; the tracker handed exactly that array pushes the device copy."""
    U = load_pkg("undistort")
    mapx, mapy = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    und = U.Undistorter.from_maps(np.ascontiguousarray(mapx), np.ascontiguousarray(mapy), ctx=gpu_ctx)
    klt = O.KLTTracker((W, H), ctx=gpu_ctx)
    calls = []
    real = O.KLTTracker.push_dev
    monkeypatch.setattr(O.KLTTracker, "push_dev", lambda self, *a: (calls.append(a), real(self, *a))[1])
    try:
        for f in frames[:2]:
            img = und.remap(f)                                             # identity maps: the same bytes, now also on the device
            np.testing.assert_array_equal(img, f)
            assert U.device_copy(img, gpu_ctx) is not None
            klt.push(img)
        assert len(calls) == 2 and all(c[1:] == (H, W, 3) for c in calls)
        _same_pairs(klt.track(points), expected[0], "device-resident frames")
        klt.push(np.array(und.remap(frames[2])))                           # a copy is an ordinary host array: uploaded
        assert len(calls) == 2
        _same_pairs(klt.track(points), expected[1], "host push after device pushes")
    finally:
        klt.close()
        und.close()
