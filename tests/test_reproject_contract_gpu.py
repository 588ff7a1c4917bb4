"""The argument contract of the four 2D-3D association entries (csrc/reproject_kernels.hip: one check, `rm_check`, behind
`sslam_reproject_match_host` / `_dev` and `sslam_reproject_match_hamming_host` / `_dev`), through `native.lib()` directly:

* every refusal - one violated condition on an otherwise legal call of 3 points x 4 keypoints - is status 2 with a message
  that begins with the name of the entry that was CALLED and holds the condition's phrase, and happens before any GPU work
  (the output buffer keeps its sentinel: the kernels write every kp_of_point);
* every entry accepts the smallest legal call, 1 point x 1 keypoint, with uv_out (and, `_host`, info_out) NULL.

The `_dev` entries get real device buffers in every case, so a check that failed to refuse would still read valid memory."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENTRIES = {  # name -> (Hamming form, device-resident)
    "sslam_reproject_match_host": (False, False),
    "sslam_reproject_match_dev": (False, True),
    "sslam_reproject_match_hamming_host": (True, False),
    "sslam_reproject_match_hamming_dev": (True, True),
}
B = 32
SENTINEL = 77
ARRAYS = ("pts3d", "obs_cnt", "obs", "kp_xy", "des", "kp_of_point", "info_out")     # device arrays of a `_dev` call
REQUIRED = ("pts3d", "obs_cnt", "obs", "K9", "Tcw16", "kp_xy", "des", "kp_of_point")


def legal(name, Q, N):
    """A legal call of Q points x N keypoints: K = (100, 100, 32, 32), identity pose, every point at (0, 0, 5) - pixel
    (32, 32) of a 64 x 64 image -, every keypoint there too, radius 1, one stored row per point, equal to every frame row."""
    hamming, _ = ENTRIES[name]
    if hamming:
        row = np.random.default_rng(3).integers(0, 256, B, dtype=np.uint8)
        obs = np.zeros((Q, 6, 64), np.uint8); obs[:, 0, :B] = row
        des = np.tile(row, (N, 1))
    else:
        row = np.random.default_rng(3).standard_normal(128).astype(np.float32); row /= np.linalg.norm(row)
        obs = np.zeros((Q, 6, 128), np.float32); obs[:, 0] = row
        des = np.tile(row, (N, 1))
    return dict(n_points=Q, pts3d=np.tile([0.0, 0.0, 5.0], (Q, 1)), obs_cnt=np.ones(Q, np.int32), obs=obs,
                K9=np.array([100.0, 0, 32, 0, 100, 32, 0, 0, 1]), Tcw16=np.eye(4).reshape(16), n_kp=N,
                kp_xy=np.full((N, 2), 32.0, np.float32), des=np.ascontiguousarray(des), desc_bytes=B, img_w=64, img_h=64,
                radius_px=1.0, max_dist=64.0 if hamming else 0.8, kp_of_point=np.full(Q, SENTINEL, np.int32), uv_out=None,
                info_out=np.full(4, SENTINEL, np.int32))


class Call:
    """The arguments of one entry by name; a `_dev` entry's arrays are uploaded (with slack behind each)."""

    def __init__(self, native, ctx, name, Q, N):
        self.native, self.ctx, self.name = native, ctx, name
        self.hamming, self.dev = ENTRIES[name]
        self.args = dict(legal(name, Q, N), ctx=ctx.handle)
        self.owned = []
        if self.dev:
            for k in ARRAYS:
                host = self.args[k]
                d = ctx.malloc(host.nbytes + 4096)
                ctx.h2d(d, host)
                self.owned.append(d)
                self.args[k] = d

    def __call__(self, **changed):
        a = dict(self.args, **changed)
        P = self.native.ptr
        argv = [a["ctx"], a["n_points"], P(a["pts3d"]), P(a["obs_cnt"]), P(a["obs"]), P(a["K9"]), P(a["Tcw16"]), a["n_kp"],
                P(a["kp_xy"]), P(a["des"])] + ([a["desc_bytes"]] if self.hamming else []) + \
               [a["img_w"], a["img_h"], a["radius_px"], a["max_dist"], P(a["kp_of_point"]), P(a["uv_out"]), P(a["info_out"])]
        if self.hamming and self.dev:
            argv.append(None)                                                        # n_kp_dev
        return getattr(self.native.lib(), self.name)(*argv)

    def read(self, key, count):
        """int32 output `key` as the host sees it after the stream drained."""
        if not self.dev:
            return self.args[key][:count].copy()
        self.ctx.sync()
        out = np.empty(count, np.int32)
        self.ctx.d2h(out, self.args[key])
        return out

    def close(self):
        for d in self.owned:
            self.ctx.free(d)


def refusals(name):
    """(case id, changed arguments, phrase) of every condition the entry `name` refuses."""
    hamming, dev = ENTRIES[name]
    cases = [("ctx", dict(ctx=None), "ctx is NULL"), ("n_points=0", dict(n_points=0), "empty input"),
             ("n_kp=0", dict(n_kp=0), "empty input"), ("radius<0", dict(radius_px=-1.0), "bad radius"),
             ("img_w=0", dict(img_w=0), "bad radius")]
    cases += [(f"{k}=NULL", {k: None}, "NULL argument") for k in REQUIRED + (("info_out",) if dev else ())]
    if not dev:
        cases += [(f"obs_cnt={v}", dict(obs_cnt=np.array([1, v, 1], np.int32)), "obs_cnt") for v in (7, -1)]
    if hamming:
        cases += [(f"desc_bytes={v}", dict(desc_bytes=v), "desc_bytes") for v in (1, 65)]
    if hamming and dev:
        cases.append(("obs+1", "obs+1", "16-byte aligned"))
    return cases


@pytest.fixture(scope="module")
def calls(native, gpu_ctx):
    made = {name: Call(native, gpu_ctx, name, 3, 4) for name in ENTRIES}
    yield made
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name,changed,phrase", [pytest.param(n, ch, ph, id=f"{n}-{cid}") for n in ENTRIES
                                                 for cid, ch, ph in refusals(n)])
def test_refusal_names_the_called_entry_and_does_no_gpu_work(native, calls, name, changed, phrase):
    call = calls[name]
    if changed == "obs+1":
        changed = dict(obs=call.args["obs"] + 1)
    rc = call(**changed)
    msg = native.lib().sslam_last_error().decode()
    print(rc, msg)
    assert rc == 2
    assert msg.startswith(name + ":") and phrase in msg
    assert (call.read("kp_of_point", 3) == SENTINEL).all()


@pytest.mark.parametrize("name", list(ENTRIES))
def test_smallest_legal_call_is_accepted(native, gpu_ctx, name):
    call = Call(native, gpu_ctx, name, 1, 1)
    try:
        native.check(call(), name)                                                   # uv_out = NULL
        assert list(call.read("kp_of_point", 1)) == [0]
        if call.dev:
            assert list(call.read("info_out", 4)) == [1, 0, 1, 0]                    # matches, overflow, candidates, 0
        else:
            assert list(call.read("info_out", 2)) == [1, 1]                          # matches, candidates
            call.args["kp_of_point"][:] = SENTINEL
            native.check(call(info_out=None), name)
            assert list(call.read("kp_of_point", 1)) == [0]
    finally:
        call.close()
