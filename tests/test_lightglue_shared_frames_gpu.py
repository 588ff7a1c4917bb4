"""GPU: frames shared between the pairs of one LightGlue enqueue (`sslam_lightglue_debug_share_frames`).

Images of one `match_batch_dev` call that name the same source pointers are one frame.  Everything before the first cross
block depends on one image alone, so the shared form runs the prologue and layer 0's self block once per distinct frame and
`lg_fanout_kernel` copies the state to the other images.  Nothing is recomputed, so the bar is bit identity: `ij`, scores and
`info` of every pair are `assert_array_equal` between the hook on, the hook off and the same pairs enqueued one at a time -
ragged counts, both forms of the linears, both split precisions, device-resident counts, pruning and early stop, a forward cut
after layer 0's self block, the fp16 range flag (the exact set of pairs that hold the offending frame) and graph replay."""
import numpy as np
import pytest

import lg_inputs
from conftest import load_pkg

pytestmark = pytest.mark.gpu

EARLY = dict(match_gain=4.0, match_bias=-4.6, conf_bias=2.3)       # seed 4: early stops and prunes (test_lightglue_batch_gpu.py)
PLAIN = dict(match_gain=4.0, match_bias=3.0)                        # seed 1: all nine layers, hundreds of matches


class Frames:
    """Device-resident frames, each uploaded ONCE: pairs built from them name equal pointers, as the frame pipeline's do."""

    def __init__(self, ctx, frames, stride, max_pairs, dev_counts=None):
        self.ctx, self.stride, self.frames = ctx, stride, frames
        self.ptrs, self.rec = [], []
        for f, (xy, desc) in enumerate(frames):
            x, d = ctx.upload(np.ascontiguousarray(xy, np.float32)), ctx.upload(np.ascontiguousarray(desc, np.float32))
            c = ctx.upload(np.int32([dev_counts[f], 0, 0, 0])) if dev_counts is not None else None
            self.ptrs += [x, d] + ([c] if c is not None else [])
            self.rec.append((x, d, len(xy), c))
        self.ij, self.sc, self.info = ctx.malloc(max_pairs * stride * 8), ctx.malloc(max_pairs * stride * 4), ctx.malloc(max_pairs * 16)
        self.ptrs += [self.ij, self.sc, self.info]

    def args(self, pairs):
        out = []
        for a, b in pairs:
            (xa, da, na, ca), (xb, db, nb, cb) = self.rec[a], self.rec[b]
            out.append((xa, da, na, xb, db, nb, ca, cb))
        return out

    def run(self, lg, pairs, min_conf=0.0):
        n = len(pairs)
        lg.match_batch_dev(self.args(pairs), self.ij, self.sc, self.info, self.stride, min_conf=min_conf)
        self.ctx.sync()
        ij, sc, info = np.empty((n, self.stride, 2), np.int32), np.empty((n, self.stride), np.float32), np.empty((n, 4), np.int32)
        self.ctx.d2h(ij, self.ij); self.ctx.d2h(sc, self.sc); self.ctx.d2h(info, self.info)
        return [(ij[p, :max(info[p, 0], 0)].copy(), sc[p, :max(info[p, 0], 0)].copy(), info[p].copy()) for p in range(n)]

    def one_at_a_time(self, lg, pairs, min_conf=0.0):
        return [self.run(lg, [pr], min_conf)[0] for pr in pairs]

    def free(self):
        for p in self.ptrs:
            self.ctx.free(p)


def chain_frames(counts, seed):
    """Frames of one lg_inputs.make_chain, frame f cut to counts[f] keypoints."""
    return [(xy[:n].copy(), d[:n].copy()) for (xy, d), n in zip(lg_inputs.make_chain(len(counts), max(counts), seed=seed), counts)]


def assert_same(a, b):
    assert len(a) == len(b)
    for (a_ij, a_sc, a_info), (b_ij, b_sc, b_info) in zip(a, b):
        np.testing.assert_array_equal(a_info, b_info)
        np.testing.assert_array_equal(a_ij, b_ij)
        np.testing.assert_array_equal(a_sc, b_sc)


def on_off_single(lg, fr, pairs, min_conf=0.0):
    """The batch with the hook on and off and its pairs one at a time (enqueued with the hook off)."""
    lg.debug_share_frames(True)
    on = fr.run(lg, pairs, min_conf)
    shared = lg.debug_share_info()
    lg.debug_share_frames(False)
    off = fr.run(lg, pairs, min_conf)
    assert lg.debug_share_info()[1] is False
    single = fr.one_at_a_time(lg, pairs, min_conf)
    lg.debug_share_frames(True)
    assert_same(on, off)
    assert_same(on, single)
    return on, shared


def make(gpu_ctx, seed, kw, max_kpts, max_pairs, big, precision=2):
    W, LG = load_pkg("weights"), load_pkg("lightglue").LightGlueHIP
    lg = LG(W.random_lightglue_state_dict(seed, **kw), max_kpts=max_kpts, max_pairs=max_pairs, ctx=gpu_ctx)
    # the form of the linears named outright, so that a batch and its single pairs run the same arithmetic (by size a single
    # pair may take the ring kernels, whose LayerNorm sums in another order); -3: no key split at any batch size
    lg.debug_big_gemm(1 if big else 0)
    lg.debug_key_split(-3)
    lg.set_precision(precision)
    return lg


def test_ring_form_three_pairs_over_four_ragged_frames(gpu_ctx):
    fr = Frames(gpu_ctx, chain_frames([128, 100, 77, 128], seed=3), 128, 3)
    lg = make(gpu_ctx, 1, PLAIN, 128, 3, big=False)
    got, shared = on_off_single(lg, fr, [(0, 1), (1, 2), (2, 3)])
    assert shared == (4, True)
    assert [tuple(g[2][2:]) for g in got] == [(128, 100), (100, 77), (77, 128)]
    assert sum(len(g[0]) for g in got) > 20
    fr.free(); lg.close()


@pytest.mark.parametrize("precision", [1, 2])
def test_big_linears_fused_ffn_and_assembly_attention(gpu_ctx, precision):
    """4 pairs over 5 frames at 512 keypoints: NI Kc = 4096, where the plan itself takes the batched form (debug_big_gemm -1)."""
    fr = Frames(gpu_ctx, chain_frames([512, 300, 512, 65, 129], seed=5), 512, 4)
    lg = make(gpu_ctx, 1, PLAIN, 512, 4, big=True, precision=precision)
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4)]
    got, shared = on_off_single(lg, fr, pairs)
    assert shared == (5, True)
    assert sum(len(g[0]) for g in got) > 100
    lg.debug_big_gemm(-1); lg.debug_key_split(0)                   # the product's own selection (key ranges merged in the FFN)
    lg.debug_share_frames(True)
    on = fr.run(lg, pairs)
    lg.debug_share_frames(False)
    assert_same(on, fr.run(lg, pairs))
    assert [g[2][0] for g in on] == [g[2][0] for g in got]         # (key ranges or not: other bits in the scores, the same matches)
    fr.free(); lg.close()


@pytest.mark.parametrize("big", [False, True])
def test_alias_shapes_one_frame_in_three_pairs_a_frame_with_itself_and_no_sharing(gpu_ctx, big):
    fr = Frames(gpu_ctx, chain_frames([256, 200, 131, 256], seed=7), 256, 3)
    lg = make(gpu_ctx, 1, PLAIN, 256, 3, big=big)
    _, shared = on_off_single(lg, fr, [(0, 1), (1, 2), (1, 3)])      # (A,B), (B,C), (B,D)
    assert shared == (4, True)
    _, shared = on_off_single(lg, fr, [(1, 0), (2, 1), (3, 1)])      # ... with the shared frame on the other side
    assert shared == (4, True)
    got, shared = on_off_single(lg, fr, [(2, 2)])                     # (A,A)
    assert shared == (1, True)
    assert len(got[0][0]) > 0                                         # a frame matches itself
    _, shared = on_off_single(lg, fr, [(0, 0), (0, 1), (1, 1)])
    assert shared == (2, True)
    _, shared = on_off_single(lg, fr, [(0, 1), (2, 3)])               # nothing shared: no fan-out launch in the sequence
    assert shared == (4, False)
    fr.free(); lg.close()


def test_device_resident_counts_below_the_bound(gpu_ctx):
    fr = Frames(gpu_ctx, chain_frames([256, 256, 256, 256], seed=9), 256, 3, dev_counts=[256, 131, 0, 77])
    lg = make(gpu_ctx, 1, PLAIN, 256, 3, big=True)
    got, shared = on_off_single(lg, fr, [(0, 1), (1, 3), (3, 0)])
    assert shared == (3, True)
    assert [tuple(g[2][2:]) for g in got] == [(256, 131), (131, 77), (77, 256)]
    # an empty frame (device count 0) shared by two pairs: both are empty-sided, the third pair is not touched
    got, shared = on_off_single(lg, fr, [(1, 2), (2, 3), (3, 1)])
    assert shared == (3, True)
    assert got[0][2][0] == 0 and got[1][2][0] == 0 and got[2][2][0] > 0
    fr.free(); lg.close()


@pytest.mark.parametrize("big", [False, True])
def test_pruning_and_early_stop_move_rows_after_the_shared_segment(gpu_ctx, big):
    fr = Frames(gpu_ctx, chain_frames([400, 350, 256, 512], seed=6), 512, 3)
    lg = make(gpu_ctx, 4, EARLY, 512, 3, big=big)
    got, shared = on_off_single(lg, fr, [(0, 1), (1, 2), (2, 3)])
    assert shared == (4, True)
    sizes = [(400, 350), (350, 256), (256, 512)]
    assert any(tuple(g[2][2:]) != s for g, s in zip(got, sizes)), "no pair pruned a point"
    assert any(g[2][1] < 9 for g in got), "no pair stopped early"
    fr.free(); lg.close()


@pytest.mark.parametrize("big", [False, True])
def test_token_state_after_layer_0_self_block_is_the_unshared_one(gpu_ctx, big):
    counts = [256, 200, 131, 256]
    fr = Frames(gpu_ctx, chain_frames(counts, seed=11), 256, 3)
    lg = make(gpu_ctx, 1, PLAIN, 256, 3, big=big)
    lg.debug_layers(1, True)
    pairs = [(0, 1), (1, 2), (1, 3)]

    def state():
        fr.run(lg, pairs)
        return [lg.debug_read(0x100 * p, (2, 256, 256)) for p in range(len(pairs))], \
               [lg.debug_read(0x100 * p + 5, (2, 256, 32)) for p in range(len(pairs))]
    lg.debug_share_frames(True)
    x_on, e_on = state()
    assert lg.debug_share_info() == (4, True)
    lg.debug_share_frames(False)
    x_off, e_off = state()
    for p, (a, b) in enumerate(pairs):
        for side, f in enumerate((a, b)):
            n = counts[f]
            np.testing.assert_array_equal(x_on[p][side, :n], x_off[p][side, :n])
            np.testing.assert_array_equal(e_on[p][side, :n], e_off[p][side, :n])
            assert np.abs(x_on[p][side, :n]).max() > 0.1
    # every image of frame 1 holds the same state
    np.testing.assert_array_equal(x_on[1][0, :200], x_on[0][1, :200])
    np.testing.assert_array_equal(x_on[2][0, :200], x_on[0][1, :200])
    fr.free(); lg.close()


@pytest.mark.parametrize("bad,flagged", [(2, {1, 2}), (0, {0}), (1, {0, 1})])
def test_range_flag_reaches_exactly_the_pairs_that_hold_the_frame(gpu_ctx, bad, flagged):
    """A descriptor value of 1e6 leaves the fp16 planes in the shared segment (the split of the descriptors): with the frame
    computed once, its flag must still reach every pair that holds it and no other.  bad = 0: image 0 of pair 0; bad = 1:
    image 1 of pair 0 (and image 0 of pair 1)."""
    frames = chain_frames([256, 200, 131, 256], seed=13)
    clean = Frames(gpu_ctx, frames, 256, 3)
    frames = [(xy, d.copy()) for xy, d in frames]
    frames[bad][1][17, 5] = 1e6
    fr = Frames(gpu_ctx, frames, 256, 3)
    lg = make(gpu_ctx, 1, PLAIN, 256, 3, big=True)
    pairs = [(0, 1), (1, 2), (2, 3)]
    want = clean.run(lg, pairs)
    assert lg.range_overflow() is False
    for share in (True, False):
        lg.debug_share_frames(share)
        got = fr.run(lg, pairs)
        assert {p for p in range(3) if got[p][2][0] == -1} == flagged, share
        assert lg.range_overflow() is True and lg.range_overflow() is False      # the sticky word: raised, read once
        for p in set(range(3)) - flagged:
            assert_same([got[p]], [want[p]])
        assert_same(fr.run(lg, pairs), got)                         # the flags are reset by every enqueue, not accumulated
        assert lg.range_overflow() is True
        assert_same(clean.run(lg, pairs), want)                     # ... and a clean batch behind it is clean
        assert lg.range_overflow() is False
    fr.free(); clean.free(); lg.close()


def test_graph_replay_and_another_alias_structure_on_the_same_instance(gpu_ctx):
    fr = Frames(gpu_ctx, chain_frames([256, 200, 131, 256], seed=15), 256, 3)
    lg = make(gpu_ctx, 4, EARLY, 256, 3, big=True)
    a, b, c = [(0, 1), (1, 2), (2, 3)], [(0, 1), (1, 2), (1, 3)], [(0, 1), (2, 3)]
    lg.debug_share_frames(False)
    want = {k: fr.run(lg, v) for k, v in (("a", a), ("b", b), ("c", c))}
    lg.debug_share_frames(True)
    lg.use_graphs(True)
    for k, v, info in (("a", a, (4, True)), ("a", a, (4, True)), ("b", b, (4, True)), ("c", c, (4, False)), ("a", a, (4, True)),
                       ("b", b, (4, True))):
        assert_same(fr.run(lg, v), want[k])                        # capture, replay, another structure, replay of the first
        assert lg.debug_share_info() == info
    lg.debug_share_frames(False)                                    # (drops the cache: the graphs above held the fan-out)
    assert_same(fr.run(lg, a), want["a"])
    assert_same(fr.run(lg, a), want["a"])
    lg.use_graphs(False)
    fr.free(); lg.close()
