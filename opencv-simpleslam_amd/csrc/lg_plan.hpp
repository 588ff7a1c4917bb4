// lg_plan.hpp - which kernel forms one LightGlue forward launches, decided ONCE per enqueue from the instance's
// hooks and the batch size.  Plain C++17 with no HIP include: tests/test_lg_plan.py compiles it with the host
// compiler and sweeps it on the CPU.  Every hooked form gives bit-identical results (tests/test_lightglue_batch_gpu.py),
// so a wrong SELECTION shows in speed only - the measured size thresholds below are guarded by that CPU test.
// The raw integers of sslam_lightglue_debug_key_split / _debug_big_gemm are interpreted here and nowhere else.
#pragma once

namespace sslam {

constexpr int LG_NH = 4;         // heads
constexpr int LG_NL = 9;         // layers
constexpr int LG_AQ = 128;       // attention: queries per block
constexpr int LG_AK = 64;        // attention: keys per LDS tile

// key split the attention partial buffers of an instance of capacity Kc are sized for
constexpr int lg_ks_max(int Kc) { return Kc >= 1024 ? 4 : (Kc >= 512 ? 2 : 1); }

// what the setters store, unchanged (sslam_hip.h documents the accepted values)
struct LGHooks {
    int precision = 2;           // set_precision: 0 fp32 MFMA everywhere; 1 fp16 hi/lo split planes (three MFMAs per product);
                                 // 2 "f16x3p1" (the DEFAULT since r05 - profiles/r05_flip_soak.md): as 1 with P as one fp16 plane in P.V
    bool sim_exact = false;      // SSLAM_LG_SIM_EXACT=1 (experiments): projections + similarity stay on the fp32 matrix instruction
    int layers = LG_NL;          // debug_layers: run only the first `layers` layers ...
    bool self_only = false;      // ... and stop after the self block of the last executed one
    int key_split = 0;           // debug_key_split: 0 by batch size; -5 .. 104, decoded in lg_plan
    int big_gemm = -1;           // debug_big_gemm: -1 by batch size; 0 .. 5, decoded in lg_plan
    int study = 0;               // debug_split_form: which cross terms of the split products are dropped (bit mask)
    bool share_frames = true;    // debug_share_frames: a frame that several images of one enqueue name is computed once up to
                                 // the end of layer 0's self block (lg_alias below)
};

enum class LGAttn { F32, FourWave, Asm };       // lg_attention_kernel | lg_attention_p_kernel | lg_attention_asm[_p1]_kernel
enum class LGMerge { None, Launch, InFfn };     // who merges the key-range partials: nobody | a merge launch | the fused FFN's tiles
enum class LGLinears { Ring, Big };             // 64-row ring linears + 3-launch FFN | 128 x 128 linears + the fused FFN kernel
enum class LGFfnTile { T64, T32 };              // tokens per fused-FFN tile

struct LGPlan {
    bool split;                  // transformer layers on the fp16 split planes (precision != 0); the fields marked (s) hold only then
    bool proj_split;             // input / final projection and the similarity GEMM on the split pipe too
    LGAttn attn;
    bool p_single;               // (s) P as ONE fp16 plane: the 4-wave kernel's argument / the assembly kernel's p1 twin
    int ks;                      // key ranges of an attention launch: 1, 2 or 4
    LGMerge merge;
    LGLinears linears;           // (s)
    LGFfnTile ffn_tile;          // (s) Big only
    bool heads_in_ffn;           // the token heads ride in the cross block's fused FFN of every layer but the last executed
                                 // one; otherwise lg_token_heads_kernel runs
    int layers;
    bool self_only_last;
    bool share_frames;           // (s) images that lg_alias maps to an earlier one skip the prologue and layer 0's self block and
                                 // receive the representative's state from lg_fanout_kernel.  The fp32 path (precision 0) keeps
                                 // computing every image: it is the exact reference, not the product path
};

// NI = images of this enqueue (2 per pair); want_heads = the instance stops early or prunes (depth_conf > 0 || width_conf > 0)
inline LGPlan lg_plan(const LGHooks& h, int Kc, int NI, bool want_heads) {
    LGPlan p{};
    p.split = h.precision != 0;
    p.proj_split = p.split && !h.sim_exact;
    p.layers = h.layers;
    p.self_only_last = h.self_only;
    p.share_frames = h.share_frames && p.split;

    // debug_key_split:   0 by size | -3 none | -5 by size, merge launch | 101 102 104 forced   -> the assembly kernel
    //                   -4 by size | -1 none |                          |   1   2   4 forced   -> the 4-wave r02 kernel
    const int k = h.key_split;
    const bool forced = k > 0, by_size = k == 0 || k == -4 || k == -5;
    const bool asm_kernel = k == 0 || k == -3 || k == -5 || k > 100;
    const bool fold_allowed = k == 0 || k > 100;              // (-5: the same launches with the merge as a launch of its own)
    p.ks = forced ? (k > 100 ? k - 100 : k) : 1;
    if (by_size) {
        // enough (image, head, query-block) units to give every CU a workgroup without it, otherwise split the keys.
        // One workgroup per CU is the measured optimum of the assembly kernel (2048-keypoint pair, 128 units: no split 1.68 ms
        // per forward, 2 ranges 1.59, 4 ranges 1.65; the 4-wave kernel 1.69 at 2 or 4)
        const int units = NI * LG_NH * (Kc / LG_AQ);
        while (p.ks < 4 && units * p.ks < 256 && Kc / LG_AK >= 2 * p.ks * 4) p.ks *= 2;
    }
    if (p.ks > lg_ks_max(Kc)) p.ks = lg_ks_max(Kc);

    if (!p.split) {              // fp32 path: one attention kernel, whose partials a launch ALWAYS merges (also a single range)
        p.attn = LGAttn::F32;
        p.merge = LGMerge::Launch;
        return p;
    }
    // study bit 0x04 (P as one plane, whatever the precision mode) exists in the 4-wave kernel only
    p.attn = asm_kernel && !(h.study & 0x04) ? LGAttn::Asm : LGAttn::FourWave;
    p.p_single = h.precision == 2 || (h.study & 0x04);

    // debug_big_gemm: -1 by size | 0 ring | 1 big | 2 big, 64-token tiles | 3 big, 32-token tiles | 5 big, heads as a launch.
    // By size: enough token rows for 128-row tiles to fill the chip (a batch of pairs); a single pair keeps the 64-row ring
    // kernels (r01 form).  Too few 64-token FFN tiles for the chip: 32-token tiles (same results).
    const int b = h.big_gemm;
    const bool big = b >= 0 ? b != 0 : ((long)NI * Kc >= 4096 && Kc % 128 == 0);
    p.linears = big ? LGLinears::Big : LGLinears::Ring;
    p.ffn_tile = b == 3 || (b != 2 && NI * (Kc / 64) <= 128) ? LGFfnTile::T32 : LGFfnTile::T64;
    p.heads_in_ffn = big && b != 5 && want_heads;

    // one pair: the key-range partials are merged by the 32-token FFN tiles (ffn_fused.hpp FOLD), not by a launch of their
    // own.  Only the assembly kernel's partials, and never under the precision study
    if (p.ks == 1) p.merge = LGMerge::None;
    else p.merge = big && p.ffn_tile == LGFfnTile::T32 && h.study == 0 && fold_allowed ? LGMerge::InFfn : LGMerge::Launch;
    return p;
}

// Which images of one enqueue are the SAME frame.  Image j is an alias of the earliest image i < j whose source entries are
// all equal - keypoint, descriptor and count pointers, the host bound and the 'image_size' pair - because everything before
// the first cross block depends on those alone.  rep[j] = that earliest image (rep[j] == j: j is computed); an alias of an
// alias therefore resolves to the earliest one.  Returns the number of distinct images.  The graph cache's key
// (lg_enqueue_cached) holds every field compared here, so a cached graph always belongs to one alias structure.
template <class PX, class PD, class PC>
inline int lg_alias(int NI, const PX* xy, const PD* desc, const PC* cnt, const int* bound, const float* size_w,
                    const float* size_h, int* rep) {
    int distinct = 0;
    for (int j = 0; j < NI; ++j) {
        rep[j] = j;
        for (int i = 0; i < j; ++i)
            if (xy[i] == xy[j] && desc[i] == desc[j] && cnt[i] == cnt[j] && bound[i] == bound[j] && size_w[i] == size_w[j] &&
                size_h[i] == size_h[j]) {
                rep[j] = i;          // the first match is the earliest: i itself is never an alias of a later image
                break;
            }
        distinct += rep[j] == j;
    }
    return distinct;
}

}  // namespace sslam
