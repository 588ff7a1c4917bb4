// al_plan.hpp - everything the host decides about one ALIKED call, decided ONCE per call from (H, W, C, F): the resize rule
// and padding, the launch splits, and whether the instance takes the frame at all; plus the element count of every
// per-frame workspace buffer.  Plain C++17 with no HIP include: tests/test_al_plan.py compiles it with the host compiler and
// sweeps every legal network size and batch size on the CPU.  aliked_kernels.hip launches from these fields and holds no
// size arithmetic of its own; the shape constants below are the ones its kernels are written for, defined here only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>

namespace sslam {

constexpr int AL_LONG_SIDE = 1024;    // the network never runs larger than this on the long side ...
constexpr int AL_PAD_DIV = 32;        // ... + centred padding to a multiple of the coarsest level's stride
constexpr int MAX_FRAMES = 16;        // frames of one batched launch sequence (FrameIn / FrameOut hold that many pointers)
constexpr int B1_SW = 30;             // al_block1_rows_kernel: output pixels per strip
constexpr int B2_SW = 30;             // al_block2_rows_kernel: output pixels per strip
constexpr int DCN3_CS = 1;            // workgroups per pixel tile of the 1/8 deformable layers ...
constexpr int DCN4_CS = 4;            // ... and of the 1/32 ones (output channels split: 10 tiles per frame there)
constexpr int AGG_PRE = 13;           // pre-aggregation planes per level (8 projections + S, H, V, D1, D2)
constexpr int L2_TW = 32, L2_TH = 8;  // al_level2_kernel: interior tile of 1/2-level pixels (whole 4 x 4 pooling cells)
constexpr int LS_TW = 16, LS_TH = 4;  // al_level_small_kernel: interior tile of 1/8- and 1/32-level pixels
constexpr int ST_W = 32, ST_H = 8;    // al_score_tail_kernel: output tile
constexpr int PRE_LDS_MAX = 48 * 1024;  // al_preprocess_kernel: most LDS bytes a tile may take (three workgroups per CU at least)
constexpr int NHALO = 10;             // dependency radius of simple_nms: 2 + 4 + 4
constexpr int NW_R = 48, NW_OW = 64 - 2 * NHALO, NW_OH = NW_R - 2 * NHALO;      // al_nms_wave_kernel: rows held, output tile
constexpr int HBINS = 4096;           // score histogram bins (uniform in score, monotone)
constexpr int COLLECT_PPT = 16;       // pixels per thread: 4096 per block -> ~80 blocks, one same-address atomic each
constexpr int SEL_CAP = 8192;         // max keypoints (sort capacity)
constexpr int EDGE_CAP = 2048;        // candidates allowed in the cut bin before falling back to radix select
constexpr int CAND_CAP = 1024 * 1024; // candidate keys per frame
constexpr int REFINE_KPB = 32;        // keys per 256-thread block
constexpr int SDDH_KSPLIT = 4;        // k ranges of the two descriptor-head GEMMs whose partials a later kernel sums

constexpr int al_cdiv(int a, int b) { return (a + b - 1) / b; }

// network-size bookkeeping of one image.  Kernels take it by value.
struct Dims {
    int H, W, C;          // input image
    int h, w;             // resized
    int Hp, Wp;           // padded (multiple of 32)
    int pl, pt;           // left / top padding
};

enum class ALAggTile { T64x64, T64x128 };      // the al_gemm_h_kernel form of the descriptor head's last GEMM

struct ALPlan {
    int F, KF;                          // frames: the last used grid dimension of every launch; x SDDH_KSPLIT for the k-split GEMMs
    int blur, ky, kx;                   // antialias blur before the resize: on / taps
    float sy, sx;                       // ... and its sigmas
    Dims d;
    int to_float_gx, pad_gx;            // 256-pixel row pieces of the input / of the padded map (also the aggregate kernel's)
    // block1 / block2: a wave owns a strip of B?_SW pixels x `hs` rows.  nblk is the row-block count aimed at, nb = cdiv(rows, hs)
    // the one launched.  Both depend on F; a frame's values do not (no sum is re-associated)
    int b1_strips, b1_nblk, b1_hs, b1_nb;
    int b2_strips, b2_nblk, b2_hs, b2_nb, b2_waves, b2_gx;
    int H2, W2, HW2, H3, W3, HW3, H4, W4, HW4;          // the 1/2, 1/8 and 1/32 levels
    int pool3_gx, pool4_gx;             // al_avgpool_kernel into the two deformable blocks
    int off3_gx, dcn3_gx, off4_gx, dcn4_gx;             // 32-pixel row tiles of the offset conv / x DCN?_CS of the deformable conv
    float mo3, mo4, mo;                 // offset clamp max(rows, cols) / 4 of the two deformable blocks and of SDDH
    int gate2_gx, gate3_gx, gate4_gx, gate34_gx;        // (the two small levels share one launch of gate3_gx + gate4_gx blocks)
    float sy2, sx2, sy8, sx8, sy32, sx32;               // Pyr: align_corners=True source steps of the three upsampled levels
    int agg_pre_gx;
    int tail_gx, tail_gy;
    int nbx, nby, n_tiles, nms_gx;      // NMS: one wave per NW_OW x NW_OH tile, four per workgroup
    int npx, collect_gx;
    ALAggTile agg_tile;
    float scale_x, scale_y;             // network pixels per input pixel
    // al_preprocess_kernel: a workgroup owns pre_tw x pre_th pixels of the padded image (pre_tw a power of two) and keeps the
    // horizontally blurred source span they read in LDS: at most pre_cols columns x pre_rows rows per channel, beside the raw
    // bytes of those rows (pre_raw bytes per row) and the 256 floats of b / 255
    int pre_tw, pre_th, pre_gx, pre_gy, pre_cols, pre_rows, pre_raw, pre_lds;
    // the fused gate + pre-aggregation kernels: L2_TW x L2_TH tiles of the 1/2 level (al_level2_kernel, which also pools into
    // block3), LS_TW x LS_TH tiles of the two small levels in one launch (lvl3_n workgroups of the 1/8 level, then lvl4_n)
    int lvl2_gx, lvl2_gy;
    int lvl3_gx, lvl3_n, lvl4_gx, lvl4_n, lvl34_n;
};

inline ALPlan al_plan(int H, int W, int C, int F) {
    ALPlan p{};
    p.F = F; p.KF = SDDH_KSPLIT * F;
    Dims& d = p.d;
    d.H = H; d.W = W; d.C = C;
    // kornia resize(side='long'): the long side becomes AL_LONG_SIDE, the other int(AL_LONG_SIDE / aspect)
    const double ar = (double)W / (double)H;
    if (ar > 1.0) { d.h = (int)(AL_LONG_SIDE / ar); d.w = AL_LONG_SIDE; }
    else { d.h = AL_LONG_SIDE; d.w = (int)(AL_LONG_SIDE * ar); }
    const double fy = (double)H / d.h, fx = (double)W / d.w;
    p.blur = (fy > fx ? fy : fx) > 1.0;
    const double sgy = (fy - 1.0) / 2.0 > 0.001 ? (fy - 1.0) / 2.0 : 0.001, sgx = (fx - 1.0) / 2.0 > 0.001 ? (fx - 1.0) / 2.0 : 0.001;
    p.sy = (float)sgy; p.sx = (float)sgx;
    const double ksy = 2.0 * 2 * sgy, ksx = 2.0 * 2 * sgx;
    p.ky = (int)(ksy > 3 ? ksy : 3); p.kx = (int)(ksx > 3 ? ksx : 3);
    if (p.ky % 2 == 0) ++p.ky;
    if (p.kx % 2 == 0) ++p.kx;
    // centred pad to a multiple of AL_PAD_DIV
    const int pad_h = (((d.h / AL_PAD_DIV) + 1) * AL_PAD_DIV - d.h) % AL_PAD_DIV;
    const int pad_w = (((d.w / AL_PAD_DIV) + 1) * AL_PAD_DIV - d.w) % AL_PAD_DIV;
    d.Hp = d.h + pad_h; d.Wp = d.w + pad_w; d.pl = pad_w / 2; d.pt = pad_h / 2;
    const int Hp = d.Hp, Wp = d.Wp;

    p.to_float_gx = al_cdiv(W, 256); p.pad_gx = al_cdiv(Wp, 256);
    // block1 (conv1 + conv2 fused): ~3 waves per SIMD when the batch allows; at least four rows per wave (two extra conv1 rows
    // per block: short blocks only when one or two frames have to fill the chip)
    p.b1_strips = al_cdiv(Wp, B1_SW);
    p.b1_nblk = std::max(1, std::min(al_cdiv(Hp, 4), 3072 / std::max(1, p.b1_strips * F)));
    p.b1_hs = al_cdiv(Hp, p.b1_nblk);
    p.b1_nb = al_cdiv(Hp, p.b1_hs);
    // block2 at 1/2 (pooling + conv1 + 1 x 1 branch + conv2 + residual fused): one wave per SIMD when the batch allows; at
    // least three rows per wave (two extra t2 rows per block)
    p.H2 = Hp / 2; p.W2 = Wp / 2; p.HW2 = p.H2 * p.W2;
    p.b2_strips = al_cdiv(p.W2, B2_SW);
    p.b2_nblk = std::max(1, std::min(al_cdiv(p.H2, 3), 1024 / std::max(1, p.b2_strips * F)));
    p.b2_hs = al_cdiv(p.H2, p.b2_nblk);
    p.b2_nb = al_cdiv(p.H2, p.b2_hs);
    p.b2_waves = p.b2_strips * p.b2_nb * F;
    p.b2_gx = al_cdiv(p.b2_waves, 4);
    // block3 at 1/8, block4 at 1/32 (deformable)
    p.H3 = Hp / 8; p.W3 = Wp / 8; p.HW3 = p.H3 * p.W3;
    p.H4 = Hp / 32; p.W4 = Wp / 32; p.HW4 = p.H4 * p.W4;
    p.pool3_gx = al_cdiv(32 * p.HW3, 256); p.pool4_gx = al_cdiv(64 * p.HW4, 256);
    p.off3_gx = al_cdiv(p.W3, 32); p.dcn3_gx = DCN3_CS * al_cdiv(p.W3, 32);
    p.off4_gx = al_cdiv(p.W4, 32); p.dcn4_gx = DCN4_CS * al_cdiv(p.W4, 32);
    p.mo3 = (float)(p.H3 > p.W3 ? p.H3 : p.W3) / 4.0f;
    p.mo4 = (float)(p.H4 > p.W4 ? p.H4 : p.W4) / 4.0f;
    p.gate2_gx = al_cdiv(p.HW2, 256); p.gate3_gx = al_cdiv(32 * p.HW3, 256); p.gate4_gx = al_cdiv(32 * p.HW4, 256);
    p.gate34_gx = p.gate3_gx + p.gate4_gx;
    // aggregation + score head
    auto step = [](int full, int S) { return (float)(full / S - 1) / (float)(full - 1); };
    p.sy2 = step(Hp, 2); p.sx2 = step(Wp, 2); p.sy8 = step(Hp, 8); p.sx8 = step(Wp, 8);
    p.sy32 = step(Hp, 32); p.sx32 = step(Wp, 32);
    p.agg_pre_gx = al_cdiv(p.HW2 + p.HW3 + p.HW4, 256);
    p.lvl2_gx = al_cdiv(p.W2, L2_TW); p.lvl2_gy = al_cdiv(p.H2, L2_TH);
    p.lvl3_gx = al_cdiv(p.W3, LS_TW); p.lvl3_n = p.lvl3_gx * al_cdiv(p.H3, LS_TH);
    p.lvl4_gx = al_cdiv(p.W4, LS_TW); p.lvl4_n = p.lvl4_gx * al_cdiv(p.H4, LS_TH);
    p.lvl34_n = p.lvl3_n + p.lvl4_n;
    p.tail_gx = al_cdiv(Wp, ST_W); p.tail_gy = al_cdiv(Hp, ST_H);
    // DKD on the un-padded map
    p.nbx = al_cdiv(d.w, NW_OW); p.nby = al_cdiv(d.h, NW_OH); p.n_tiles = p.nbx * p.nby;
    p.nms_gx = al_cdiv(p.n_tiles, 4);
    p.npx = d.h * d.w;
    p.collect_gx = al_cdiv(p.npx, 256 * COLLECT_PPT);
    // SDDH
    p.mo = (float)(d.h > d.w ? d.h : d.w) / 4.0f;
    // (batches: 64 x 128 tiles - the 16.8 MB of sampled-feature planes are read once; with two column blocks the PMC counters
    //  showed 35.7 MB fetched per frame.  One or two frames: 64 x 64 tiles, twice the workgroups.  Same k-split, same order:
    //  bit-identical)
    p.agg_tile = F >= 4 ? ALAggTile::T64x128 : ALAggTile::T64x64;
    p.scale_x = (float)d.w / (float)W; p.scale_y = (float)d.h / (float)H;
    // pre-processing: the largest tile of the ladder whose source span fits PRE_LDS_MAX.  Neighbouring network pixels are fx (fy)
    // source pixels apart and a pixel reads source columns x0 and x0 + 1, so tw pixels span at most fx (tw - 1) + 3 columns (one
    // more here for the rounding of the device's fp32 coordinates), rows the same plus the vertical taps either side; the raw rows
    // carry the horizontal taps either side, C bytes a pixel, whole dwords from an aligned address.  The last tile, 4 x 1, takes
    // 35 KB at 31 taps (fx = fy = 17, C = 4): every size al_refusal admits fits
    {
        static constexpr int ladder[][2] = {{64, 8}, {32, 8}, {32, 4}, {16, 4}, {16, 2}, {8, 2}, {8, 1}, {4, 1}};
        const int rx = p.blur ? p.kx / 2 : 0, ry = p.blur ? p.ky / 2 : 0, planes = C == 1 ? 1 : 3;
        for (const auto& t : ladder) {
            p.pre_tw = t[0]; p.pre_th = t[1];
            p.pre_cols = (int)(fx * (t[0] - 1)) + 4;
            p.pre_rows = (int)(fy * (t[1] - 1)) + 4 + 2 * ry;
            p.pre_raw = ((p.pre_cols + 2 * rx) * C + 3) / 4 * 4 + 4;
            p.pre_lds = 256 * 4 + planes * p.pre_rows * p.pre_cols * 4 + p.pre_rows * p.pre_raw;
            if (p.pre_lds <= PRE_LDS_MAX) break;
        }
        p.pre_gx = al_cdiv(Wp, p.pre_tw); p.pre_gy = al_cdiv(Hp, p.pre_th);
    }
    return p;
}

// Why an instance of capacity (Hp_cap, Wp_cap, max_frames) does not take the plan's call: None, or the reason with its
// message in `msg`.  Nothing of a refused call may be launched or captured.
enum class ALRefusal { None, Size, Frames, Blur };
inline ALRefusal al_refusal(const ALPlan& p, int Hp_cap, int Wp_cap, int max_frames, char* msg, size_t n) {
    const Dims& d = p.d;
    if (!(d.Hp <= Hp_cap && d.Wp <= Wp_cap && d.h >= 8 && d.w >= 8)) {
        snprintf(msg, n, "sslam_aliked: network size %dx%d outside the instance capacity %dx%d", d.Hp, d.Wp, Hp_cap, Wp_cap);
        return ALRefusal::Size;
    }
    if (!(p.F >= 1 && p.F <= max_frames)) {
        snprintf(msg, n, "sslam_aliked: %d frames, instance capacity %d", p.F, max_frames);
        return ALRefusal::Frames;
    }
    if (!(p.kx <= 31 && p.ky <= 31)) {        // (al_reset_kernel writes the taps into 32 floats per axis)
        snprintf(msg, n, "sslam_aliked: blur kernel too large (%d,%d)", p.kx, p.ky);
        return ALRefusal::Blur;
    }
    return ALRefusal::None;
}

// The descriptor head works on the instance's keypoint CAPACITY NK (rows past the frame's count are skipped on the device), so
// its grids are fixed at instance creation.
struct ALKptPlan {
    int NK;
    int refine_gx, patch_gx, offsets_gx, sample_gx, finalize_gx;
    int rows_x16, rows64, rows64_x16;   // the 16 samples of every keypoint as rows; 64-row tiles of the GEMMs over [NK] and [NK * 16] rows
    size_t plane;                       // halves between the hi and the lo plane of `sampled` / `feats`
};

inline ALKptPlan al_kpt_plan(int NK) {
    ALKptPlan k{};
    k.NK = NK;
    k.refine_gx = al_cdiv(NK, REFINE_KPB);
    k.patch_gx = al_cdiv(NK * 3, 4);
    k.rows64 = al_cdiv(NK, 64);
    k.offsets_gx = al_cdiv(NK * 32, 256);
    k.sample_gx = al_cdiv(NK * 16, 4);
    k.rows_x16 = NK * 16;
    k.rows64_x16 = al_cdiv(NK * 16, 64);
    k.finalize_gx = al_cdiv(NK, 4);
    k.plane = (size_t)(NK * 16 + 64) * 128;
    return k;
}

// Elements of every per-frame workspace buffer for HWp padded pixels, HWi input pixels and NK keypoints: the instance carves
// them at its capacities, sslam_aliked_debug_read bounds a read by the last frame's.
struct ALExtents {
    size_t ctrl, in_u8, fsrc, img, x1, x2, p3, off, t3, x3, p3cl, t3cl, p4cl, t4cl, p4, t4, x4, g2, g3, g4, g2cl, g3cl, g4cl;
    size_t s8, rnorm, g1cl, pre2, pre3, pre4, score, nms, bsum, cand, hist, kp_index, sel_keys;
    size_t kp_norm, kp_score, patch, h32, pos, sampled, feats, raw, out_xy, out_desc, out_score, out_n;
};

inline ALExtents al_extents(size_t HWp, size_t HWi, size_t NK) {
    ALExtents e{};
    e.ctrl = 1;
    e.in_u8 = HWi * 4;
    e.fsrc = 3 * HWi; e.img = 3 * HWp;
    e.x1 = 16 * HWp; e.x2 = 32 * HWp / 4;
    e.p3 = 32 * HWp / 64; e.off = 18 * HWp / 64;
    e.t3 = 64 * HWp / 64; e.x3 = 64 * HWp / 64;
    e.p3cl = 32 * HWp / 64; e.t3cl = 64 * HWp / 64;
    e.p4cl = 64 * HWp / 1024; e.t4cl = 128 * HWp / 1024;
    e.p4 = 64 * HWp / 1024; e.t4 = 128 * HWp / 1024; e.x4 = 128 * HWp / 1024;
    e.g2 = 32 * HWp / 4; e.g3 = 32 * HWp / 64; e.g4 = 32 * HWp / 1024;
    e.g2cl = 32 * HWp / 4; e.g3cl = 32 * HWp / 64; e.g4cl = 32 * HWp / 1024;
    e.s8 = 8 * HWp; e.rnorm = HWp; e.g1cl = 32 * HWp;
    e.pre2 = AGG_PRE * HWp / 4; e.pre3 = AGG_PRE * HWp / 64; e.pre4 = AGG_PRE * HWp / 1024;
    e.score = HWp; e.nms = HWp; e.bsum = 4096;
    e.cand = CAND_CAP; e.hist = HBINS;
    e.kp_index = SEL_CAP; e.sel_keys = SEL_CAP;
    e.kp_norm = 2 * NK + 64; e.kp_score = NK + 64;
    e.patch = (NK + 64) * 1152; e.h32 = SDDH_KSPLIT * (NK + 64) * 32; e.pos = NK * 32 + 64;
    e.sampled = (NK * 16 + 64) * 128; e.feats = (NK * 16 + 64) * 128;      // (the (hi, lo) fp16 planes of [rows][128])
    e.raw = SDDH_KSPLIT * (NK + 64) * 128;
    e.out_xy = 2 * NK; e.out_desc = NK * 128; e.out_score = NK;
    e.out_n = 16;
    return e;
}

}  // namespace sslam
