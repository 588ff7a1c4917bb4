// orb_plan.hpp - everything the host decides about an ORB instance and about one call on it, decided ONCE: the parameter
// refusals, the level scales, sizes, strides and slab offsets (interior and border), the per-level quotas, the `umax` table,
// the blur taps, the float constants of the response, the candidate capacities, the per-level tile tables of
// the all-level launches, the default sampling pattern.  Plain C++17 with no HIP include: tests/test_orb_plan.py compiles it
// with the host compiler and compares it with tests/orb_ref.py.  orb_kernels.hip launches from these fields and holds no
// size arithmetic of its own.  Semantics and what is unconfirmed without cv2: tests/orb_ref.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "feat_plan.hpp"

namespace sslam {

constexpr int ORB_MAX_LEVELS = 16;
constexpr int ORB_MAX_SIDE = FEAT_MAX_SIDE;
constexpr int ORB_MAX_FEATURES = 1 << 20;
constexpr int ORB_PATCH = 31, ORB_HALF = 15;   // patchSize and its half: the disc of the orientation, the pattern's range
constexpr int ORB_HARRIS_BLOCK = 7;
constexpr int ORB_REACH = 22;                  // ceil(15 sqrt 2): the reach of a rotated pattern point
constexpr int ORB_PATTERN_POINTS = 512;
constexpr int ORB_TILE_W = 32, ORB_TILE_H = 8; // the blur tile: a workgroup of 256, a stored pixel per lane
constexpr int ORB_FAST_W = 32, ORB_FAST_H = 32;// the FAST tile: four blur-sized strips, one append per workgroup
constexpr int ORB_SEL_T = 1024;                // the select workgroup, one per level
constexpr int ORB_SEL_K = 8;                   // ... and the keys a thread holds per turn
constexpr int ORB_RESP_GX = 32;                // response workgroups per level (grid-stride over the device count)
constexpr int ORB_DESC_GX = 512;               // describe workgroups per level, four keypoints (wavefronts) each

struct OrbParams {
    int nfeatures = 500;
    double scale_factor = 1.2;     // rounded to float32 first, as the Python binding of cv2 passes it
    int nlevels = 8, edge_threshold = 31, score_type = 0, fast_threshold = 20;
};

struct OrbLevel {
    int w, h;                      // interior
    int stride, rows;              // stored: w + 2 border, h + 2 border
    int active;                    // both sides >= 2 edgeThreshold + 1 (else: no storage, no keypoints; so is every later level)
    float scale;                   // (float)pow(scaleFactor, level)
    int quota;                     // nfeaturesPerLevel
    int cut1_n;                    // retainBest's n of the first cut: 2 quota (HARRIS_SCORE) or quota (FAST_SCORE)
    long long off;                 // byte offset of the stored level (border included) in the image slab and in the blur slab
    int fast_tx, fast_ty, fast_base;       // tiles over the interior, first tile index in the FAST launch
    int pad_tx, pad_ty, pad_base;          // tiles over the stored level, first tile index in the blur launch
    int cand_cap;                  // ceil(w / 2) ceil(h / 2): strict NMS leaves no two 8-adjacent survivors
    long long cand_off;            // first candidate of the level in the candidate arrays
};

struct OrbPlan {
    int w, h, nlevels, border;
    OrbLevel lv[ORB_MAX_LEVELS];
    int nactive;                   // levels 0 .. nactive - 1 are stored
    long long slab_bytes;          // one slab of all stored levels (the blurred slab has the same layout)
    long long cand_total;          // sum of cand_cap over the active levels = the bound on the output rows
    int fast_tiles, blur_tiles;
    int umax[ORB_HALF + 1];
    int gauss[7];
    float harris_k, harris_scale4;
    FastAtan atan;                 // fastAtan2's polynomial (feat_plan.hpp)
    float patch_size;
};

// -> 0, or a non-zero code with the message written
inline int orb_check_params(const OrbParams& p, int max_w, int max_h, char* msg, size_t n) {
    const double sf = (double)(float)p.scale_factor;
    if (p.nfeatures < 1 || p.nfeatures > ORB_MAX_FEATURES) { std::snprintf(msg, n, "nfeatures %d outside 1..%d", p.nfeatures, ORB_MAX_FEATURES); return 1; }
    if (!(sf > 1.0 && sf <= 2.0)) { std::snprintf(msg, n, "scaleFactor %g outside (1, 2]", p.scale_factor); return 2; }
    if (p.nlevels < 1 || p.nlevels > ORB_MAX_LEVELS) { std::snprintf(msg, n, "nlevels %d outside 1..%d", p.nlevels, ORB_MAX_LEVELS); return 3; }
    if (p.edge_threshold < 3 || p.edge_threshold > ORB_MAX_SIDE) { std::snprintf(msg, n, "edgeThreshold %d below 3 (the FAST circle)", p.edge_threshold); return 4; }
    if (p.score_type != 0 && p.score_type != 1) { std::snprintf(msg, n, "scoreType %d is neither HARRIS_SCORE (0) nor FAST_SCORE (1)", p.score_type); return 5; }
    if (p.fast_threshold < 1 || p.fast_threshold > 254) { std::snprintf(msg, n, "fastThreshold %d outside 1..254", p.fast_threshold); return 6; }
    if (max_w < 1 || max_w > ORB_MAX_SIDE || max_h < 1 || max_h > ORB_MAX_SIDE) { std::snprintf(msg, n, "frame size %dx%d outside 1..%d", max_w, max_h, ORB_MAX_SIDE); return 7; }
    return 0;
}

// a user pattern must stay inside the patch: the memory-safety argument of the descriptor rests on |x|, |y| <= 15
inline int orb_check_pattern(const int8_t* pat, char* msg, size_t n) {
    for (int i = 0; i < 2 * ORB_PATTERN_POINTS; ++i)
        if (pat[i] < -ORB_HALF || pat[i] > ORB_HALF) {
            std::snprintf(msg, n, "pattern point %d has coordinate %d outside -%d..%d", i / 2, (int)pat[i], ORB_HALF, ORB_HALF);
            return 8;
        }
    return 0;
}

inline int orb_border(int edge) { return std::max(std::max(edge, ORB_REACH), (ORB_HARRIS_BLOCK + 2) / 2) + 1; }

// makeRandomPattern(31, pattern, 512): cv::RNG(0x34985739), x then y of each point from uniform(-15, 16)
inline void orb_default_pattern(int8_t* out) {
    uint64_t state = 0x34985739ull;
    for (int i = 0; i < 2 * ORB_PATTERN_POINTS; ++i) {
        state = (uint64_t)(uint32_t)state * 4164903690ull + (uint32_t)(state >> 32);
        out[i] = (int8_t)((int)((uint32_t)state % (uint32_t)ORB_PATCH) - ORB_HALF);
    }
}

inline void orb_quotas(const OrbParams& p, int* out) {
    const float factor = (float)(1.0 / (double)(float)p.scale_factor);
    const float den = 1.0f - (float)std::pow((double)factor, (double)p.nlevels);
    float nd = (float)p.nfeatures * (1.0f - factor);
    nd = nd / den;
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; ++l) {
        out[l] = cv_roundf(nd);
        sum += out[l];
        nd = nd * factor;
    }
    out[p.nlevels - 1] = std::max(p.nfeatures - sum, 0);
}

inline OrbPlan orb_plan(const OrbParams& p, int w, int h) {
    OrbPlan P{};
    P.w = w; P.h = h; P.nlevels = p.nlevels; P.border = orb_border(p.edge_threshold);
    int quota[ORB_MAX_LEVELS];
    orb_quotas(p, quota);
    const double sf = (double)(float)p.scale_factor;
    const int need = 2 * p.edge_threshold + 1;
    bool alive = true;
    for (int l = 0; l < p.nlevels; ++l) {
        OrbLevel& L = P.lv[l];
        L.scale = (float)std::pow(sf, (double)l);
        const float inv = 1.0f / L.scale;
        L.w = cv_roundf((float)w * inv);
        L.h = cv_roundf((float)h * inv);
        L.quota = quota[l];
        L.cut1_n = p.score_type == 0 ? 2 * quota[l] : quota[l];
        alive = alive && L.w >= need && L.h >= need;
        L.active = alive;
        if (!alive) continue;
        L.stride = L.w + 2 * P.border; L.rows = L.h + 2 * P.border;
        L.off = P.slab_bytes;
        P.slab_bytes += ((long long)L.stride * L.rows + 255) / 256 * 256;
        L.fast_tx = feat_cdiv(L.w, ORB_FAST_W); L.fast_ty = feat_cdiv(L.h, ORB_FAST_H); L.fast_base = P.fast_tiles;
        P.fast_tiles += L.fast_tx * L.fast_ty;
        L.pad_tx = feat_cdiv(L.stride, ORB_TILE_W); L.pad_ty = feat_cdiv(L.rows, ORB_TILE_H); L.pad_base = P.blur_tiles;
        P.blur_tiles += L.pad_tx * L.pad_ty;
        L.cand_cap = feat_cdiv(L.w, 2) * feat_cdiv(L.h, 2);
        L.cand_off = P.cand_total;
        P.cand_total += L.cand_cap;
        P.nactive = l + 1;
    }
    // umax: the half-widths of the disc's rows, OpenCV's table with its symmetry fix-up
    const int vmax = (int)std::floor(ORB_HALF * std::sqrt(2.0) / 2 + 1), vmin = (int)std::ceil(ORB_HALF * std::sqrt(2.0) / 2);
    int um[ORB_HALF + 2] = {};
    for (int v = 0; v <= vmax; ++v) um[v] = cv_round(std::sqrt((double)ORB_HALF * ORB_HALF - (double)v * v));
    for (int v = ORB_HALF, v0 = 0; v >= vmin; --v) {
        while (um[v0] == um[v0 + 1]) ++v0;
        um[v] = v0;
        ++v0;
    }
    for (int v = 0; v <= ORB_HALF; ++v) P.umax[v] = um[v];
    // GaussianBlur 7x7 sigma 2 in 8 fractional bits, the centre tap takes the rounding remainder
    double g[7], gs = 0;
    for (int i = 0; i < 7; ++i) { g[i] = std::exp(-(double)((i - 3) * (i - 3)) / (2 * 2.0 * 2.0)); gs += g[i]; }
    int ks = 0;
    for (int i = 0; i < 7; ++i) { P.gauss[i] = cv_round(g[i] / gs * 256); ks += P.gauss[i]; }
    P.gauss[3] += 256 - ks;
    P.harris_k = 0.04f;
    const float hs = 1.0f / (float)(4 * ORB_HARRIS_BLOCK * 255);
    float s4 = hs * hs; s4 = s4 * hs; s4 = s4 * hs;
    P.harris_scale4 = s4;
    P.atan = fast_atan_consts();
    P.patch_size = (float)ORB_PATCH;
    return P;
}

// the bound on the output rows of any call on an instance made for max_w x max_h: every level's NMS bound (ties are never
// dropped, so nfeatures does not bound them)
inline long long orb_capacity(const OrbParams& p, int max_w, int max_h) { return std::max(orb_plan(p, max_w, max_h).cand_total, 1LL); }

}  // namespace sslam
