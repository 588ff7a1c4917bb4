// sift_plan.hpp - everything the host decides about a SIFT instance and about one call on it, decided ONCE: the parameter
// refusals, the octave count, sizes and slab offsets, the per-layer sigmas and float32 tap tables, the integer contrast
// threshold, the candidate and row capacities, the tile table of the all-octave extrema launch, the fixed-point scale of the
// two histograms and the float constants (fastAtan2's are feat_plan.hpp's).  Plain C++17 with no HIP include: tests/test_sift_plan.py
// compiles it with the host compiler and compares it with tests/sift_ref.py.  sift_kernels.hip launches from these fields and
// holds no size arithmetic of its own.  Semantics and what is unconfirmed without cv2: tests/sift_ref.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "feat_plan.hpp"

namespace sslam {

constexpr int SIFT_MAX_OCTAVES = 16;
constexpr int SIFT_MAX_OCTAVE_LAYERS = 8;
constexpr int SIFT_MAX_LAYERS = SIFT_MAX_OCTAVE_LAYERS + 3;    // Gaussian layers per octave
constexpr int SIFT_MAX_SIDE = FEAT_MAX_SIDE;
constexpr int SIFT_MAX_FEATURES = 1 << 20;
constexpr int SIFT_IMG_BORDER = 5;
constexpr int SIFT_MAX_INTERP_STEPS = 5;
constexpr int SIFT_ORI_BINS = 36;
constexpr int SIFT_DESCR_WIDTH = 4, SIFT_DESCR_BINS = 8, SIFT_DESCR_LEN = 128;
constexpr int SIFT_TILE_W = 64, SIFT_TILE_H = 4;               // a workgroup of 256: a wavefront along a row
constexpr int SIFT_TAIL_T = 1024, SIFT_TAIL_PIXELS = 8192;    // octaves this small (never octave 0) are computed by one workgroup
constexpr int SIFT_KP_GX = 1024;                               // workgroups of the per-keypoint launches, four wavefronts each
// The two histograms are sums of 64-bit integers at this scale.  A contribution is at most a gradient magnitude
// (<= 255 sqrt 2 < 361) times a weight <= 1; with sigma <= 8 the descriptor radius is at most 240 (scl <= 8 * 2^1.5, radius
// 3 scl sqrt 2 * 2.5) and the orientation radius at most 102, so a bin gathers fewer than 481^2 * 361 < 2^27 and its sum stays
// below 2^59; at the default sigma it is 4 761 samples * 361 < 2^21 and the sum below 2^53.
constexpr int SIFT_HIST_SCALE_LOG2 = 32;
static_assert(481LL * 481 * 361 < (1LL << 27) && 27 + SIFT_HIST_SCALE_LOG2 < 63, "the histograms fit in 63 bits");

struct SiftParams {
    int nfeatures = 0, nol = 3;                                // nOctaveLayers
    double contrast = 0.04, edge = 10, sigma = 1.6;
};

struct SiftOctave {
    int w, h;
    long long goff, doff;          // first float of the octave's nol + 3 Gaussian planes / nol + 2 DoG planes in their slabs
    int tx, ty, tile_base;         // tiles over the octave, first tile index in the extrema launch (0 tiles: no interior)
};

struct SiftPlan {
    int w, h, nol, noct;           // the input size; noct octaves are computed
    int tail_first;                // octaves tail_first .. noct - 1 have at most SIFT_TAIL_PIXELS pixels: one launch computes them
    SiftOctave oc[SIFT_MAX_OCTAVES];
    long long gauss_floats, dog_floats, tmp_floats;    // tmp: the doubled image and the row pass's intermediate, each 4 w h
    int ext_tiles;
    int threshold;
};

struct SiftTaps {
    int n[SIFT_MAX_LAYERS], off[SIFT_MAX_LAYERS];      // table 0: the base blur, table i: layer i from layer i - 1
    double sigma[SIFT_MAX_LAYERS];
    std::vector<float> taps;
};

struct SiftConsts {
    FastAtan atan;
    float flt_epsilon;
    float img_scale, deriv_scale, second_scale, cross_scale;
};

// -> 0, or a non-zero code with the message written
inline int sift_check_params(const SiftParams& p, int max_w, int max_h, char* msg, size_t n) {
    if (p.nfeatures < 0 || p.nfeatures > SIFT_MAX_FEATURES) { std::snprintf(msg, n, "nfeatures %d outside 0..%d", p.nfeatures, SIFT_MAX_FEATURES); return 1; }
    if (p.nol < 1 || p.nol > SIFT_MAX_OCTAVE_LAYERS) { std::snprintf(msg, n, "nOctaveLayers %d outside 1..%d", p.nol, SIFT_MAX_OCTAVE_LAYERS); return 2; }
    if (!(p.contrast > 0) || !std::isfinite(p.contrast)) { std::snprintf(msg, n, "contrastThreshold %g is not positive", p.contrast); return 3; }
    if (!(p.edge > 0) || !std::isfinite(p.edge)) { std::snprintf(msg, n, "edgeThreshold %g is not positive", p.edge); return 4; }
    if (!(p.sigma > 0.5 && p.sigma <= 8)) { std::snprintf(msg, n, "sigma %g outside (0.5, 8]", p.sigma); return 5; }
    if (max_w < 1 || max_w > SIFT_MAX_SIDE || max_h < 1 || max_h > SIFT_MAX_SIDE) { std::snprintf(msg, n, "frame size %dx%d outside 1..%d", max_w, max_h, SIFT_MAX_SIDE); return 6; }
    return 0;
}

// nOctaves of a w x h input: cvRound(log2(min side of the doubled image) - 2) + 1 (firstOctave -1), none below 1
inline int sift_n_octaves(int w, int h) {
    const int n = cv_round(std::log((double)std::min(2 * w, 2 * h)) / std::log(2.0) - 2) + 1;
    return std::min(std::max(n, 0), SIFT_MAX_OCTAVES);
}

inline int sift_threshold(const SiftParams& p) { return (int)std::floor(0.5 * p.contrast / p.nol * 255); }

inline SiftPlan sift_plan(const SiftParams& p, int w, int h) {
    SiftPlan P{};
    P.w = w; P.h = h; P.nol = p.nol; P.threshold = sift_threshold(p);
    P.tmp_floats = 4LL * w * h;
    int ow = 2 * w, oh = 2 * h;
    const int n = sift_n_octaves(w, h);
    for (int o = 0; o < n && ow >= 1 && oh >= 1; ++o, ow /= 2, oh /= 2) {
        SiftOctave& O = P.oc[o];
        O.w = ow; O.h = oh;
        O.goff = P.gauss_floats; O.doff = P.dog_floats;
        const long long plane = (long long)ow * oh;
        P.gauss_floats += plane * (p.nol + 3);
        P.dog_floats += plane * (p.nol + 2);
        const bool interior = ow > 2 * SIFT_IMG_BORDER && oh > 2 * SIFT_IMG_BORDER;     // a side <= 10 yields nothing
        O.tx = interior ? feat_cdiv(ow, SIFT_TILE_W) : 0; O.ty = interior ? feat_cdiv(oh, SIFT_TILE_H) : 0;
        O.tile_base = P.ext_tiles;
        P.ext_tiles += O.tx * O.ty;
        P.noct = o + 1;
    }
    P.tail_first = P.noct;
    while (P.tail_first > 1 && (long long)P.oc[P.tail_first - 1].w * P.oc[P.tail_first - 1].h <= SIFT_TAIL_PIXELS) --P.tail_first;
    return P;
}

// the blur of each layer: sigma in double, ksize = cvRound(8 sigma + 1) | 1, getGaussianKernel's taps in double rounded to float32
inline SiftTaps sift_taps(const SiftParams& p) {
    SiftTaps T{};
    T.sigma[0] = std::sqrt(std::max(p.sigma * p.sigma - 1.0, 0.01));
    const double k = std::pow(2.0, 1.0 / p.nol);
    for (int i = 1; i < p.nol + 3; ++i) {
        const double prev = std::pow(k, (double)(i - 1)) * p.sigma, total = prev * k;
        T.sigma[i] = std::sqrt(total * total - prev * prev);
    }
    for (int i = 0; i < p.nol + 3; ++i) {
        const double s = T.sigma[i], s2 = -0.5 / (s * s);
        const int n = cv_round(s * 8 + 1) | 1;
        T.n[i] = n; T.off[i] = (int)T.taps.size();
        std::vector<double> t(n);
        double sum = 0;
        for (int j = 0; j < n; ++j) { const double x = j - (n - 1) * 0.5; t[j] = std::exp(s2 * (x * x)); sum += t[j]; }
        const double inv = 1.0 / sum;
        for (int j = 0; j < n; ++j) T.taps.push_back((float)(t[j] * inv));
    }
    return T;
}

inline SiftConsts sift_consts() {
    SiftConsts c{};
    c.atan = fast_atan_consts();
    c.flt_epsilon = 1.1920928955078125e-07f;
    c.img_scale = 1.0f / 255.0f;
    c.deriv_scale = c.img_scale * 0.5f; c.second_scale = c.img_scale; c.cross_scale = c.img_scale * 0.25f;
    return c;
}

// The capacities of an instance made for max_w x max_h.  Extrema have no NMS-style bound (ties are candidates), so the
// candidate list holds one per 32 pixels of the doubled frame (at least 1024) - a natural image yields about one per 200 -
// and the rows (keypoints after the orientation, before duplicates and the quota; they bound the output) the same, or
// max(4 nfeatures, 16384) if that is less.  A positive override replaces either.  Exceeding one voids the frame.
inline void sift_capacities(const SiftParams& p, int max_w, int max_h, int cand_override, int kp_override, int* cand_cap, int* kp_cap) {
    const long long px = 4LL * max_w * max_h;
    const long long c = cand_override > 0 ? cand_override : std::max(px / 32, 1024LL);
    long long k = c;
    if (p.nfeatures > 0) k = std::min(k, std::max(4LL * p.nfeatures, 16384LL));
    if (kp_override > 0) k = kp_override;
    *cand_cap = (int)std::min(c, (long long)1 << 26);
    *kp_cap = (int)std::min(k, (long long)1 << 26);
}

// device bytes of an instance: the Gaussian and DoG slabs, two temporaries, 208 bytes per candidate, 576 per row
inline long long sift_instance_bytes(const SiftParams& p, int max_w, int max_h, int cand_cap, int kp_cap) {
    const SiftPlan P = sift_plan(p, max_w, max_h);
    return 4 * (P.gauss_floats + P.dog_floats + 2 * P.tmp_floats) + 208LL * cand_cap + 576LL * kp_cap;
}

}  // namespace sslam
