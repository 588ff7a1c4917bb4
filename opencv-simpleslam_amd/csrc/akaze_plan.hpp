// akaze_plan.hpp - everything the host decides about an AKAZE instance and about one call on it, decided ONCE: the parameter
// refusals, the evolution levels with their sizes, esigma / etime / sigma_size, borders, plane offsets and tile counts, the FED
// step tables in the order they are taken, the Gaussian and scaled-Scharr taps, the gauss25 table, the float constants of the
// orientation, the capacities and which levels run their diffusion in one workgroup.  Plain C++17 with no HIP include:
// tests/test_akaze_plan.py compiles it with the host compiler and compares it with tests/akaze_ref.py.  akaze_kernels.hip
// launches from these fields and holds no size arithmetic of its own.  Semantics and what is unconfirmed without cv2:
// tests/akaze_ref.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "feat_plan.hpp"

namespace sslam {

constexpr int AKZ_DESCRIPTOR_MLDB = 5, AKZ_DIFF_PM_G2 = 1;     // cv2's values
constexpr int AKZ_MAX_OCTAVES = 8, AKZ_MAX_SUBLEVELS = 8, AKZ_MAX_LEVELS = AKZ_MAX_OCTAVES * AKZ_MAX_SUBLEVELS;
constexpr int AKZ_MAX_SIDE = FEAT_MAX_SIDE;
constexpr int AKZ_MAX_POINTS = 1 << 20;
constexpr int AKZ_MIN_OCTAVE_W = 80, AKZ_MIN_OCTAVE_H = 40;
constexpr int AKZ_DESC_BYTES = 61, AKZ_DESC_BITS = 486;
constexpr int AKZ_NBINS = 300;
constexpr int AKZ_TILE_W = 64, AKZ_TILE_H = 4;                 // a workgroup of 256: a wavefront along a row
// A level of at most AKZ_WG_PIXELS pixels (never level 0) runs its flow and ALL its FED steps in one workgroup of AKZ_WG_T threads
// with Lt and Lflow in LDS: 2 * 4 * 20 000 = 160 000 of the 163 840 bytes; a thread holds at most AKZ_WG_PER_THREAD pixels of a step.
constexpr int AKZ_WG_PIXELS = 20000, AKZ_WG_T = 1024, AKZ_WG_PER_THREAD = 20;
static_assert(AKZ_WG_T * AKZ_WG_PER_THREAD >= AKZ_WG_PIXELS && 8 * AKZ_WG_PIXELS <= 160 * 1024, "the one-workgroup level fits");
constexpr int AKZ_KP_GX = 1024;                                // workgroups of the per-keypoint launches, four wavefronts each
constexpr int AKZ_FIXED_LOG2 = 32;                             // the orientation and M-LDB sums: 64-bit integers at this scale
constexpr int AKZ_N_WINDOWS = 42, AKZ_ORI_SAMPLES = 109;
constexpr double AKZ_SOFFSET = 1.6, AKZ_DERIVATIVE_FACTOR = 1.5, AKZ_KCONTRAST_PERCENTILE = 0.7, AKZ_TAU_MAX = 0.25;

constexpr float AKZ_GAUSS25[7][7] = {
    {0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f},
    {0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f},
    {0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f},
    {0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f},
    {0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f},
    {0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f},
    {0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f}};

struct AkzParams {
    int descriptor_type = AKZ_DESCRIPTOR_MLDB, descriptor_size = 0, descriptor_channels = 3;
    double threshold = 0.001;
    int noct = 4, nol = 4, diffusivity = AKZ_DIFF_PM_G2, max_points = -1;
};

struct AkzLevel {
    int octave, sublevel, w, h, sigma_size, border;
    double esigma, etime;
    float size, radius, ratio, half, norm, wnorm, quat;        // 2 esigma df, esigma df, 2^octave, 0.5 (2^octave - 1), the Scharr taps, sigma_size^4
    long long off;                                             // first float of the level's plane in each per-level slab
    int fed_off, fed_n;                                        // its transition's steps in AkzFed::tau (level 0: none)
    int tx, ty;                                                // tiles over the level (0: no interior inside the border)
    int one_wg;                                                // the diffusion into this level runs in one workgroup
};

struct AkzPlan {
    int w, h, nlev, noct, interior;                            // interior: level 0 has pixels inside its border (else: no keypoint)
    AkzLevel lv[AKZ_MAX_LEVELS];
    long long plane_floats, tmp_floats;                        // the sum of the levels' planes; one full-size temporary
    int max_tiles;
};

struct AkzFed {                                                // of the parameters alone (not of the frame's size)
    int off[AKZ_MAX_LEVELS], n[AKZ_MAX_LEVELS];
    std::vector<float> tau;
    int total = 0;
};

struct AkzConsts {
    FastAtan atan;
    float win_step, pi3, two_pi, five_pi3;
    float img_div, kfallback, koctave;
};

// -> 0, or a non-zero code with the message written
inline int akz_check_params(const AkzParams& p, int max_w, int max_h, char* msg, size_t n) {
    if (p.descriptor_type != AKZ_DESCRIPTOR_MLDB) { std::snprintf(msg, n, "descriptor_type %d is not supported (only DESCRIPTOR_MLDB = %d)", p.descriptor_type, AKZ_DESCRIPTOR_MLDB); return 1; }
    if (p.descriptor_size != 0) { std::snprintf(msg, n, "descriptor_size %d is not supported (only 0: the full 486 bits)", p.descriptor_size); return 2; }
    if (p.descriptor_channels != 3) { std::snprintf(msg, n, "descriptor_channels %d is not supported (only 3)", p.descriptor_channels); return 3; }
    if (!(p.threshold > 0) || !std::isfinite(p.threshold)) { std::snprintf(msg, n, "threshold %g is not positive and finite", p.threshold); return 4; }
    if (p.noct < 1 || p.noct > AKZ_MAX_OCTAVES) { std::snprintf(msg, n, "nOctaves %d outside 1..%d", p.noct, AKZ_MAX_OCTAVES); return 5; }
    if (p.nol < 1 || p.nol > AKZ_MAX_SUBLEVELS) { std::snprintf(msg, n, "nOctaveLayers %d outside 1..%d", p.nol, AKZ_MAX_SUBLEVELS); return 6; }
    if (p.diffusivity != AKZ_DIFF_PM_G2) { std::snprintf(msg, n, "diffusivity %d is not supported (only DIFF_PM_G2 = %d)", p.diffusivity, AKZ_DIFF_PM_G2); return 7; }
    if (!(p.max_points == -1 || (p.max_points >= 1 && p.max_points <= AKZ_MAX_POINTS))) { std::snprintf(msg, n, "max_points %d is neither -1 nor in 1..%d", p.max_points, AKZ_MAX_POINTS); return 8; }
    if (max_w < 1 || max_w > AKZ_MAX_SIDE || max_h < 1 || max_h > AKZ_MAX_SIDE) { std::snprintf(msg, n, "frame size %dx%d outside 1..%d", max_w, max_h, AKZ_MAX_SIDE); return 9; }
    return 0;
}

inline void akz_scharr_taps(int s, float* norm, float* wnorm) {
    const double w = 10.0 / 3.0, nm = 1.0 / (2.0 * s * (w + 2.0));
    *norm = (float)nm; *wnorm = (float)(w * nm);
}

inline AkzPlan akz_plan(const AkzParams& p, int w, int h) {
    AkzPlan P{};
    P.w = w; P.h = h; P.tmp_floats = (long long)w * h;
    for (int i = 0; i < p.noct; ++i) {
        const int lw = w >> i, lh = h >> i;
        if (i > 0 && (lw < AKZ_MIN_OCTAVE_W || lh < AKZ_MIN_OCTAVE_H)) break;
        P.noct = i + 1;
        for (int j = 0; j < p.nol; ++j) {
            AkzLevel& L = P.lv[P.nlev];
            L.octave = i; L.sublevel = j; L.w = lw; L.h = lh;
            L.esigma = AKZ_SOFFSET * std::pow(2.0, (double)j / p.nol + i);
            L.etime = 0.5 * (L.esigma * L.esigma);
            L.sigma_size = cv_round(L.esigma * AKZ_DERIVATIVE_FACTOR / (1 << i));
            L.border = 2 * L.sigma_size + 1;
            L.size = (float)(2.0 * L.esigma * AKZ_DERIVATIVE_FACTOR); L.radius = (float)(L.esigma * AKZ_DERIVATIVE_FACTOR);
            L.ratio = (float)(1 << i); L.half = (float)(0.5 * ((1 << i) - 1));
            akz_scharr_taps(L.sigma_size, &L.norm, &L.wnorm);
            L.quat = (float)(L.sigma_size * L.sigma_size * L.sigma_size * L.sigma_size);
            L.off = P.plane_floats;
            P.plane_floats += (long long)lw * lh;
            const bool interior = lw > 2 * L.border && lh > 2 * L.border;
            L.tx = interior ? feat_cdiv(lw, AKZ_TILE_W) : 0; L.ty = interior ? feat_cdiv(lh, AKZ_TILE_H) : 0;
            P.max_tiles = std::max(P.max_tiles, L.tx * L.ty);
            L.one_wg = P.nlev > 0 && (long long)lw * lh <= AKZ_WG_PIXELS;
            ++P.nlev;
        }
    }
    P.interior = P.lv[0].tx > 0;
    return P;
}

inline bool akz_is_prime(int n) {
    if (n < 2) return false;
    for (int d = 2; d * d <= n; ++d)
        if (n % d == 0) return false;
    return true;
}

// the FED cycle of process time T, reordered by the kappa-cycle (`ordered` false: the cycle as computed)
inline std::vector<float> akz_fed_steps(double T, bool ordered = true) {
    const int n = (int)(std::ceil(std::sqrt(3.0 * T / AKZ_TAU_MAX + 0.25) - 0.5 - 1.0e-8) + 0.5);
    const double scale = 3.0 * T / (AKZ_TAU_MAX * (double)(n * (n + 1)));
    const double c = 1.0 / (4.0 * n + 2.0), d = scale * AKZ_TAU_MAX / 2.0;
    std::vector<float> tauh(n), out(n);
    for (int k = 0; k < n; ++k) {
        const double cs = std::cos(M_PI * (2.0 * k + 1.0) * c);
        tauh[k] = (float)(d / (cs * cs));
    }
    if (!ordered) return tauh;
    const int kappa = n / 2;
    int prime = n + 1;
    while (!akz_is_prime(prime)) ++prime;
    for (int k = 0, l = 0; l < n; ++k, ++l) {
        int index = ((k + 1) * kappa) % prime - 1;
        while (index >= n) { ++k; index = ((k + 1) * kappa) % prime - 1; }
        out[l] = tauh[index];
    }
    return out;
}

// the step tables of all nOctaves * nOctaveLayers transitions (a frame uses those of its levels)
inline AkzFed akz_fed(const AkzParams& p) {
    AkzFed F{};
    double prev = 0;
    int lvl = 0;
    for (int i = 0; i < p.noct; ++i)
        for (int j = 0; j < p.nol; ++j, ++lvl) {
            const double esigma = AKZ_SOFFSET * std::pow(2.0, (double)j / p.nol + i), etime = 0.5 * (esigma * esigma);
            F.off[lvl] = (int)F.tau.size(); F.n[lvl] = 0;
            if (lvl > 0) {
                const std::vector<float> t = akz_fed_steps(etime - prev);
                F.n[lvl] = (int)t.size();
                F.tau.insert(F.tau.end(), t.begin(), t.end());
            }
            prev = etime;
        }
    F.total = (int)F.tau.size();
    return F;
}

// gaussian_2D_convolution's kernel: ksize = ceil(2 (1 + (sigma - 0.8) / 0.3)) made odd, getGaussianKernel's taps in double
inline std::vector<float> akz_gauss_taps(double sigma) {
    int n = (int)std::ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3));
    n += 1 - n % 2;
    const double s2 = -0.5 / (sigma * sigma);
    std::vector<double> t(n);
    double sum = 0;
    for (int j = 0; j < n; ++j) { const double x = j - (n - 1) * 0.5; t[j] = std::exp(s2 * (x * x)); sum += t[j]; }
    const double inv = 1.0 / sum;
    std::vector<float> out(n);
    for (int j = 0; j < n; ++j) out[j] = (float)(t[j] * inv);
    return out;
}

inline AkzConsts akz_consts() {
    AkzConsts c{};
    c.atan = fast_atan_consts();
    c.win_step = 0.15f; c.pi3 = (float)(M_PI / 3); c.two_pi = (float)(2 * M_PI); c.five_pi3 = (float)(5 * M_PI / 3);
    c.img_div = 255.f; c.kfallback = 0.03f; c.koctave = 0.75f;
    return c;
}

// The capacities of an instance made for max_w x max_h.  A candidate is a strict 3 x 3 maximum of its level, so a level holds
// fewer than one per 4 pixels; the list holds one per 8 pixels of the frame (at least 1024) - a dense synthetic mosaic yields one
// per 20 - and the rows (refined keypoints before the quota; they bound the output) one per 16, or max(4 max_points, 16384) if
// that is less.  A positive override replaces either.  Exceeding one voids the frame.
inline void akz_capacities(const AkzParams& p, int max_w, int max_h, int cand_override, int kp_override, int* cand_cap, int* kp_cap) {
    const long long px = (long long)max_w * max_h;
    const long long c = cand_override > 0 ? cand_override : std::max(px / 8, 1024LL);
    long long k = std::max(px / 16, 1024LL);
    if (p.max_points > 0) k = std::min(k, std::max(4LL * p.max_points, 16384LL));
    if (kp_override > 0) k = kp_override;
    *cand_cap = (int)std::min(c, (long long)1 << 24);
    *kp_cap = (int)std::min(k, (long long)1 << 24);
}

// device bytes of an instance: five planes per level, five full-size temporaries, 20 bytes per candidate, 48 + 93 per row
inline long long akz_instance_bytes(const AkzParams& p, int max_w, int max_h, int cand_cap, int kp_cap) {
    const AkzPlan P = akz_plan(p, max_w, max_h);
    return 4 * (5 * P.plane_floats + 5 * P.tmp_floats) + 20LL * cand_cap + (48LL + 93LL) * kp_cap;
}

}  // namespace sslam
