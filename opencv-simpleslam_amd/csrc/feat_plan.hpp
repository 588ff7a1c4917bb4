// feat_plan.hpp - what the host plans of the feature detectors (orb_plan.hpp, sift_plan.hpp, akaze_plan.hpp) and the KLT tracker
// share, written ONCE: the largest frame side, cvRound, the tile quotient, the per-call image refusal and fastAtan2's polynomial.
// Plain C++17 with no HIP include: tests/test_feat_plan.py compiles it with the host compiler and compares it with
// tests/orb_ref.py.  What stays per detector: its parameters and their refusals, its pyramid and capacities, its tables.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>

namespace sslam {

constexpr int FEAT_MAX_SIDE = 16384;

constexpr int feat_cdiv(int a, int b) { return (a + b - 1) / b; }      // (its own name: common.hpp has the launch code's cdiv)
inline int cv_round(double v) { return (int)std::nearbyint(v); }         // cvRound: half to even
inline int cv_roundf(float v) { return (int)std::nearbyintf(v); }

// fastAtan2's polynomial in degrees, the epsilon of its quotient, and degrees -> radians
struct FastAtan { float p1, p3, p5, p7, eps, deg2rad; };

inline FastAtan fast_atan_consts() {
    const float r2d = (float)(180 / 3.14159265358979323846);
    FastAtan k{};
    k.p1 = 0.9997878412794807f * r2d; k.p3 = -0.3258083974640975f * r2d;
    k.p5 = 0.1555786518463281f * r2d; k.p7 = -0.04432655554792128f * r2d;
    k.eps = (float)2.2204460492503131e-16;
    k.deg2rad = (float)(3.14159265358979323846 / 180.0);
    return k;
}

// the per-call refusal: an image larger than the instance (never clipped).  -> 0, or a non-zero code with the message written
inline int feat_check_image(int w, int h, int c, int max_w, int max_h, char* msg, size_t n) {
    if (c != 1 && c != 3 && c != 4) { std::snprintf(msg, n, "%d channels (want 1, 3 or 4)", c); return 1; }
    if (w < 1 || h < 1) { std::snprintf(msg, n, "frame size %dx%d", w, h); return 2; }
    if (w > max_w || h > max_h) { std::snprintf(msg, n, "frame %dx%d is larger than the instance's %dx%d", w, h, max_w, max_h); return 3; }
    return 0;
}

}  // namespace sslam
