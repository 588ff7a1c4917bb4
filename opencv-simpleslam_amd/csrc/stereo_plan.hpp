// stereo_plan.hpp - the host plan of the semi-global stereo matcher (stereo_kernels.hip): every decision that is not arithmetic on
// pixels.  Plain C++17, no HIP: tests/test_stereo_plan.py compiles it with the host compiler and compares it with
// tests/stereo_ref.py.  The constexpr functions (the path layout, the lane split) are also what the kernels call, so the layout the
// test checks IS the device's.
//   * parameter normalisation (cv2.StereoSGBM's defaults and clamps, as recalled)
//   * refusals with their messages, before any HIP call
//   * workspace extents: every piece of the instance's slab in the order the instance takes them
//   * launch splits: the lanes of a path's group, disparities per lane, the paths of a direction and where each starts
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace sslam {

constexpr int SGBM_MODE_SGBM = 0;
constexpr int SGBM_MAX_SIDE = 16384;
constexpr int SGBM_MAX_COST = 32767;
constexpr unsigned long long SGBM_MAX_WORKSPACE = 4ull << 30;
constexpr int SGBM_DIRECTIONS = 5;             // ->, <-, down, down-right, down-left
constexpr int SGBM_PATH_T = 256;               // threads of a path workgroup
enum { SGBM_STAGE_PF_LEFT = 0, SGBM_STAGE_PF_RIGHT = 1, SGBM_STAGE_C = 2, SGBM_STAGE_S = 3, SGBM_STAGE_RAW = 4, SGBM_STAGE_RIGHT = 5,
       SGBM_STAGE_CHECKED = 6 };

// ------------------------------------------------------------------------------------------------------------ normalisation
struct SgbmParams {
    int minD, D, bs, P1, P2, d12, uniq, ftzero, maxD, invalid;
};

constexpr SgbmParams sgbm_normalise(int minDisparity, int numDisparities, int blockSize, int P1, int P2, int disp12MaxDiff, int preFilterCap,
                                    int uniquenessRatio) {
    SgbmParams p{};
    p.minD = minDisparity; p.D = numDisparities; p.bs = blockSize;
    p.P1 = P1 > 0 ? P1 : 2;
    const int p2 = P2 > 0 ? P2 : 5;
    p.P2 = p2 > p.P1 + 1 ? p2 : p.P1 + 1;
    p.d12 = disp12MaxDiff > 0 ? disp12MaxDiff : 1;           // the left-right check always runs
    p.uniq = uniquenessRatio >= 0 ? uniquenessRatio : 10;
    p.ftzero = (preFilterCap > 15 ? preFilterCap : 15) | 1;
    p.maxD = p.minD + p.D;
    p.invalid = (p.minD - 1) * 16;
    return p;
}

// the Sobel plane spans 0 .. 2 ftzero, the intensity plane 0 .. 255; a plane's Birchfield-Tomasi cost is shifted right by 2
constexpr int sgbm_max_pixel_cost(const SgbmParams& p) { return ((2 * p.ftzero) >> 2) + (255 >> 2); }
constexpr int sgbm_max_block_cost(const SgbmParams& p) { return p.bs * p.bs * sgbm_max_pixel_cost(p); }

// ---------------------------------------------------------------------------------------------------------------- extents
// one piece of an instance's slab (geom_slab.hpp: Slab::take)
constexpr unsigned long long sgbm_piece(unsigned long long bytes) { return (bytes + 8 + 255) / 256 * 256; }

struct SgbmExtents {
    unsigned long long px;       // pixels of the largest image
    unsigned long long cols;     // computed columns of the largest image: max_w - maxD, 0 when none
    unsigned long long vol;      // elements of one cost volume [max_h][cols][D]
    unsigned long long bytes;    // the whole slab
};

constexpr SgbmExtents sgbm_extents(int max_w, int max_h, int maxD, int D) {
    SgbmExtents e{};
    e.px = (unsigned long long)max_w * (unsigned long long)max_h;
    e.cols = max_w > maxD ? (unsigned long long)(max_w - maxD) : 0ull;
    e.vol = (unsigned long long)max_h * e.cols * (unsigned long long)D;
    e.bytes = 2 * sgbm_piece(e.px * 4)             // staging of the host entry's two images, up to four channels
            + 2 * sgbm_piece(e.px)                 // grey planes of a 3- / 4-channel pair
            + 2 * sgbm_piece(e.px)                 // prefiltered planes
            + 3 * sgbm_piece(e.vol * 2)            // row sums, C, S (int16)
            + sgbm_piece((unsigned long long)max_h * e.cols * 4)      // the selection's (cost, d) key
            + 4 * sgbm_piece(e.px * 2);            // raw, right, checked, final (int16)
    return e;
}

// ---------------------------------------------------------------------------------------------------------------- refusals
inline int sgbm_check_create(int max_w, int max_h, int minDisparity, int numDisparities, int blockSize, int P1, int P2, int disp12MaxDiff,
                             int preFilterCap, int uniquenessRatio, int speckleWindowSize, int speckleRange, int mode, char* msg, size_t n) {
    (void)speckleRange;
    if (mode != SGBM_MODE_SGBM) { std::snprintf(msg, n, "mode %d is not built (only MODE_SGBM = 0)", mode); return 1; }
    if (speckleWindowSize > 0) { std::snprintf(msg, n, "speckleWindowSize %d: the speckle filter is not built (want 0)", speckleWindowSize); return 2; }
    if (minDisparity < 0) { std::snprintf(msg, n, "minDisparity %d < 0", minDisparity); return 3; }
    if (numDisparities < 16 || numDisparities > 256 || numDisparities % 16) {
        std::snprintf(msg, n, "numDisparities %d is not a multiple of 16 in 16..256", numDisparities); return 4;
    }
    if (blockSize < 1 || blockSize > 11 || blockSize % 2 == 0) { std::snprintf(msg, n, "blockSize %d is not odd in 1..11", blockSize); return 5; }
    if (preFilterCap < 0 || preFilterCap > 63) { std::snprintf(msg, n, "preFilterCap %d outside 0..63", preFilterCap); return 6; }
    if (uniquenessRatio > 100) { std::snprintf(msg, n, "uniquenessRatio %d > 100", uniquenessRatio); return 7; }
    if (max_w < 1 || max_w > SGBM_MAX_SIDE || max_h < 1 || max_h > SGBM_MAX_SIDE) {
        std::snprintf(msg, n, "image size %dx%d outside 1..%d", max_w, max_h, SGBM_MAX_SIDE); return 8;
    }
    const SgbmParams p = sgbm_normalise(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio);
    if ((long long)sgbm_max_block_cost(p) + (long long)p.P2 > SGBM_MAX_COST) {
        std::snprintf(msg, n, "P2 %d with blockSize %d: the largest block cost %d (= %d^2 x %d per pixel) + P2 exceeds %d", p.P2, p.bs,
                      sgbm_max_block_cost(p), p.bs, sgbm_max_pixel_cost(p), SGBM_MAX_COST);
        return 9;
    }
    const SgbmExtents e = sgbm_extents(max_w, max_h, p.maxD, p.D);
    if (e.bytes > SGBM_MAX_WORKSPACE) { std::snprintf(msg, n, "workspace of %llu bytes exceeds %llu", e.bytes, SGBM_MAX_WORKSPACE); return 10; }
    return 0;
}

inline int sgbm_check_image(int w, int h, int c, int max_w, int max_h, char* msg, size_t n) {
    if (c != 1 && c != 3 && c != 4) { std::snprintf(msg, n, "%d channels (want 1, 3 or 4)", c); return 1; }
    if (w < 1 || w > SGBM_MAX_SIDE || h < 1 || h > SGBM_MAX_SIDE) { std::snprintf(msg, n, "image size %dx%d outside 1..%d", w, h, SGBM_MAX_SIDE); return 2; }
    if (w > max_w || h > max_h) { std::snprintf(msg, n, "image %dx%d is larger than the instance's %dx%d", w, h, max_w, max_h); return 3; }
    return 0;
}

// ----------------------------------------------------------------------------------------------------------- launch splits
// A path is walked by a group of lanes that holds its running costs.  D is rounded up to a power of two Dp (16 .. 256) for the
// split: min(Dp, 64) lanes, Dp / lanes consecutive disparities each (1, 1, 1, 2, 4 for Dp = 16 .. 256), 256 / lanes paths per
// workgroup (a wave carries 4, 2 or 1 paths).  Slots d >= D (D = 48, 80, ...) hold the out-of-range value and touch no memory.
constexpr int sgbm_pow2(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : D <= 64 ? 64 : D <= 128 ? 128 : 256; }
constexpr int sgbm_group_lanes(int D) { return sgbm_pow2(D) < 64 ? sgbm_pow2(D) : 64; }
constexpr int sgbm_d_per_lane(int D) { return sgbm_pow2(D) / sgbm_group_lanes(D); }
constexpr int sgbm_paths_per_block(int D) { return SGBM_PATH_T / sgbm_group_lanes(D); }

// paths of one direction over an H x W1 region; every pixel lies on exactly one path of a direction
constexpr int sgbm_path_count(int dir, int H, int W1) { return dir < 2 ? H : (dir == 2 ? W1 : W1 + H - 1); }
constexpr int sgbm_path_blocks(int dir, int H, int W1, int D) {
    return (sgbm_path_count(dir, H, W1) + sgbm_paths_per_block(D) - 1) / sgbm_paths_per_block(D);
}

struct SgbmPath {
    int y0, x0;      // the border pixel the path starts from (x in computed columns)
    int dy, dx;
    int len;
};

constexpr SgbmPath sgbm_path(int dir, int p, int H, int W1) {
    SgbmPath q{};
    switch (dir) {
    case 0: q.y0 = p; q.x0 = 0; q.dy = 0; q.dx = 1; q.len = W1; break;
    case 1: q.y0 = p; q.x0 = W1 - 1; q.dy = 0; q.dx = -1; q.len = W1; break;
    case 2: q.y0 = 0; q.x0 = p; q.dy = 1; q.dx = 0; q.len = H; break;
    case 3:
        q.y0 = p < W1 ? 0 : p - W1 + 1; q.x0 = p < W1 ? p : 0; q.dy = 1; q.dx = 1;
        q.len = H - q.y0 < W1 - q.x0 ? H - q.y0 : W1 - q.x0;
        break;
    default:
        q.y0 = p < W1 ? 0 : p - W1 + 1; q.x0 = p < W1 ? p : W1 - 1; q.dy = 1; q.dx = -1;
        q.len = H - q.y0 < q.x0 + 1 ? H - q.y0 : q.x0 + 1;
        break;
    }
    return q;
}

}  // namespace sslam
