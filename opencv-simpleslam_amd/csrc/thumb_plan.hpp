// thumb_plan.hpp - the host plan of the keyframe-thumbnail pipeline (thumb_kernels.hip): every decision and every table that is
// not arithmetic on pixels.  Plain C++17, no HIP: tests/test_thumb_plan.py compiles it with the host compiler and compares it with
// tests/thumb_ref.py.  The constexpr functions (geometry, block layout, resize taps) are also what the kernels call - a constexpr
// function is callable from device code as it is - so the layout and the taps the test checks ARE the device's.
//   * refusals (quality, sizes, channels) with their messages, before any HIP call
//   * libjpeg's quantisation tables for a quality, the integer DCT matrix, the zigzag order, the Annex K Huffman tables as
//     (code, length) per symbol
//   * the geometry of one encode: MCU grid, padded planes, blocks in scan order, the dummy-block rule
//   * the header bytes (SOI .. SOS) and the capacity no encode can exceed
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace sslam {

constexpr int THUMB_MAX_DST = 4096;
constexpr int THUMB_MAX_SRC = 16384;
constexpr int THUMB_BLOCK_BITS = 20 + 63 * 26;                   // DC: 9-bit code + 11 bits; each AC: 16-bit code + 10 bits
constexpr int THUMB_BLOCK_WORDS = (THUMB_BLOCK_BITS + 31) / 32;  // 52 words = 208 bytes of bit buffer per block
constexpr int THUMB_BLOCK_BYTES = 2 * 4 * THUMB_BLOCK_WORDS;     // 416: every byte stuffed
constexpr int THUMB_CHUNK = 16;                                  // bytes of unstuffed scan per lane of the stuffing passes: one 16-byte load
enum { THUMB_STAGE_RESIZED = 0, THUMB_STAGE_Y = 1, THUMB_STAGE_CB = 2, THUMB_STAGE_CR = 3, THUMB_STAGE_COEF = 4, THUMB_STAGE_BITOFF = 5 };

// ---------------------------------------------------------------------------------------------------------------- refusals
inline int thumb_check_create(int max_src_w, int max_src_h, int dst_w, int dst_h, int quality, char* msg, size_t n) {
    if (quality < 1 || quality > 100) { std::snprintf(msg, n, "quality %d outside 1..100", quality); return 1; }
    if (dst_w < 1 || dst_w > THUMB_MAX_DST || dst_h < 1 || dst_h > THUMB_MAX_DST) {
        std::snprintf(msg, n, "thumbnail size %dx%d outside 1..%d", dst_w, dst_h, THUMB_MAX_DST); return 2;
    }
    if (max_src_w < 1 || max_src_w > THUMB_MAX_SRC || max_src_h < 1 || max_src_h > THUMB_MAX_SRC) {
        std::snprintf(msg, n, "source size %dx%d outside 1..%d", max_src_w, max_src_h, THUMB_MAX_SRC); return 3;
    }
    return 0;
}

inline int thumb_check_image(int ws, int hs, int c, int max_w, int max_h, char* msg, size_t n) {
    if (c != 1 && c != 3 && c != 4) { std::snprintf(msg, n, "%d channels (want 1, 3 or 4)", c); return 1; }
    if (ws < 1 || ws > THUMB_MAX_SRC || hs < 1 || hs > THUMB_MAX_SRC) {
        std::snprintf(msg, n, "source size %dx%d outside 1..%d", ws, hs, THUMB_MAX_SRC); return 2;
    }
    if (ws > max_w || hs > max_h) { std::snprintf(msg, n, "source %dx%d is larger than the instance's %dx%d", ws, hs, max_w, max_h); return 3; }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------ tables
constexpr uint8_t THUMB_LUMA_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t THUMB_CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                        47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// THUMB_ZIGZAG[i]: natural (row-major) index of the i-th coefficient in zigzag order
constexpr uint8_t THUMB_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr uint8_t THUMB_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t THUMB_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t THUMB_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// what the kernels read, uploaded once per instance.  Index 0: luma, 1: chroma.
struct ThumbTables {
    int32_t dct[64];             // M[k][n] = round(2^13 c_k / 2 cos((2n + 1) k pi / 16))
    uint16_t quant[2][64];       // natural order
    uint8_t zigzag_pos[64];      // natural index -> position in zigzag order
    uint16_t dc_code[2][12];
    uint8_t dc_len[2][12];
    uint16_t ac_code[2][256];    // by symbol (run << 4 | category); length 0: no such symbol
    uint8_t ac_len[2][256];
};

// libjpeg: jpeg_quality_scaling, then jpeg_add_quant_table with force_baseline; natural order
inline void thumb_quant_tables(int quality, uint16_t* luma, uint16_t* chroma) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (THUMB_LUMA_Q[i] * s + 50) / 100, c = (THUMB_CHROMA_Q[i] * s + 50) / 100;
        luma[i] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[i] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
}

// Annex C: canonical codes in the order of the value list
inline void thumb_huff_codes(const uint8_t* bits, const uint8_t* vals, uint16_t* code_of, uint8_t* len_of) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) { code_of[vals[k]] = (uint16_t)code++; len_of[vals[k]] = (uint8_t)len; }
        code <<= 1;
    }
}

inline ThumbTables thumb_tables(int quality) {
    ThumbTables T{};
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < 8; ++k)
        for (int n = 0; n < 8; ++n)
            T.dct[8 * k + n] = (int32_t)std::lround(8192.0 * (k == 0 ? 1.0 / std::sqrt(2.0) : 1.0) / 2 * std::cos((2 * n + 1) * k * pi / 16));
    thumb_quant_tables(quality, T.quant[0], T.quant[1]);
    for (int i = 0; i < 64; ++i) T.zigzag_pos[THUMB_ZIGZAG[i]] = (uint8_t)i;
    uint8_t dc_vals[12];
    for (int i = 0; i < 12; ++i) dc_vals[i] = (uint8_t)i;
    for (int t = 0; t < 2; ++t) {
        thumb_huff_codes(THUMB_DC_BITS[t], dc_vals, T.dc_code[t], T.dc_len[t]);
        thumb_huff_codes(THUMB_AC_BITS[t], THUMB_AC_VALS[t], T.ac_code[t], T.ac_len[t]);
    }
    return T;
}

// ---------------------------------------------------------------------------------------------------------------- geometry
// One encode at thumbnail size w x h.  ncomp 1: a one-channel source, 8 x 8 MCUs of one block; ncomp 3: Y Cb Cr at 4:2:0, 16 x 16
// MCUs of six blocks (Y00 Y01 Y10 Y11 Cb Cr).  Planes are padded to the MCU multiple by replicating the last column and row.
struct ThumbGeom {
    int w, h, ncomp;
    int mcux, mcuy;              // MCU grid
    int yw, yh;                  // the padded Y plane
    int cw, ch;                  // a padded chroma plane (0 x 0 for one component)
    int bw, bh;                  // the image's own block grid: ceil(w / 8) x ceil(h / 8)
    int blocks;
};

constexpr ThumbGeom thumb_geom(int w, int h, int channels) {
    ThumbGeom g{};
    g.w = w; g.h = h; g.ncomp = channels == 1 ? 1 : 3;
    const int mcu = g.ncomp == 1 ? 8 : 16;
    g.mcux = (w + mcu - 1) / mcu; g.mcuy = (h + mcu - 1) / mcu;
    g.yw = g.mcux * mcu; g.yh = g.mcuy * mcu;
    g.cw = g.ncomp == 1 ? 0 : g.mcux * 8; g.ch = g.ncomp == 1 ? 0 : g.mcuy * 8;
    g.bw = (w + 7) / 8; g.bh = (h + 7) / 8;
    g.blocks = g.mcux * g.mcuy * (g.ncomp == 1 ? 1 : 6);
    return g;
}

// libjpeg's dummy blocks: a Y block (8-pixel units of the padded plane) wholly beyond the image's own block grid
constexpr bool thumb_is_dummy(const ThumbGeom& g, int bx, int by) { return bx >= g.bw || by >= g.bh; }

struct ThumbBlock {
    int comp;                    // 0 Y, 1 Cb, 2 Cr
    int bx, by;                  // the block in its plane, 8-pixel units
    int dummy;                   // carries the DC of the preceding Y block of its MCU and no AC
    int sx, sy;                  // the block whose pixels give that DC (bx, by when not a dummy)
    int prev;                    // the preceding block of the same component in scan order, -1: none (predictor 0)
};

constexpr ThumbBlock thumb_block(const ThumbGeom& g, int b) {
    ThumbBlock k{};
    if (g.ncomp == 1) {
        k.bx = k.sx = b % g.mcux; k.by = k.sy = b / g.mcux; k.prev = b - 1;
        return k;
    }
    const int m = b / 6, i = b - 6 * m, mx = m % g.mcux, my = m / g.mcux;
    if (i >= 4) {
        k.comp = i - 3; k.bx = k.sx = mx; k.by = k.sy = my; k.prev = m ? b - 6 : -1;
        return k;
    }
    k.bx = 2 * mx + (i & 1); k.by = 2 * my + (i >> 1);
    int j = i;
    while (j > 0 && thumb_is_dummy(g, 2 * mx + (j & 1), 2 * my + (j >> 1))) --j;      // (block 0 of an MCU is never a dummy)
    k.dummy = j != i;
    k.sx = 2 * mx + (j & 1); k.sy = 2 * my + (j >> 1);
    k.prev = i ? b - 1 : (m ? b - 3 : -1);
    return k;
}

// One axis of cv2.resize's INTER_LINEAR taps for destination index d: s, the second tap min(s + 1, src - 1), and the weights at
// scale 2^11.  Every operation is one IEEE operation in the written order (thumb_kernels.hip switches contraction into fused
// multiply-adds off for its whole text).  floor and round-half-to-even are written out: both are exact here (|f| < 2^15, the
// product by 2048 is below 2^23) and stay constexpr.
constexpr int thumb_floor(double f) {
    const int s = (int)f;
    return (double)s > f ? s - 1 : s;
}
constexpr int thumb_rint(float x) {          // 0 <= x <= 2048
    const int i = (int)x;
    const float frac = x - (float)i;
    return frac > 0.5f || (frac == 0.5f && (i & 1)) ? i + 1 : i;
}
constexpr void thumb_tap(int d, int dst, int src, int* s0, int* s1, int* a0, int* a1) {
    const double p = ((double)d + 0.5) * ((double)src / (double)dst);
    const double f = p - 0.5;
    int s = thumb_floor(f);
    float ff = (float)(f - (double)s);
    if (s < 0) { s = 0; ff = 0.0f; }
    if (s >= src - 1) { s = src - 1; ff = 0.0f; }
    *s0 = s; *s1 = s + 1 < src ? s + 1 : src - 1;
    *a1 = thumb_rint(ff * 2048.0f);
    *a0 = thumb_rint((1.0f - ff) * 2048.0f);
}

// ------------------------------------------------------------------------------------------------------- header, capacity
inline void thumb_segment(std::vector<uint8_t>& out, int marker, const std::vector<uint8_t>& payload) {
    const size_t len = payload.size() + 2;
    out.push_back(0xFF); out.push_back((uint8_t)marker); out.push_back((uint8_t)(len >> 8)); out.push_back((uint8_t)len);
    out.insert(out.end(), payload.begin(), payload.end());
}

// SOI, APP0 (JFIF 1.01), DQT per table, SOF0, DHT per table (DC then AC, luma then chroma), SOS
inline std::vector<uint8_t> thumb_header(int w, int h, int ncomp, int quality) {
    uint16_t q[2][64];
    thumb_quant_tables(quality, q[0], q[1]);
    std::vector<uint8_t> out = {0xFF, 0xD8};
    thumb_segment(out, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    const int ntab = ncomp == 3 ? 2 : 1;
    for (int t = 0; t < ntab; ++t) {
        std::vector<uint8_t> p = {(uint8_t)t};
        for (int i = 0; i < 64; ++i) p.push_back((uint8_t)q[t][THUMB_ZIGZAG[i]]);
        thumb_segment(out, 0xDB, p);
    }
    std::vector<uint8_t> sof = {8, (uint8_t)(h >> 8), (uint8_t)h, (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)ncomp};
    for (int c = 0; c < ncomp; ++c) { sof.push_back((uint8_t)(c + 1)); sof.push_back(c == 0 && ncomp == 3 ? 0x22 : 0x11); sof.push_back(c ? 1 : 0); }
    thumb_segment(out, 0xC0, sof);
    for (int t = 0; t < ntab; ++t) {
        std::vector<uint8_t> dc = {(uint8_t)t};
        dc.insert(dc.end(), THUMB_DC_BITS[t], THUMB_DC_BITS[t] + 16);
        for (int i = 0; i < 12; ++i) dc.push_back((uint8_t)i);
        thumb_segment(out, 0xC4, dc);
        std::vector<uint8_t> ac = {(uint8_t)(0x10 | t)};
        ac.insert(ac.end(), THUMB_AC_BITS[t], THUMB_AC_BITS[t] + 16);
        ac.insert(ac.end(), THUMB_AC_VALS[t], THUMB_AC_VALS[t] + 162);
        thumb_segment(out, 0xC4, ac);
    }
    std::vector<uint8_t> sos = {(uint8_t)ncomp};
    for (int c = 0; c < ncomp; ++c) { sos.push_back((uint8_t)(c + 1)); sos.push_back(c ? 0x11 : 0x00); }
    sos.push_back(0); sos.push_back(63); sos.push_back(0);
    thumb_segment(out, 0xDA, sos);
    return out;
}

// bytes no encode at this size can exceed: the colour layout (the larger header, at least as many blocks), every block at its
// worst and every byte stuffed, EOI.  So there is no overflow word and nothing is ever truncated.
inline size_t thumb_capacity(int w, int h) {
    return thumb_header(w, h, 3, 50).size() + (size_t)THUMB_BLOCK_BYTES * (size_t)thumb_geom(w, h, 3).blocks + 2;
}

// chunks of THUMB_CHUNK unstuffed bytes the bit buffer of `blocks` blocks holds (13 per block, no remainder)
inline size_t thumb_chunks(int blocks) { return ((size_t)blocks * 4 * THUMB_BLOCK_WORDS + THUMB_CHUNK - 1) / THUMB_CHUNK; }

}  // namespace sslam
