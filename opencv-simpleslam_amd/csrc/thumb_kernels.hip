// thumb_kernels.hip - keyframe thumbnails: cv2.resize (INTER_LINEAR, uint8) and a baseline JPEG encoder on the device.
//
// Replaces `cv2.resize(bgr, hw)` + `cv2.imencode('.jpg', th, [IMWRITE_JPEG_QUALITY, q])` of slam/core/keyframe_utils.py:26-30.
// One encode is eight launches on the context's stream, nothing synchronises before the byte count is read:
//   * th_pixels_kernel<C>  a 2 x 2 quad of thumbnail pixels per lane: OpenCV's fixed-point bilinear taps (thumb_plan.hpp:
//                          thumb_tap; horizontal sums at scale 2^11, the vertical pass in its shifted form), libjpeg's integer
//                          Y Cb Cr, the quad's chroma average with bias 1, 2, 1, 2 along a row.  Planes are padded to the MCU
//                          multiple by clamping the pixel coordinate (= replicating the last column and row).  The resized image
//                          itself is written only for sslam_thumb_resize_host and the stage read.
//   * th_dct_kernel        a wave per 8 x 8 block, scan order: D = M (B - 128) M^T in integers at scale 2^26 (the first product
//                          fits int32, the second is int64), q = sign(D) ((|D| + (Q << 25)) / (Q << 26)), int16 in zigzag order.
//                          A dummy Y block transforms the block it copies and keeps the DC.  Each wave also zeroes its block's
//                          52 words of the bit buffer.
//   * th_bits_kernel       a wave per block: the length of its code, a lane per coefficient (ballot of the non-zero lanes gives
//                          each lane its zero run).
//   * th_scan_kernel       one workgroup: exclusive scan of the lengths -> bit offsets; pads the last byte with 1-bits.
//   * th_emit_kernel       a wave per block: the same codes, a wave prefix sum of their lengths, atomicOr of up to three words
//                          per lane into the big-endian bit buffer: bits of different lanes never overlap, so the result does not
//                          depend on the order.
//   * th_ff_count_kernel, th_scan_kernel, th_scatter_kernel: byte stuffing as a counted pass, a lane per 16-byte chunk (one
//                          vector load) of the part of the buffer the scan reaches; the last also copies the header in front,
//                          writes EOI behind and leaves the byte count.
// Wave size is 64 throughout.  PARITY UNPINNED: cv2 is absent here; tests/thumb_ref.py restates every stage, names what could not
// be confirmed, and tests/test_thumb_ref.py measures the streams against Pillow's libjpeg-turbo.
// (the resize taps of thumb_plan.hpp are defined operation by operation in double: no fused multiply-add anywhere in this file)
#pragma clang fp contract(off)
#include "common.hpp"
#include "thumb_plan.hpp"

using sslam::ThumbBlock;
using sslam::ThumbGeom;
using sslam::ThumbTables;

struct sslam_thumb {
    sslam_ctx* ctx = nullptr;
    int max_w = 0, max_h = 0, w = 0, h = 0, quality = 0;
    size_t capacity = 0;
    int max_blocks = 0;
    sslam::OwnedSlab slab;
    ThumbTables* tables = nullptr;
    uint8_t* hdr[2] = {nullptr, nullptr};    // [0]: one component, [1]: three
    int hdr_len[2] = {0, 0};
    uint8_t* src = nullptr;                  // staging of the host entries' source [max_h][max_w][4]
    uint8_t* img = nullptr;                  // the resized image [h][w][4], written on request only
    uint8_t *Y = nullptr, *Cb = nullptr, *Cr = nullptr;
    int16_t* coef = nullptr;                 // [blocks][64]
    uint32_t *blockbits = nullptr, *bitoff = nullptr, *bitbuf = nullptr, *ffcount = nullptr, *ffoff = nullptr;
    uint32_t* meta = nullptr;                // [0]: bits of the scan, [1]: 0xFF bytes in it
    uint8_t* out = nullptr;                  // the host entry's stream [capacity]
    int32_t* nbytes = nullptr;
    const uint8_t* last_src = nullptr;       // the last encode's source (for the stage read of the resized image)
    int last_hs = 0, last_ws = 0, last_c = 0;
};

namespace {

constexpr int TH_T = 256;
constexpr int TH_WAVE = 64;

template <int C>
__global__ __launch_bounds__(TH_T)
void th_pixels_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, ThumbGeom g, uint8_t* __restrict__ img,
                      uint8_t* __restrict__ Y, uint8_t* __restrict__ Cb, uint8_t* __restrict__ Cr) {
    const int qx = blockIdx.x * 32 + (threadIdx.x & 31), qy = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (qx >= g.yw / 2 || qy >= g.yh / 2) return;
    int xs0[2], xs1[2], xa0[2], xa1[2], ys0[2], ys1[2], yb0[2], yb1[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sslam::thumb_tap(min(2 * qx + i, g.w - 1), g.w, Ws, &xs0[i], &xs1[i], &xa0[i], &xa1[i]);
        sslam::thumb_tap(min(2 * qy + i, g.h - 1), g.h, Hs, &ys0[i], &ys1[i], &yb0[i], &yb1[i]);
    }
    int sum_cb = 0, sum_cr = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint8_t* r0 = src + (size_t)ys0[j] * Ws * C;      // every tap index is inside the source (thumb_tap clamps)
        const uint8_t* r1 = src + (size_t)ys1[j] * Ws * C;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int h0 = (int)r0[(size_t)xs0[i] * C + c] * xa0[i] + (int)r0[(size_t)xs1[i] * C + c] * xa1[i];
                const int h1 = (int)r1[(size_t)xs0[i] * C + c] * xa0[i] + (int)r1[(size_t)xs1[i] * C + c] * xa1[i];
                v[c] = min(max((((yb0[j] * (h0 >> 4)) >> 16) + ((yb1[j] * (h1 >> 4)) >> 16) + 2) >> 2, 0), 255);
            }
            const int X = 2 * qx + i, Yr = 2 * qy + j;
            if (img != nullptr && X < g.w && Yr < g.h) {
#pragma unroll
                for (int c = 0; c < C; ++c) img[((size_t)Yr * g.w + X) * C + c] = (uint8_t)v[c];
            }
            if (Y != nullptr) {
                if constexpr (C == 1) {
                    Y[(size_t)Yr * g.yw + X] = (uint8_t)v[0];
                } else {
                    const int B = v[0], G = v[1], R = v[2];
                    Y[(size_t)Yr * g.yw + X] = (uint8_t)((19595 * R + 38470 * G + 7471 * B + 32768) >> 16);
                    sum_cb += (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                    sum_cr += (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                }
            }
        }
    }
    if constexpr (C != 1) {
        if (Y != nullptr) {
            const int bias = 1 + (qx & 1);
            Cb[(size_t)qy * g.cw + qx] = (uint8_t)((sum_cb + bias) >> 2);
            Cr[(size_t)qy * g.cw + qx] = (uint8_t)((sum_cr + bias) >> 2);
        }
    }
}

// a wave per block; four blocks per workgroup (every lane reaches both barriers)
__global__ __launch_bounds__(TH_T)
void th_dct_kernel(ThumbGeom g, const ThumbTables* __restrict__ T, const uint8_t* __restrict__ Y, const uint8_t* __restrict__ Cb,
                   const uint8_t* __restrict__ Cr, int16_t* __restrict__ coef, uint32_t* __restrict__ bitbuf) {
    __shared__ int s_in[4][64];
    __shared__ int s_t[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const int b = blockIdx.x * 4 + wave;
    const bool live = b < g.blocks;
    ThumbBlock k{};
    if (live) {
        k = sslam::thumb_block(g, b);
        const uint8_t* plane = k.comp == 0 ? Y : (k.comp == 1 ? Cb : Cr);
        const int stride = k.comp == 0 ? g.yw : g.cw;
        s_in[wave][lane] = (int)plane[(size_t)(8 * k.sy + r) * stride + 8 * k.sx + c] - 128;
        if (lane < sslam::THUMB_BLOCK_WORDS) bitbuf[(size_t)b * sslam::THUMB_BLOCK_WORDS + lane] = 0u;
    }
    __syncthreads();
    if (live) {
        int acc = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc += T->dct[8 * r + n] * s_in[wave][8 * n + c];        // |acc| < 2^23
        s_t[wave][lane] = acc;
    }
    __syncthreads();
    if (!live) return;
    long long D = 0;
#pragma unroll
    for (int n = 0; n < 8; ++n) D += (long long)s_t[wave][8 * r + n] * (long long)T->dct[8 * c + n];
    const long long Q = (long long)T->quant[k.comp ? 1 : 0][lane];
    const long long mag = ((D < 0 ? -D : D) + (Q << 25)) / (Q << 26);
    int q = (int)(D < 0 ? -mag : mag);
    if (k.dummy && lane != 0) q = 0;
    coef[(size_t)b * 64 + T->zigzag_pos[lane]] = (int16_t)q;
}

// The code of one lane of a block's wave.  Lane 0: the DC difference `v`; lanes 1..63: the coefficient `v` with the zero run in
// front of it (ZRLs first); lane 63 with v == 0: the EOB.  nz: the ballot of the non-zero coefficients.  At most 3 * 11 + 16 + 10
// = 59 bits.
struct ThLaneCode { uint64_t code; int len; };

__device__ __forceinline__ ThLaneCode th_lane_code(const ThumbTables* __restrict__ T, int t, int lane, int v, uint64_t nz) {
    ThLaneCode o{0, 0};
    const int mag = v < 0 ? -v : v;
    const int cat = mag ? 32 - __clz(mag) : 0;
    const uint64_t vb = (uint64_t)((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u));
    if (lane == 0) {
        o.code = ((uint64_t)T->dc_code[t][cat] << cat) | vb;
        o.len = T->dc_len[t][cat] + cat;
    } else if (v != 0) {
        const uint64_t below = nz & ((1ull << lane) - 1ull) & ~1ull;
        const int prev = below ? 63 - __clzll((long long)below) : 0;
        const int run = lane - 1 - prev;
        const int zl = T->ac_len[t][0xF0];
        for (int z = run >> 4; z > 0; --z) { o.code = (o.code << zl) | T->ac_code[t][0xF0]; o.len += zl; }
        const int sym = ((run & 15) << 4) | cat;
        const int sl = T->ac_len[t][sym];
        o.code = (((o.code << sl) | T->ac_code[t][sym]) << cat) | vb;
        o.len += sl + cat;
    } else if (lane == 63) {
        o.code = T->ac_code[t][0];
        o.len = T->ac_len[t][0];
    }
    return o;
}

// the block's coefficient of this lane, lane 0 as the difference to the preceding block of the component
__device__ __forceinline__ int th_lane_value(const ThumbGeom& g, const int16_t* __restrict__ coef, int b, int lane, int* table) {
    const ThumbBlock k = sslam::thumb_block(g, b);
    *table = k.comp ? 1 : 0;
    int v = coef[(size_t)b * 64 + lane];
    if (lane == 0 && k.prev >= 0) v -= coef[(size_t)k.prev * 64];
    return v;
}

__global__ __launch_bounds__(TH_T)
void th_bits_kernel(ThumbGeom g, const ThumbTables* __restrict__ T, const int16_t* __restrict__ coef, uint32_t* __restrict__ blockbits) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= g.blocks) return;                               // (a whole wave)
    int t;
    const int v = th_lane_value(g, coef, b, lane, &t);
    const uint64_t nz = __ballot(v != 0);
    int x = th_lane_code(T, t, lane, v, nz).len;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, TH_WAVE);
    if (lane == 0) blockbits[b] = (uint32_t)x;
}

// One workgroup: out[i] = sum of in[0 .. i), *total = the whole sum.  pad != NULL: the sum is the scan's length in bits and the
// rest of its last byte is filled with 1-bits (the buffer was zeroed before; the codes are OR-ed in later).  bits != NULL: only
// the chunks that *bits bits of scan reach are summed (the stuffing passes: n is the worst case, the scan is a few percent of it).
constexpr int TH_SCAN_T = 1024;
__global__ __launch_bounds__(TH_SCAN_T)
void th_scan_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int n, uint32_t* __restrict__ total, uint32_t* pad,
                    const uint32_t* __restrict__ bits) {
    if (bits != nullptr) n = min(n, (int)(((((size_t)*bits + 7) >> 3) + sslam::THUMB_CHUNK - 1) / sslam::THUMB_CHUNK));
    __shared__ uint32_t s[TH_SCAN_T];
    const int tid = threadIdx.x;
    const int per = (n + TH_SCAN_T - 1) / TH_SCAN_T;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    uint32_t mine = 0;
    for (int i = lo; i < hi; ++i) mine += in[i];
    s[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TH_SCAN_T; d <<= 1) {
        const uint32_t y = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += y;
        __syncthreads();
    }
    uint32_t run = s[tid] - mine;
    for (int i = lo; i < hi; ++i) { const uint32_t x = in[i]; out[i] = run; run += x; }
    if (tid == TH_SCAN_T - 1) {
        const uint32_t sum = s[tid];
        *total = sum;
        if (pad != nullptr && (sum & 7u)) {
            const uint32_t p = sum & 31u, nb = 8u - (sum & 7u);          // p + nb <= 32
            atomicOr(&pad[sum >> 5], ((1u << nb) - 1u) << (32u - p - nb));
        }
    }
}

__global__ __launch_bounds__(TH_T)
void th_emit_kernel(ThumbGeom g, const ThumbTables* __restrict__ T, const int16_t* __restrict__ coef,
                    const uint32_t* __restrict__ bitoff, uint32_t* __restrict__ bitbuf) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= g.blocks) return;
    int t;
    const int v = th_lane_value(g, coef, b, lane, &t);
    const uint64_t nz = __ballot(v != 0);
    const ThLaneCode lc = th_lane_code(T, t, lane, v, nz);
    int x = lc.len;
#pragma unroll
    for (int d = 1; d < TH_WAVE; d <<= 1) {
        const int y = __shfl_up(x, d, TH_WAVE);
        if (lane >= d) x += y;
    }
    if (lc.len == 0) return;
    const uint32_t pos = bitoff[b] + (uint32_t)(x - lc.len);
    const uint32_t sh = pos & 31u;
    const uint64_t left = lc.code << (64 - lc.len);          // the code's first bit at bit 63
    const uint64_t hi = left >> sh;
    const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi, w2 = sh ? (uint32_t)((left << (64u - sh)) >> 32) : 0u;
    // a word beyond the first is touched only where the code has bits in it, so every index stays inside the blocks' own words
    uint32_t* wp = bitbuf + (pos >> 5);
    if (w0) atomicOr(wp, w0);
    if (w1) atomicOr(wp + 1, w1);
    if (w2) atomicOr(wp + 2, w2);
}

// byte `i` (0..15) of a 16-byte chunk of the big-endian bit buffer
__device__ __forceinline__ uint32_t th_byte(const uint4& c, int i) {
    const uint32_t w = i < 8 ? (i < 4 ? c.x : c.y) : (i < 12 ? c.z : c.w);
    return (w >> (24u - 8u * (uint32_t)(i & 3))) & 0xFFu;
}

// a lane per 16-byte chunk the scan reaches (bytes behind the scan's end are zero: the buffer was zeroed, so they count nothing)
__global__ __launch_bounds__(TH_T)
void th_ff_count_kernel(const uint32_t* __restrict__ bitbuf, const uint32_t* __restrict__ meta, size_t chunks,
                        uint32_t* __restrict__ ffcount) {
    const size_t k = (size_t)blockIdx.x * TH_T + threadIdx.x;
    const size_t nbytes = ((size_t)meta[0] + 7) >> 3;
    if (k >= chunks || k * sslam::THUMB_CHUNK >= nbytes) return;
    const uint4 c = reinterpret_cast<const uint4*>(bitbuf)[k];
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < sslam::THUMB_CHUNK; ++i) n += th_byte(c, i) == 0xFFu;
    ffcount[k] = n;
}

__global__ __launch_bounds__(TH_T)
void th_scatter_kernel(const uint32_t* __restrict__ bitbuf, const uint32_t* __restrict__ meta, const uint32_t* __restrict__ ffoff,
                       size_t chunks, const uint8_t* __restrict__ hdr, int hdr_len, uint8_t* __restrict__ out,
                       int32_t* __restrict__ nbytes_out) {
    const size_t k = (size_t)blockIdx.x * TH_T + threadIdx.x;
    const size_t nbytes = ((size_t)meta[0] + 7) >> 3;
    if (k < (size_t)hdr_len) out[k] = hdr[k];
    if (k == 0) {
        const size_t end = (size_t)hdr_len + nbytes + meta[1];
        out[end] = 0xFF; out[end + 1] = 0xD9;
        *nbytes_out = (int32_t)(end + 2);
    }
    const size_t lo = k * sslam::THUMB_CHUNK;
    if (k >= chunks || lo >= nbytes) return;
    const int cnt = (int)min((size_t)sslam::THUMB_CHUNK, nbytes - lo);
    const uint4 c = reinterpret_cast<const uint4*>(bitbuf)[k];
    uint8_t* o = out + hdr_len + lo + ffoff[k];
#pragma unroll
    for (int i = 0; i < sslam::THUMB_CHUNK; ++i) {
        if (i < cnt) {
            const uint32_t v = th_byte(c, i);
            *o++ = (uint8_t)v;
            if (v == 0xFFu) *o++ = 0;
        }
    }
}

int th_refuse(const char* who, const char* msg) {
    sslam::set_error("%s: %s", who, msg);
    return 2;
}

int th_check_image(const char* who, sslam_thumb* t, const void* src, int Hs, int Ws, int C) {
    SSLAM_REQUIRE(t != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(src != nullptr, "%s: NULL argument", who);
    char msg[160];
    if (sslam::thumb_check_image(Ws, Hs, C, t->max_w, t->max_h, msg, sizeof msg)) return th_refuse(who, msg);
    return 0;
}

// the resize and, with planes, the colour conversion; img may be NULL
int th_enqueue_pixels(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* img, bool planes) {
    const ThumbGeom g = sslam::thumb_geom(t->w, t->h, C);
    const dim3 grid((unsigned)sslam::cdiv(g.yw / 2, 32), (unsigned)sslam::cdiv(g.yh / 2, 8)), block(TH_T);
    hipStream_t s = t->ctx->stream;
    uint8_t *Y = planes ? t->Y : nullptr, *Cb = planes ? t->Cb : nullptr, *Cr = planes ? t->Cr : nullptr;
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (C == 1) hipLaunchKernelGGL(th_pixels_kernel<1>, grid, block, 0, s, src, Hs, Ws, g, img, Y, Cb, Cr);
    else if (C == 3) hipLaunchKernelGGL(th_pixels_kernel<3>, grid, block, 0, s, src, Hs, Ws, g, img, Y, Cb, Cr);
    else hipLaunchKernelGGL(th_pixels_kernel<4>, grid, block, 0, s, src, Hs, Ws, g, img, Y, Cb, Cr);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

int th_enqueue_encode(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* out, int32_t* nbytes) {
    if (int rc = th_enqueue_pixels(t, src, Hs, Ws, C, nullptr, true)) return rc;
    const ThumbGeom g = sslam::thumb_geom(t->w, t->h, C);
    hipStream_t s = t->ctx->stream;
    const dim3 waves((unsigned)sslam::cdiv(g.blocks, 4)), block(TH_T);
    const size_t chunks = sslam::thumb_chunks(g.blocks);
    const int hsel = g.ncomp == 3 ? 1 : 0;
    const dim3 bytes_grid((unsigned)((std::max(chunks, (size_t)t->hdr_len[hsel]) + TH_T - 1) / TH_T));
    hipLaunchKernelGGL(th_dct_kernel, waves, block, 0, s, g, t->tables, t->Y, t->Cb, t->Cr, t->coef, t->bitbuf);
    hipLaunchKernelGGL(th_bits_kernel, waves, block, 0, s, g, t->tables, t->coef, t->blockbits);
    hipLaunchKernelGGL(th_scan_kernel, dim3(1), dim3(TH_SCAN_T), 0, s, t->blockbits, t->bitoff, g.blocks, t->meta, t->bitbuf, (const uint32_t*)nullptr);
    hipLaunchKernelGGL(th_emit_kernel, waves, block, 0, s, g, t->tables, t->coef, t->bitoff, t->bitbuf);
    hipLaunchKernelGGL(th_ff_count_kernel, bytes_grid, block, 0, s, t->bitbuf, t->meta, chunks, t->ffcount);
    hipLaunchKernelGGL(th_scan_kernel, dim3(1), dim3(TH_SCAN_T), 0, s, t->ffcount, t->ffoff, (int)chunks, t->meta + 1, (uint32_t*)nullptr, (const uint32_t*)t->meta);
    hipLaunchKernelGGL(th_scatter_kernel, bytes_grid, block, 0, s, t->bitbuf, t->meta, t->ffoff, chunks, t->hdr[hsel], t->hdr_len[hsel], out, nbytes);
    SSLAM_HIP_CHECK(hipGetLastError());
    t->last_src = src; t->last_hs = Hs; t->last_ws = Ws; t->last_c = C;
    return 0;
}

}  // namespace

extern "C" int sslam_thumb_create(sslam_ctx* ctx, int max_src_w, int max_src_h, int dst_w, int dst_h, int quality, sslam_thumb** out) {
    const char* who = "sslam_thumb_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    char msg[160];
    if (sslam::thumb_check_create(max_src_w, max_src_h, dst_w, dst_h, quality, msg, sizeof msg)) return th_refuse(who, msg);
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<sslam_thumb> t(new sslam_thumb);
    t->ctx = ctx; t->max_w = max_src_w; t->max_h = max_src_h; t->w = dst_w; t->h = dst_h; t->quality = quality;
    t->capacity = sslam::thumb_capacity(dst_w, dst_h);
    const ThumbGeom g3 = sslam::thumb_geom(dst_w, dst_h, 3), g1 = sslam::thumb_geom(dst_w, dst_h, 1);
    t->max_blocks = std::max(g3.blocks, g1.blocks);
    const std::vector<uint8_t> h1 = sslam::thumb_header(dst_w, dst_h, 1, quality), h3 = sslam::thumb_header(dst_w, dst_h, 3, quality);
    t->hdr_len[0] = (int)h1.size(); t->hdr_len[1] = (int)h3.size();
    const size_t nb = (size_t)t->max_blocks, chunks = sslam::thumb_chunks(t->max_blocks);
    const size_t ypix = (size_t)std::max(g3.yw, g1.yw) * std::max(g3.yh, g1.yh);
    if (int rc = t->slab.alloc(who, false, [&](sslam::Slab& S) {
            t->tables = S.take<ThumbTables>(1);
            t->hdr[0] = S.take<uint8_t>(h1.size());
            t->hdr[1] = S.take<uint8_t>(h3.size());
            t->src = S.take<uint8_t>((size_t)max_src_w * max_src_h * 4);
            t->img = S.take<uint8_t>((size_t)dst_w * dst_h * 4);
            t->Y = S.take<uint8_t>(ypix);
            t->Cb = S.take<uint8_t>((size_t)g3.cw * g3.ch);
            t->Cr = S.take<uint8_t>((size_t)g3.cw * g3.ch);
            t->coef = S.take<int16_t>(nb * 64);
            t->blockbits = S.take<uint32_t>(nb);
            t->bitoff = S.take<uint32_t>(nb);
            t->bitbuf = S.take<uint32_t>(nb * sslam::THUMB_BLOCK_WORDS);
            t->ffcount = S.take<uint32_t>(chunks);
            t->ffoff = S.take<uint32_t>(chunks);
            t->meta = S.take<uint32_t>(4);
            t->out = S.take<uint8_t>(t->capacity);
            t->nbytes = S.take<int32_t>(1);
        })) return rc;
    const ThumbTables T = sslam::thumb_tables(quality);
    SSLAM_HIP_CHECK(hipMemcpy(t->tables, &T, sizeof T, hipMemcpyHostToDevice));
    SSLAM_HIP_CHECK(hipMemcpy(t->hdr[0], h1.data(), h1.size(), hipMemcpyHostToDevice));
    SSLAM_HIP_CHECK(hipMemcpy(t->hdr[1], h3.data(), h3.size(), hipMemcpyHostToDevice));
    sslam::ctx_retain(ctx);
    *out = t.release();
    return 0;
}

extern "C" int sslam_thumb_destroy(sslam_thumb* t) {
    return sslam::destroy_instance(t);
}

extern "C" int sslam_thumb_capacity(sslam_thumb* t, int* capacity) {
    SSLAM_REQUIRE(t != nullptr && capacity != nullptr, "sslam_thumb_capacity: NULL argument");
    *capacity = (int)t->capacity;
    return 0;
}

extern "C" int sslam_thumb_encode_dev(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* out, int32_t* nbytes) {
    const char* who = "sslam_thumb_encode_dev";
    if (int rc = th_check_image(who, t, src, Hs, Ws, C)) return rc;
    SSLAM_REQUIRE(out != nullptr && nbytes != nullptr, "%s: NULL argument", who);
    SSLAM_HIP_CHECK(hipSetDevice(t->ctx->device));
    return th_enqueue_encode(t, src, Hs, Ws, C, out, nbytes);
}

extern "C" int sslam_thumb_encode_host(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* out, int cap, int* nbytes) {
    const char* who = "sslam_thumb_encode_host";
    if (int rc = th_check_image(who, t, src, Hs, Ws, C)) return rc;
    SSLAM_REQUIRE(out != nullptr && nbytes != nullptr, "%s: NULL argument", who);
    SSLAM_HIP_CHECK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, t->src, src, (size_t)Hs * Ws * C));
    if (int rc = th_enqueue_encode(t, t->src, Hs, Ws, C, t->out, t->nbytes)) return rc;
    int32_t n = 0;
    SSLAM_HIP_CHECK(sslam::copy_down(s, &n, t->nbytes, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    *nbytes = n;
    SSLAM_REQUIRE(n >= 0 && (size_t)n <= t->capacity, "%s: the device left a byte count of %d (capacity %zu)", who, n, t->capacity);
    SSLAM_REQUIRE(cap >= n, "%s: the stream has %d bytes, out holds %d (sslam_thumb_capacity is always enough)", who, n, cap);
    SSLAM_HIP_CHECK(sslam::copy_down(s, out, t->out, (size_t)n));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_thumb_resize_host(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst) {
    const char* who = "sslam_thumb_resize_host";
    if (int rc = th_check_image(who, t, src, Hs, Ws, C)) return rc;
    SSLAM_REQUIRE(dst != nullptr, "%s: NULL argument", who);
    SSLAM_HIP_CHECK(hipSetDevice(t->ctx->device));
    hipStream_t s = t->ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, t->src, src, (size_t)Hs * Ws * C));
    if (int rc = th_enqueue_pixels(t, t->src, Hs, Ws, C, t->img, false)) return rc;
    SSLAM_HIP_CHECK(sslam::copy_down(s, dst, t->img, (size_t)t->w * t->h * C));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    t->last_src = nullptr;       // (the staging buffer no longer holds the last encode's source)
    return 0;
}

extern "C" int sslam_thumb_stage_read(sslam_thumb* t, int which, void* dst) {
    const char* who = "sslam_thumb_stage_read";
    SSLAM_REQUIRE(t != nullptr && dst != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(t->last_c != 0, "%s: no encode yet", who);
    SSLAM_HIP_CHECK(hipSetDevice(t->ctx->device));
    const ThumbGeom g = sslam::thumb_geom(t->w, t->h, t->last_c);
    hipStream_t s = t->ctx->stream;
    const void* from = nullptr;
    size_t bytes = 0;
    switch (which) {
    case sslam::THUMB_STAGE_RESIZED:
        SSLAM_REQUIRE(t->last_src != nullptr, "%s: the last encode's source is gone (a resize came after it)", who);
        if (int rc = th_enqueue_pixels(t, t->last_src, t->last_hs, t->last_ws, t->last_c, t->img, false)) return rc;
        from = t->img; bytes = (size_t)t->w * t->h * t->last_c;
        break;
    case sslam::THUMB_STAGE_Y: from = t->Y; bytes = (size_t)g.yw * g.yh; break;
    case sslam::THUMB_STAGE_CB:
    case sslam::THUMB_STAGE_CR:
        SSLAM_REQUIRE(g.ncomp == 3, "%s: the last encode had one component, there is no chroma plane", who);
        from = which == sslam::THUMB_STAGE_CB ? t->Cb : t->Cr; bytes = (size_t)g.cw * g.ch;
        break;
    case sslam::THUMB_STAGE_COEF: from = t->coef; bytes = (size_t)g.blocks * 64 * sizeof(int16_t); break;
    case sslam::THUMB_STAGE_BITOFF: from = t->bitoff; bytes = (size_t)g.blocks * sizeof(uint32_t); break;
    default: SSLAM_REQUIRE(false, "%s: stage %d outside 0..5", who, which);
    }
    SSLAM_HIP_CHECK(hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
