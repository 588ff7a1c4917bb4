// undistort_kernels.hip - lens undistortion: the undistort / rectify maps and the per-frame bilinear remap.
//
// Replaces `cv2.initUndistortRectifyMap(K, D, None, new_K, (W, H), cv2.CV_32FC1)` and `cv2.remap(img, mapx, mapy,
// cv2.INTER_LINEAR)` as the frame loop calls them (slam/monocular/main_revamped.py:311-316, :324).  Three kernels:
//   * ud_map_kernel       once per instance, a destination pixel per lane, fp64, OpenCV's model: [x y w] = inv(newK R) [u v 1]
//                         (the 3 x 3 inverse comes from the host), x / w, y / w, the rational radial factor, the two tangential
//                         terms, fx xd + cx / fy yd + cy rounded to float32.  OpenCV walks a row by repeated addition; this
//                         evaluates u ir[0] + (v ir[1] + ir[2]) directly (tests/undistort_ref.py carries both orders), without
//                         contraction into fused multiply-adds, so that the restatement's `direct` variant is the same arithmetic.
//   * ud_quantise_kernel  once per instance, shared by both constructors: the float32 maps in the fixed-point form of
//                         cv2.convertMaps - sx = rint(mapx * 32) (half to even; the product by 32 is exact), ix = sx >> 5
//                         saturated to int16, fx = sx & 31, alpha = fy * 32 + fx.  A non-finite coordinate, or one with
//                         |v * 32| >= 2^31, becomes a record outside every source (ix = iy = -32768, alpha = 0).
//   * ud_remap_kernel<C>  per frame, integer only: 6 B of record per pixel, C bytes from each of four neighbours (each one outside
//                         the source counts as 0: BORDER_CONSTANT, value 0), weights (32 - fx)(32 - fy) 32 ... fx fy 32 that sum to
//                         2^15, dst = (sum + 2^14) >> 15.  dst is a flat array of H W pixels; a lane owns four consecutive pixels =
//                         4, 12 or 16 bytes = whole aligned dwords from the buffer's base whatever W C is, written with one vector
//                         store; the last H W mod 4 pixels take a byte path on one extra lane.  No LDS, no atomics.
// PARITY UNPINNED: cv2 is absent here; tests/undistort_ref.py restates the functions and names what could not be confirmed.
#include "common.hpp"

#include <cmath>

struct sslam_undistort {
    sslam_ctx* ctx = nullptr;
    int W = 0, H = 0;
    sslam::OwnedSlab slab;
    float* mapx = nullptr;       // [H*W]
    float* mapy = nullptr;       // [H*W]
    int16_t* ixy = nullptr;      // [H*W][2]
    uint16_t* alpha = nullptr;   // [H*W]
};

namespace {

constexpr int UD_T = 256;
constexpr int UD_MAX = 16384;

struct UDMapArgs {
    double ir[9];                // inv(newK R), row-major
    double k[8];                 // k1 k2 p1 p2 k3 k4 k5 k6
    double fx, fy, cx, cy;
    int W;
    size_t n;
    float* mapx; float* mapy;
};

__global__ __launch_bounds__(UD_T) void ud_map_kernel(UDMapArgs a) {
    // every operation below is one IEEE fp64 operation in the written order (no fused multiply-add): the numpy restatement
    // performs the same ones, so the maps can be compared bit for bit - also where fx xd + cx cancels to almost nothing
    // (column 0 of an identity map), where no float32 tolerance would be meaningful
#pragma clang fp contract(off)
    const size_t p = (size_t)blockIdx.x * UD_T + threadIdx.x;
    if (p >= a.n) return;
    const double u = (double)(int)(p % (size_t)a.W), v = (double)(int)(p / (size_t)a.W);
    const double X = u * a.ir[0] + (v * a.ir[1] + a.ir[2]);
    const double Y = u * a.ir[3] + (v * a.ir[4] + a.ir[5]);
    const double Wh = u * a.ir[6] + (v * a.ir[7] + a.ir[8]);
    const double x = X / Wh, y = Y / Wh;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2 * x * y;
    const double k1 = a.k[0], k2 = a.k[1], p1 = a.k[2], p2 = a.k[3], k3 = a.k[4], k4 = a.k[5], k5 = a.k[6], k6 = a.k[7];
    const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
    const double xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2);
    const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2;
    a.mapx[p] = (float)(a.fx * xd + a.cx);
    a.mapy[p] = (float)(a.fy * yd + a.cy);
}

// one coordinate: false when it has no fixed-point form
__device__ __forceinline__ bool ud_fixed(float m, int& s) {
    const float t = m * 32.0f;                           // exact (a power of two), or +-inf
    if (!(fabsf(t) < 2147483648.0f)) { s = 0; return false; }      // NaN, inf, |t| >= 2^31
    s = (int)rintf(t);                                   // round half to even
    return true;
}

__device__ __forceinline__ int ud_sat16(int v) { return min(max(v, -32768), 32767); }

__global__ __launch_bounds__(UD_T)
void ud_quantise_kernel(const float* __restrict__ mapx, const float* __restrict__ mapy, size_t n, int16_t* __restrict__ ixy,
                        uint16_t* __restrict__ alpha) {
    const size_t p = (size_t)blockIdx.x * UD_T + threadIdx.x;
    if (p >= n) return;
    int sx, sy;
    const bool okx = ud_fixed(mapx[p], sx), oky = ud_fixed(mapy[p], sy);
    int ix = -32768, iy = -32768, al = 0;
    if (okx && oky) {
        ix = ud_sat16(sx >> 5); iy = ud_sat16(sy >> 5);
        al = (sy & 31) * 32 + (sx & 31);
    }
    // (one 4-byte store of the pair: ixy is 4-byte aligned per pixel)
    reinterpret_cast<uint32_t*>(ixy)[p] = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
    alpha[p] = (uint16_t)al;
}

// one destination pixel: C channel values 0..255 in out[]
template <int C>
__device__ __forceinline__ void ud_pixel(const uint8_t* __restrict__ src, int Hs, int Ws, uint32_t rec, uint32_t al, uint32_t* out) {
    const int ix = (int)(int16_t)(rec & 0xffffu), iy = (int)(int16_t)(rec >> 16);
    const int fx = (int)(al & 31u), fy = (int)((al >> 5) & 31u);
    const bool x0 = ix >= 0 && ix < Ws, x1 = ix + 1 >= 0 && ix + 1 < Ws;
    const bool y0 = iy >= 0 && iy < Hs, y1 = iy + 1 >= 0 && iy + 1 < Hs;
    // a sample outside the source has weight 0 and is read at the nearest inside address: every load is in bounds, no branch
    const int w00 = x0 && y0 ? (32 - fx) * (32 - fy) * 32 : 0, w01 = x1 && y0 ? fx * (32 - fy) * 32 : 0;
    const int w10 = x0 && y1 ? (32 - fx) * fy * 32 : 0, w11 = x1 && y1 ? fx * fy * 32 : 0;
    const int xa = min(max(ix, 0), Ws - 1), xb = min(max(ix + 1, 0), Ws - 1);
    const int ya = min(max(iy, 0), Hs - 1), yb = min(max(iy + 1, 0), Hs - 1);
    const uint8_t* ra = src + (size_t)ya * Ws * C;
    const uint8_t* rb = src + (size_t)yb * Ws * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int acc = (1 << 14) + (int)ra[xa * C + c] * w00 + (int)ra[xb * C + c] * w01 + (int)rb[xa * C + c] * w10
                        + (int)rb[xb * C + c] * w11;
        out[c] = (uint32_t)(acc >> 15);
    }
}

template <int C>
__global__ __launch_bounds__(UD_T)
void ud_remap_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, const uint32_t* __restrict__ ixy,
                     const uint16_t* __restrict__ alpha, size_t n, uint8_t* __restrict__ dst) {
    const size_t quads = n >> 2;
    const size_t t = (size_t)blockIdx.x * UD_T + threadIdx.x;
    if (t < quads) {
        const uint4 rec = reinterpret_cast<const uint4*>(ixy)[t];            // 16 B: four (ix, iy) pairs
        const uint2 al2 = reinterpret_cast<const uint2*>(alpha)[t];          // 8 B: four alphas
        const uint32_t recs[4] = {rec.x, rec.y, rec.z, rec.w};
        const uint32_t als[4] = {al2.x & 0xffffu, al2.x >> 16, al2.y & 0xffffu, al2.y >> 16};
        uint32_t b[4 * C];
#pragma unroll
        for (int q = 0; q < 4; ++q) ud_pixel<C>(src, Hs, Ws, recs[q], als[q], b + q * C);
        uint32_t w[C];
#pragma unroll
        for (int d = 0; d < C; ++d) w[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
        uint32_t* o = reinterpret_cast<uint32_t*>(dst) + t * C;
        if constexpr (C == 1) {
            o[0] = w[0];
        } else if constexpr (C == 3) {
            struct alignas(4) U3 { uint32_t a, b, c; };
            *reinterpret_cast<U3*>(o) = U3{w[0], w[1], w[2]};
        } else {
            *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else if (t == quads) {
        for (size_t p = quads << 2; p < n; ++p) {                            // the last n mod 4 pixels, byte by byte
            uint32_t b[C];
            ud_pixel<C>(src, Hs, Ws, ixy[p], alpha[p], b);
#pragma unroll
            for (int c = 0; c < C; ++c) dst[p * C + c] = (uint8_t)b[c];
        }
    }
}

unsigned ud_blocks(size_t threads) { return (unsigned)((threads + UD_T - 1) / UD_T); }

bool ud_inverse3(const double* m, double* o) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return false;
    o[0] = c0 / det; o[1] = (m[2] * m[7] - m[1] * m[8]) / det; o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = c1 / det; o[4] = (m[0] * m[8] - m[2] * m[6]) / det; o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = c2 / det; o[7] = (m[1] * m[6] - m[0] * m[7]) / det; o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}

// the instance and its four device arrays (sizes in whole units of four records: the remap kernel reads records four at a time)
int ud_alloc(const char* who, sslam_ctx* ctx, int W, int H, std::unique_ptr<sslam_undistort>& u) {
    SSLAM_HIP_CHECK(hipSetDevice(ctx->device));
    u.reset(new sslam_undistort);
    u->ctx = ctx; u->W = W; u->H = H;
    const size_t n4 = sslam::align_up((size_t)W * H, 4);
    return u->slab.alloc(who, false, [&](sslam::Slab& S) {
        u->mapx = S.take<float>(n4);
        u->mapy = S.take<float>(n4);
        u->ixy = S.take<int16_t>(2 * n4);
        u->alpha = S.take<uint16_t>(n4);
    });
}

int ud_quantise(sslam_undistort* u) {
    const size_t n = (size_t)u->W * u->H;
    hipLaunchKernelGGL(ud_quantise_kernel, dim3(ud_blocks(n)), dim3(UD_T), 0, u->ctx->stream, u->mapx, u->mapy, n, u->ixy, u->alpha);
    SSLAM_HIP_CHECK(hipGetLastError());
    SSLAM_HIP_CHECK(hipStreamSynchronize(u->ctx->stream));
    return 0;
}

int ud_check_size(const char* who, int W, int H) {
    SSLAM_REQUIRE(W >= 1 && W <= UD_MAX && H >= 1 && H <= UD_MAX, "%s: map size %dx%d outside 1..%d", who, W, H, UD_MAX);
    return 0;
}

int ud_check_remap(const char* who, sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst) {
    SSLAM_REQUIRE(u != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(src && dst, "%s: NULL argument", who);
    SSLAM_REQUIRE(C == 1 || C == 3 || C == 4, "%s: %d channels (want 1, 3 or 4)", who, C);
    SSLAM_REQUIRE(Hs >= 1 && Hs <= UD_MAX && Ws >= 1 && Ws <= UD_MAX, "%s: source size %dx%d outside 1..%d", who, Ws, Hs, UD_MAX);
    return 0;
}

int ud_enqueue_remap(sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst) {
    const size_t n = (size_t)u->W * u->H;
    const size_t threads = (n >> 2) + ((n & 3) ? 1 : 0);
    const dim3 grid(ud_blocks(threads)), block(UD_T);
    hipStream_t s = u->ctx->stream;
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(u->ixy);
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    if (C == 1) hipLaunchKernelGGL(ud_remap_kernel<1>, grid, block, 0, s, src, Hs, Ws, rec, u->alpha, n, dst);
    else if (C == 3) hipLaunchKernelGGL(ud_remap_kernel<3>, grid, block, 0, s, src, Hs, Ws, rec, u->alpha, n, dst);
    else hipLaunchKernelGGL(ud_remap_kernel<4>, grid, block, 0, s, src, Hs, Ws, rec, u->alpha, n, dst);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int sslam_undistort_create(sslam_ctx* ctx, const double* K9, const double* D, int n_dist, const double* R9,
                                      const double* newK9, int W, int H, sslam_undistort** out) {
    const char* who = "sslam_undistort_create";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(K9 && newK9, "%s: K9 / newK9 is NULL", who);
    SSLAM_REQUIRE(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8, "%s: %d distortion coefficients (want 0, 4, 5 or 8)", who, n_dist);
    SSLAM_REQUIRE(n_dist == 0 || D != nullptr, "%s: D is NULL", who);
    if (int rc = ud_check_size(who, W, H)) return rc;
    UDMapArgs a{};
    for (int i = 0; i < n_dist; ++i) a.k[i] = D[i];
    double A[9];                 // newK R
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            A[3 * r + c] = R9 ? newK9[3 * r] * R9[c] + newK9[3 * r + 1] * R9[3 + c] + newK9[3 * r + 2] * R9[6 + c] : newK9[3 * r + c];
    SSLAM_REQUIRE(ud_inverse3(A, a.ir), "%s: newK R is singular", who);
    a.fx = K9[0]; a.fy = K9[4]; a.cx = K9[2]; a.cy = K9[5];
    std::unique_ptr<sslam_undistort> u;
    if (int rc = ud_alloc(who, ctx, W, H, u)) return rc;
    a.W = W; a.n = (size_t)W * H; a.mapx = u->mapx; a.mapy = u->mapy;
    (void)hipGetLastError();
    hipLaunchKernelGGL(ud_map_kernel, dim3(ud_blocks(a.n)), dim3(UD_T), 0, ctx->stream, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) { sslam::set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return 1; }
    if (int rc = ud_quantise(u.get())) return rc;
    sslam::ctx_retain(ctx);
    *out = u.release();
    return 0;
}

extern "C" int sslam_undistort_create_from_maps(sslam_ctx* ctx, const float* mapx, const float* mapy, int W, int H,
                                                sslam_undistort** out) {
    const char* who = "sslam_undistort_create_from_maps";
    SSLAM_REQUIRE(ctx != nullptr && out != nullptr, "%s: NULL argument", who);
    SSLAM_REQUIRE(mapx && mapy, "%s: mapx / mapy is NULL", who);
    if (int rc = ud_check_size(who, W, H)) return rc;
    std::unique_ptr<sslam_undistort> u;
    if (int rc = ud_alloc(who, ctx, W, H, u)) return rc;
    const size_t n = (size_t)W * H;
    hipError_t e = hipMemcpyAsync(u->mapx, mapx, n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(u->mapy, mapy, n * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) { sslam::set_error("%s: upload failed: %s", who, hipGetErrorString(e)); return 1; }
    if (int rc = ud_quantise(u.get())) return rc;        // (synchronises: the caller's maps have been read when this returns)
    sslam::ctx_retain(ctx);
    *out = u.release();
    return 0;
}

extern "C" int sslam_undistort_destroy(sslam_undistort* u) {
    return sslam::destroy_instance(u);
}

extern "C" int sslam_undistort_maps_read(sslam_undistort* u, float* mapx, float* mapy, int16_t* ixy, uint16_t* alpha) {
    SSLAM_REQUIRE(u != nullptr, "sslam_undistort_maps_read: instance is NULL");
    SSLAM_HIP_CHECK(hipSetDevice(u->ctx->device));
    const size_t n = (size_t)u->W * u->H;
    hipStream_t s = u->ctx->stream;
    if (mapx) SSLAM_HIP_CHECK(hipMemcpyAsync(mapx, u->mapx, n * 4, hipMemcpyDeviceToHost, s));
    if (mapy) SSLAM_HIP_CHECK(hipMemcpyAsync(mapy, u->mapy, n * 4, hipMemcpyDeviceToHost, s));
    if (ixy) SSLAM_HIP_CHECK(hipMemcpyAsync(ixy, u->ixy, n * 4, hipMemcpyDeviceToHost, s));
    if (alpha) SSLAM_HIP_CHECK(hipMemcpyAsync(alpha, u->alpha, n * 2, hipMemcpyDeviceToHost, s));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}

extern "C" int sslam_undistort_remap_dev(sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst) {
    const char* who = "sslam_undistort_remap_dev";
    if (int rc = ud_check_remap(who, u, src, Hs, Ws, C, dst)) return rc;
    SSLAM_REQUIRE(((uintptr_t)dst & 15) == 0, "%s: dst is not 16-byte aligned", who);
    SSLAM_HIP_CHECK(hipSetDevice(u->ctx->device));
    return ud_enqueue_remap(u, src, Hs, Ws, C, dst);
}

extern "C" int sslam_undistort_remap_host(sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst) {
    const char* who = "sslam_undistort_remap_host";
    if (int rc = ud_check_remap(who, u, src, Hs, Ws, C, dst)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(u->ctx->device));
    const size_t sb = (size_t)Hs * Ws * C, db = (size_t)u->H * u->W * C;
    uint8_t *src_dev = nullptr, *dst_dev = nullptr;
    if (int rc = sslam::ctx_bind(u->ctx, [&](sslam::Slab& S) { src_dev = S.take<uint8_t>(sb); dst_dev = S.take<uint8_t>(db); })) return rc;
    hipStream_t s = u->ctx->stream;
    SSLAM_HIP_CHECK(sslam::copy_up(s, src_dev, src, sb));
    if (int rc = ud_enqueue_remap(u, src_dev, Hs, Ws, C, dst_dev)) return rc;
    SSLAM_HIP_CHECK(sslam::copy_down(s, dst, dst_dev, db));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
}
