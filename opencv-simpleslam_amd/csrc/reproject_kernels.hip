// reproject_kernels.hip - projection + radius search + descriptor matching of map points against
// the current frame's keypoints (2D-3D association for PnP tracking).
//
// Replaces the per-point Python loop of `reproject_and_match_2d3d`
// (slam/core/pnp_utils.py:224-304: `_project_points` :127-141, cKDTree ball query :238/:265,
// `_best_mp_distance_to_cur_desc` :107-120, greedy `used_kps` assignment :260-286) for float
// descriptors - SURVEY.md section 8(f) rank 3.
//
// The loop is sequential only through `used_kps`; everything it consumes is independent per map
// point: (1) project (float64, float32 pixels like the reference), (2) per candidate point the
// keypoints within `radius_px` (squared distance in float64, as cKDTree compares) and for each of
// them the minimum L2 distance to the point's last <= 6 observation descriptors (float32), one
// wave per point; (3) one lane then replays the greedy pass over the stored (keypoint, distance)
// lists in map order.  HBM-bound: Q x 6 x 512 B of observation descriptors read once.
//
// Binary descriptors (`uint8` rows: ORB 32 bytes, AKAZE 61) take the same steps (1) and (3); step (2) scores with the
// Hamming distance (`_desc_distance` :78-112 -> cv2.norm(a, b, NORM_HAMMING)) in `rp_pairs_hamming_kernel`: one LANE per
// keypoint in range (two passes cover the 128), the point's observation rows read once per wave through uniform
// addresses, popcount of the XOR, no cross-lane step.  The distance is stored as an exact float (<= 512), so the greedy
// pass serves both forms.  Equal minima: the lowest keypoint index wins (ascending lists + the strict `<` below).
// HBM-bound: Q x 6 x 64 B of observation rows read once plus the gathered frame rows (N x B bytes, cache resident).
//
// Host half, below the kernels: the four C entries (float / Hamming x `_host` / `_dev`) each name themselves, the shared
// parameters (RMCall) and their descriptor form (RMForm) to ONE argument check and one of two bodies, rm_dev or rm_host.
#include "common.hpp"

namespace {

constexpr int RP_MAXC = 128;      // keypoints kept per map point (within radius)
constexpr int RP_DIM = 128;
constexpr int RP_HB = 64;         // bytes of a stored binary observation row (zero beyond the descriptor's width)

struct RMArgs {
    int Q, N, img_w, img_h;
    double radius2, thr;
    const double* pts;            // [Q][3]
    const int32_t* obs_cnt;       // [Q] descriptors among the last six observations (0: point is skipped)
    const float* obs_desc;        // [Q][6][128], the valid ones first
    const double* K;              // [9]
    const double* Tcw;            // [16]
    const float* kp;              // [N][2]
    const float* des;             // [N][128]
    const int32_t* n_kp_dev;      // device count of keypoint rows, clamped to [0, N]; may be NULL (then N)
    const uint8_t* obs_u8;        // Hamming form: [Q][6][RP_HB], the valid ones first, zero beyond B bytes
    const uint8_t* des_u8;        // Hamming form: [N][B] contiguous
    int B;                        // Hamming form: bytes per descriptor row, 2..RP_HB
    float* uv;                    // [Q][2]
    int32_t* cand_n;              // [Q]  (-1: not a candidate)
    int32_t* cand_kp;             // [Q][RP_MAXC]
    float* cand_d;                // [Q][RP_MAXC]
    int32_t* kp_of_point;         // [Q] out
    int32_t* info;                // [0] matches, [1] overflow flag, [2] candidates
};

// The part both scoring kernels share, one wave per map point q: project, decide whether the point is a candidate, collect
// the keypoints in range into `list` (LDS, ascending index).  -> the number kept (<= RP_MAXC, overflow flagged), -1 when the
// point is no candidate (cand_n[q] is then already written).  The wave's LDS writes are complete on return.
__device__ __forceinline__ int rp_project_collect(const RMArgs& a, int q, int lane, int* list) {
    // `_project_points`: Xc = p R^T + t (float64), uv = (K (Xc / z))[:2] as float32, -1 where z <= 1e-8
    const double px = a.pts[3 * q], py = a.pts[3 * q + 1], pz = a.pts[3 * q + 2];
    const double* T = a.Tcw;
    const double xc = (px * T[0] + py * T[1] + pz * T[2]) + T[3];
    const double yc = (px * T[4] + py * T[5] + pz * T[6]) + T[7];
    const double zc = (px * T[8] + py * T[9] + pz * T[10]) + T[11];
    float u = -1.0f, v = -1.0f;
    if (zc > 1e-8) {
        const double xn = xc / zc, yn = yc / zc, zn = zc / zc;
        u = (float)((a.K[0] * xn + a.K[1] * yn) + a.K[2] * zn);
        v = (float)((a.K[3] * xn + a.K[4] * yn) + a.K[5] * zn);
    }
    const bool cand = zc > 0.0 && u >= 0.0f && u < (float)a.img_w && v >= 0.0f && v < (float)a.img_h && a.obs_cnt[q] > 0;
    if (lane == 0) { a.uv[2 * q] = u; a.uv[2 * q + 1] = v; a.kp_of_point[q] = -1; }
    if (!cand) { if (lane == 0) a.cand_n[q] = -1; return -1; }
    // radius search, ascending keypoint index (ballot compaction)
    const int N = a.n_kp_dev ? min(max(a.n_kp_dev[0], 0), a.N) : a.N;
    int n = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < N) {
            const double dx = (double)a.kp[2 * i] - (double)u, dy = (double)a.kp[2 * i + 1] - (double)v;
            in = dx * dx + dy * dy <= a.radius2;
        }
        const unsigned long long m = __ballot(in);
        if (in) {
            const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < RP_MAXC) list[pos] = i;
        }
        n += __popcll(m);
    }
    if (n > RP_MAXC) { if (lane == 0) atomicOr(&a.info[1], 1); n = RP_MAXC; }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    return n;
}

// one wave per map point: project, collect the keypoints in range (ascending index), score them
__global__ __launch_bounds__(256) void rp_pairs_kernel(RMArgs a) {
    __shared__ int list[4][RP_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.Q) return;
    const int n = rp_project_collect(a, q, lane, list[wave]);
    if (n < 0) return;
    // min over the stored observation descriptors of |obs - des|_2 (float32), lane = 2 dimensions
    const int cnt = a.obs_cnt[q];
    float2 o[6];
    for (int j = 0; j < 6; ++j)
        o[j] = j < cnt ? *reinterpret_cast<const float2*>(a.obs_desc + ((size_t)q * 6 + j) * RP_DIM + 2 * lane) : make_float2(0.0f, 0.0f);
    for (int c = 0; c < n; ++c) {
        const int i = list[wave][c];
        const float2 d = *reinterpret_cast<const float2*>(a.des + (size_t)i * RP_DIM + 2 * lane);
        float best = INFINITY;
        for (int j = 0; j < cnt; ++j) {
            const float ex = o[j].x - d.x, ey = o[j].y - d.y;
            float s = ex * ex + ey * ey;
            for (int sft = 32; sft > 0; sft >>= 1) s += __shfl_xor(s, sft);
            best = fminf(best, sqrtf(s));
        }
        if (lane == 0) { a.cand_kp[(size_t)q * RP_MAXC + c] = i; a.cand_d[(size_t)q * RP_MAXC + c] = best; }
    }
    if (lane == 0) a.cand_n[q] = n;
}

// 16 bytes [16 k, 16 k + 16) of a frame row of B bytes as four little-endian words, zero beyond B.  VEC is the widest load the
// row layout allows (the host chooses): 16 - B % 16 == 0 and a 16-byte aligned base; 4 - B % 4 == 0 and a 4-byte aligned
// base; 1 - bytes (AKAZE's 61), which never touches a byte beyond the row.
template <int VEC>
__device__ __forceinline__ uint4 rp_row_chunk(const uint8_t* row, int B, int k) {
    if constexpr (VEC == 16) {
        return *reinterpret_cast<const uint4*>(row + 16 * k);
    } else {
        uint32_t w[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int o = 16 * k + 4 * t;
            w[t] = 0u;
            if constexpr (VEC == 4) {
                if (o < B) w[t] = *reinterpret_cast<const uint32_t*>(row + o);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (o + b < B) w[t] |= (uint32_t)row[o + b] << (8 * b);
            }
        }
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The Hamming form of rp_pairs_kernel: the same front, then one LANE per keypoint in range.  A lane holds its keypoint's row
// chunk by chunk; the point's observation rows have wave-uniform addresses (q through readfirstlane), so they are read once
// per wave, not per lane; min_j popcount(obs_j ^ des_i) needs no cross-lane step.
template <int VEC>
__global__ __launch_bounds__(256) void rp_pairs_hamming_kernel(RMArgs a) {
    __shared__ int list[4][RP_MAXC];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.x * 4 + wave;
    if (q >= a.Q) return;
    const int n = rp_project_collect(a, q, lane, list[wave]);
    if (n < 0) return;
    const int cnt = min(__builtin_amdgcn_readfirstlane(a.obs_cnt[q]), 6);
    const int chunks = (a.B + 15) >> 4;
    const uint4* obs = reinterpret_cast<const uint4*>(a.obs_u8 + (size_t)q * 6 * RP_HB);
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int c = c0 + lane;
        if (c < n) {
            const int i = list[wave][c];
            const uint8_t* row = a.des_u8 + (size_t)i * a.B;
            int acc[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 0; k < chunks; ++k) {
                const uint4 d = rp_row_chunk<VEC>(row, a.B, k);
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    if (j < cnt) {
                        const uint4 o = obs[j * (RP_HB / 16) + k];
                        acc[j] += __popcll(((unsigned long long)(o.x ^ d.x) << 32) | (o.y ^ d.y))
                                + __popcll(((unsigned long long)(o.z ^ d.z) << 32) | (o.w ^ d.w));
                    }
                }
            }
            int best = acc[0];
#pragma unroll
            for (int j = 1; j < 6; ++j)
                if (j < cnt) best = min(best, acc[j]);
            a.cand_kp[(size_t)q * RP_MAXC + c] = i;
            a.cand_d[(size_t)q * RP_MAXC + c] = (float)best;
        }
    }
    if (lane == 0) a.cand_n[q] = n;
}

// the greedy pass, in map order (one lane; `used` bitmap in LDS)
__global__ __launch_bounds__(64) void rp_assign_kernel(RMArgs a) {
    extern __shared__ unsigned used[];
    for (int i = threadIdx.x; i < (a.N + 31) / 32; i += 64) used[i] = 0u;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int matches = 0, cands = 0;
    for (int q = 0; q < a.Q; ++q) {
        const int n = a.cand_n[q];
        if (n < 0) continue;
        ++cands;
        int best_i = -1;
        float best_d = 1e9f;
        for (int c = 0; c < n; ++c) {
            const int i = a.cand_kp[(size_t)q * RP_MAXC + c];
            if (used[i >> 5] & (1u << (i & 31))) continue;
            const float d = a.cand_d[(size_t)q * RP_MAXC + c];
            if (d < best_d) { best_d = d; best_i = i; }
        }
        if (best_i < 0 || (double)best_d > a.thr) continue;
        used[best_i >> 5] |= 1u << (best_i & 31);
        a.kp_of_point[q] = best_i;
        ++matches;
    }
    a.info[0] = matches;
    a.info[2] = cands;
}

// ---- host half: the parameters every entry shares, as passed, and the descriptor form of a call
struct RMCall {
    sslam_ctx* ctx; int n_points; const double* pts3d; const int32_t* obs_cnt; const double *K9, *Tcw16; int n_kp;
    const float* kp_xy; int img_w, img_h; double radius_px, max_dist; int32_t* kp_of_point; float* uv_out; int32_t* info_out;
};
struct RMForm {
    const void* obs;              // stored rows [n_points][6]: float[RP_DIM], or uint8[RP_HB] (zero beyond B bytes)
    const void* des;              // frame rows [n_kp]: float[RP_DIM], or uint8[B]
    bool hamming; int B;          // B: 0 for float descriptors, else the bytes of a row as given (rm_check refuses a bad width)
    const int32_t* n_kp_dev;      // Hamming `_dev` only; may be NULL
    size_t obs_row() const { return hamming ? RP_HB : RP_DIM * sizeof(float); }       // bytes
    size_t des_row() const { return hamming ? (size_t)B : RP_DIM * sizeof(float); }
    void point(RMArgs& a) const {                                   // the form's fields of RMArgs
        if (hamming) { a.obs_u8 = static_cast<const uint8_t*>(obs); a.des_u8 = static_cast<const uint8_t*>(des); }
        else { a.obs_desc = static_cast<const float*>(obs); a.des = static_cast<const float*>(des); }
        a.B = B; a.n_kp_dev = n_kp_dev;
    }
};

// The argument contract; `who` is the entry that was called.  `_dev` reports through the device info[4] alone, so it needs
// info_out, and its kernels read the caller's rows in place, so they must be aligned; `_host` can read obs_cnt, and does.
int rm_check(const char* who, const RMCall& c, const RMForm& f, bool dev) {
    SSLAM_REQUIRE(c.ctx != nullptr, "%s: ctx is NULL", who);
    SSLAM_REQUIRE(c.n_points > 0 && c.n_kp > 0, "%s: empty input (the caller returns early)", who);
    SSLAM_REQUIRE(c.pts3d && c.obs_cnt && f.obs && c.K9 && c.Tcw16 && c.kp_xy && f.des && c.kp_of_point && (c.info_out || !dev),
                  "%s: NULL argument", who);
    SSLAM_REQUIRE(!f.hamming || (f.B >= 2 && f.B <= RP_HB), "%s: desc_bytes=%d not in [2,%d]", who, f.B, RP_HB);
    SSLAM_REQUIRE(!f.hamming || !dev || reinterpret_cast<uintptr_t>(f.obs) % 16 == 0, "%s: obs_desc_u8 is not 16-byte aligned",
                  who);
    SSLAM_REQUIRE(c.radius_px >= 0.0 && c.img_w > 0 && c.img_h > 0, "%s: bad radius / image size", who);
    for (int q = 0; !dev && q < c.n_points; ++q)
        SSLAM_REQUIRE(c.obs_cnt[q] >= 0 && c.obs_cnt[q] <= 6, "%s: obs_cnt[%d]=%d not in [0,6]", who, q, c.obs_cnt[q]);
    return 0;
}

// the slab-backed pointers of RMArgs, in slab order.  staged: the map and keypoint arrays are the slab's too, and the rows
// of this form are moved there (its obs / des become the slab's pieces)
void rm_bind(sslam::Slab& sl, RMArgs& a, size_t Q, size_t N, RMForm* staged) {
    a.K = sl.take<double>(9); a.Tcw = sl.take<double>(16); a.uv = sl.take<float>(Q * 2); a.cand_n = sl.take<int32_t>(Q);
    a.cand_kp = sl.take<int32_t>(Q * RP_MAXC); a.cand_d = sl.take<float>(Q * RP_MAXC);
    a.kp_of_point = sl.take<int32_t>(Q); a.info = sl.take<int32_t>(4);
    if (!staged) return;
    a.pts = sl.take<double>(Q * 3); a.obs_cnt = sl.take<int32_t>(Q); a.kp = sl.take<float>(N * 2);
    staged->obs = sl.take<uint8_t>(Q * 6 * staged->obs_row()); staged->des = sl.take<uint8_t>(N * staged->des_row());
    staged->point(a);
}

// enqueue the two kernels on device-resident inputs (`a`: every pointer set); K9 / Tcw16 are host values
int rm_enqueue(RMArgs a, const RMCall& c) {
    hipStream_t s = c.ctx->stream;
    (void)hipGetLastError();     // (a stale error of another library on this thread is not ours)
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.K, c.K9, 9));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.Tcw, c.Tcw16, 16));
    SSLAM_HIP_CHECK(hipMemsetAsync(a.info, 0, 16, s));
    a.img_w = c.img_w; a.img_h = c.img_h; a.radius2 = c.radius_px * c.radius_px; a.thr = c.max_dist;
    const dim3 grid(sslam::cdiv(a.Q, 4)), block(256);
    if (a.B == 0) {
        hipLaunchKernelGGL(rp_pairs_kernel, grid, block, 0, s, a);
    } else {                     // the widest load every frame row allows (rp_row_chunk)
        const uintptr_t p = reinterpret_cast<uintptr_t>(a.des_u8);
        if (a.B % 16 == 0 && p % 16 == 0) hipLaunchKernelGGL(rp_pairs_hamming_kernel<16>, grid, block, 0, s, a);
        else if (a.B % 4 == 0 && p % 4 == 0) hipLaunchKernelGGL(rp_pairs_hamming_kernel<4>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(rp_pairs_hamming_kernel<1>, grid, block, 0, s, a);
    }
    hipLaunchKernelGGL(rp_assign_kernel, dim3(1), dim3(64), (((size_t)a.N + 31) / 32) * 4, s, a);
    SSLAM_HIP_CHECK(hipGetLastError());
    return 0;
}

// device-resident body: the caller's device arrays as they are; enqueue only
int rm_dev(const char* who, const RMCall& c, const RMForm& f) {
    if (int rc = rm_check(who, c, f, true)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(c.ctx->device));
    const size_t Q = (size_t)c.n_points, N = (size_t)c.n_kp;
    RMArgs a{};
    if (int rc = sslam::ctx_bind(c.ctx, [&](sslam::Slab& sl) { rm_bind(sl, a, Q, N, nullptr); })) return rc;
    a.Q = c.n_points; a.N = c.n_kp; a.pts = c.pts3d; a.obs_cnt = c.obs_cnt; a.kp = c.kp_xy; f.point(a);
    if (c.uv_out) a.uv = c.uv_out;
    a.kp_of_point = c.kp_of_point; a.info = c.info_out;
    return rm_enqueue(a, c);
}

// host-staged body: every array through the slab, one synchronisation, info_out[2] = {matches, candidates}
int rm_host(const char* who, const RMCall& c, const RMForm& f) {
    if (int rc = rm_check(who, c, f, false)) return rc;
    SSLAM_HIP_CHECK(hipSetDevice(c.ctx->device));
    const size_t Q = (size_t)c.n_points, N = (size_t)c.n_kp;
    RMArgs a{};
    RMForm d = f;                // the same form, rows in the slab
    if (int rc = sslam::ctx_bind(c.ctx, [&](sslam::Slab& sl) { rm_bind(sl, a, Q, N, &d); })) return rc;
    a.Q = c.n_points; a.N = c.n_kp;
    hipStream_t s = c.ctx->stream;
    const auto rows = [](const void* p) { return static_cast<const uint8_t*>(p); };     // rows travel as bytes
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.pts, c.pts3d, Q * 3)); SSLAM_HIP_CHECK(sslam::copy_up(s, a.obs_cnt, c.obs_cnt, Q));
    SSLAM_HIP_CHECK(sslam::copy_up(s, rows(d.obs), rows(f.obs), Q * 6 * f.obs_row()));
    SSLAM_HIP_CHECK(sslam::copy_up(s, a.kp, c.kp_xy, N * 2));
    SSLAM_HIP_CHECK(sslam::copy_up(s, rows(d.des), rows(f.des), N * f.des_row()));
    if (int rc = rm_enqueue(a, c)) return rc;
    int32_t info[4] = {0, 0, 0, 0};
    SSLAM_HIP_CHECK(sslam::copy_down(s, c.kp_of_point, a.kp_of_point, Q));
    if (c.uv_out) SSLAM_HIP_CHECK(sslam::copy_down(s, c.uv_out, a.uv, Q * 2));
    SSLAM_HIP_CHECK(sslam::copy_down(s, info, a.info, 4));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    SSLAM_REQUIRE(info[1] == 0, "%s: more than %d keypoints within %.1f px of one projection", who, RP_MAXC, c.radius_px);
    if (c.info_out) { c.info_out[0] = info[0]; c.info_out[1] = info[2]; }
    return 0;
}

}  // namespace

/* Device-resident variant: the map arrays (an incrementally maintained SoA map keeps them on the GPU)
 * and the current frame's keypoints / descriptors (straight from sslam_aliked_extract_dev) are device
 * pointers; K9 / Tcw16 are host values.  Enqueue only.  kp_of_point[n_points], uv_out[n_points*2]
 * (may be NULL) and info_out[4] = {matches, overflow flag, candidate points, 0} are device buffers. */
extern "C" int sslam_reproject_match_dev(sslam_ctx* ctx, int n_points, const double* pts3d, const int32_t* obs_cnt,
                                         const float* obs_desc, const double* K9, const double* Tcw16, int n_kp,
                                         const float* kp_xy, const float* des, int img_w, int img_h, double radius_px,
                                         double max_dist, int32_t* kp_of_point, float* uv_out, int32_t* info_out) {
    return rm_dev("sslam_reproject_match_dev", {ctx, n_points, pts3d, obs_cnt, K9, Tcw16, n_kp, kp_xy, img_w, img_h, radius_px,
                                                max_dist, kp_of_point, uv_out, info_out}, {obs_desc, des, false, 0, nullptr});
}

extern "C" int sslam_reproject_match_host(sslam_ctx* ctx, int n_points, const double* pts3d, const int32_t* obs_cnt,
                                          const float* obs_desc, const double* K9, const double* Tcw16, int n_kp,
                                          const float* kp_xy, const float* des, int img_w, int img_h, double radius_px,
                                          double max_dist, int32_t* kp_of_point, float* uv_out, int32_t* info_out) {
    return rm_host("sslam_reproject_match_host", {ctx, n_points, pts3d, obs_cnt, K9, Tcw16, n_kp, kp_xy, img_w, img_h, radius_px,
                                                  max_dist, kp_of_point, uv_out, info_out}, {obs_desc, des, false, 0, nullptr});
}

/* The Hamming form of the device-resident variant: obs_desc_u8[n_points][6][64] (zero beyond desc_bytes, 16-byte aligned)
 * and des_u8[n_kp][desc_bytes] (what sslam_orb_detect_dev writes) are device pointers.  n_kp_dev (may be NULL): the device
 * count that the detector left, clamped to n_kp rows and read by the kernels - no synchronisation.  Enqueue only. */
extern "C" int sslam_reproject_match_hamming_dev(sslam_ctx* ctx, int n_points, const double* pts3d, const int32_t* obs_cnt,
                                                 const uint8_t* obs_desc_u8, const double* K9, const double* Tcw16, int n_kp,
                                                 const float* kp_xy, const uint8_t* des_u8, int desc_bytes, int img_w,
                                                 int img_h, double radius_px, double max_hamm, int32_t* kp_of_point,
                                                 float* uv_out, int32_t* info_out, const int32_t* n_kp_dev) {
    return rm_dev("sslam_reproject_match_hamming_dev", {ctx, n_points, pts3d, obs_cnt, K9, Tcw16, n_kp, kp_xy, img_w, img_h,
                                                        radius_px, max_hamm, kp_of_point, uv_out, info_out},
                  {obs_desc_u8, des_u8, true, desc_bytes, n_kp_dev});
}

extern "C" int sslam_reproject_match_hamming_host(sslam_ctx* ctx, int n_points, const double* pts3d, const int32_t* obs_cnt,
                                                  const uint8_t* obs_desc_u8, const double* K9, const double* Tcw16, int n_kp,
                                                  const float* kp_xy, const uint8_t* des_u8, int desc_bytes, int img_w,
                                                  int img_h, double radius_px, double max_hamm, int32_t* kp_of_point,
                                                  float* uv_out, int32_t* info_out) {
    return rm_host("sslam_reproject_match_hamming_host", {ctx, n_points, pts3d, obs_cnt, K9, Tcw16, n_kp, kp_xy, img_w, img_h,
                                                          radius_px, max_hamm, kp_of_point, uv_out, info_out},
                   {obs_desc_u8, des_u8, true, desc_bytes, nullptr});
}
