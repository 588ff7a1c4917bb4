/*
 * sslam_hip.h - C-ABI of libsslam_hip.so, the MI355X (gfx950) backend for the
 * ALIKED + LightGlue + local-BA hot path of KlrShaK/opencv-SimpleSLAM.
 *
 * The reference has no FFI of its own: its hot path is Python calling
 * third-party wheels.  The drop-in boundary is the set
 * of Python names `slam/monocular/main_revamped.py` imports; this C-ABI sits
 * directly behind those names and is what a ctypes binding of that path binds
 * (INTEGRATION.md shows the binding).  Each entry point cites the reference
 * call it replaces as  file:line  relative to the reference root.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types in any signature
 *   - every function returns 0 on success, non-zero on error;
 *     sslam_last_error() returns the message of the calling thread's last error
 *   - "_host" entry points take host pointers and block until results are in
 *     the caller's buffers; "_dev" entry points take device pointers, enqueue
 *     on the context's HIP stream and return without synchronising
 *   - outputs are caller-allocated
 *   - one context per process per GPU; a context is not thread-safe
 */
#ifndef SSLAM_HIP_H
#define SSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sslam_ctx sslam_ctx;          /* device + stream + timers            */
typedef struct sslam_aliked sslam_aliked;    /* ALIKED-n16 extractor instance       */
typedef struct sslam_lightglue sslam_lightglue; /* LightGlue(features='aliked') inst.*/

/* ------------------------------------------------------------------ library */
int sslam_abi_version(void);
const char* sslam_last_error(void);
int sslam_device_count(int* n_out);

/* ------------------------------------------------------------------ context
 * Replaces the implicit `torch.cuda` device selection at
 * slam/core/features_utils.py:24 and :222.  `stream` may be NULL (the context
 * then owns a new non-blocking HIP stream) or an existing hipStream_t. */
int sslam_ctx_create(int device, void* stream, sslam_ctx** out);
int sslam_ctx_destroy(sslam_ctx* ctx);
int sslam_ctx_sync(sslam_ctx* ctx);
void* sslam_ctx_stream(sslam_ctx* ctx);
/* HIP-event timer on the context's stream (bench.py roofline measurement). */
int sslam_timer_start(sslam_ctx* ctx);
int sslam_timer_stop(sslam_ctx* ctx, float* elapsed_ms_out);
/* Device memory helpers so a ctypes host needs no other GPU runtime. */
int sslam_malloc(sslam_ctx* ctx, size_t bytes, void** dptr_out);
int sslam_free(sslam_ctx* ctx, void* dptr);
int sslam_memcpy_h2d(sslam_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int sslam_memcpy_d2h(sslam_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Enqueue-only helpers on the context's stream, and events to order one context's stream behind
 * another's: what the frame pipeline (several extractor / matcher contexts on one GPU) needs, so
 * the single-GPU product path runs without any other GPU runtime. */
int sslam_memcpy_d2d_async(sslam_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes);
int sslam_memset_async(sslam_ctx* ctx, void* dst_dev, int value, size_t bytes);
/* Page-locked host memory and enqueue-only host <-> device copies on the context's stream (the host buffer
 * must stay valid, and for a real overlap be page-locked, until the stream has passed the copy): the
 * drop-in `feature_extractor` / `feature_matcher` (slam/core/features_utils.py:85-171) stage the image and
 * read the result records back through these instead of the torch `.cuda()` / `.cpu()` calls at :222, :97. */
int sslam_host_alloc(sslam_ctx* ctx, size_t bytes, void** hptr_out);
int sslam_host_free(sslam_ctx* ctx, void* hptr);
int sslam_memcpy_h2d_async(sslam_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int sslam_memcpy_d2h_async(sslam_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int sslam_event_create(sslam_ctx* ctx, void** event_out);
int sslam_event_destroy(void* event);
int sslam_event_record(sslam_ctx* ctx, void* event);      /* on ctx's stream */
int sslam_ctx_wait_event(sslam_ctx* ctx, void* event);    /* ctx's stream waits, host does not */
/* Timing events (the ordering events above are created without timestamps) and the time between two recorded
 * ones (waits for the second): per-round durations of a running pipeline without synchronising inside it. */
int sslam_timing_event_create(sslam_ctx* ctx, void** event_out);
int sslam_event_elapsed_ms(void* start_event, void* stop_event, float* ms_out);

/* ------------------------------------------------------------------ local BA
 * Batched reprojection residual + Jacobian.  Replaces the per-observation
 * `cost_functions.ReprojErrorCost(CameraModelId.PINHOLE, uv)` blocks that
 * slam/core/ba_utils.py:56-68 adds and Ceres evaluates inside
 * `pyceres.solve` (ba_utils.py:293).  All float64.
 *   pose_idx[n_obs], point_idx[n_obs] : int32 indices into q/t and X
 *   uv[n_obs*2]; q[n_poses*4] quaternion (x,y,z,w) cam-from-world;
 *   t[n_poses*3]; X[n_points*3]; intr[4] = fx,fy,cx,cy
 *   r[n_obs*2]; Jq[n_obs*8] (2x4 row-major, ambient xyzw); Jt[n_obs*6];
 *   JX[n_obs*6].  Any of Jq/Jt/JX may be NULL (residual only). */
int sslam_ba_residual_jacobian_host(sslam_ctx* ctx, int n_obs,
                                    const int32_t* pose_idx, const int32_t* point_idx,
                                    const double* uv, int n_poses, const double* q,
                                    const double* t, int n_points, const double* X,
                                    const double* intr, double* r, double* Jq,
                                    double* Jt, double* JX);
int sslam_ba_residual_jacobian_dev(sslam_ctx* ctx, int n_obs,
                                   const int32_t* pose_idx, const int32_t* point_idx,
                                   const double* uv, int n_poses, const double* q,
                                   const double* t, int n_points, const double* X,
                                   const double* intr, double* r, double* Jq,
                                   double* Jt, double* JX);

/* Whole local-BA solve on the device: replaces `pyceres.solve(opts, problem, summary)` at
 * slam/core/ba_utils.py:288-293 for the problem `_core_ba` assembles (:220-286): Huber(delta)
 * on every reprojection block (:236), EigenQuaternionManifold on every quaternion (:245-249),
 * constant blocks for the gauge keyframes (:250-257) and - with points_const - for the
 * landmarks (pose_only_ba, :89-140); Ceres' default trust-region constants, at most
 * `max_iters` iterations (:289-292).  Levenberg-Marquardt with the Schur complement onto the
 * optimised poses; linearisation, reduction, Cholesky, step evaluation and the accept / reject /
 * terminate logic all run on the GPU as one enqueue (no host round trip per iteration).
 *   q[n_poses*4], t[n_poses*3], X[n_points*3] : in = initial values, out = optimised
 *   pose_const[n_poses] : 1 = held fixed.  At most 256 non-constant poses (more is refused with an error;
 *                         up to 12 - local BA - the reduced pose system is factored in LDS, beyond that in
 *                         device memory by one workgroup; the dense Schur blocks must fit 32 GiB)
 *   summary[8] : iterations, successful steps, initial cost, final cost (0.5 sum rho),
 *                termination (0 max iterations, 1 gradient, 2 parameter, 3 function tolerance,
 *                4 trust region collapsed), final radius, #optimised poses, 0 */
int sslam_ba_solve_host(sslam_ctx* ctx, int n_obs, const int32_t* pose_idx,
                        const int32_t* point_idx, const double* uv, int n_poses, double* q,
                        double* t, const unsigned char* pose_const, int n_points, double* X,
                        const double* intr, int max_iters, double huber_delta, int points_const,
                        double* summary);

/* ------------------------------------------------------- F-matrix RANSAC
 * Replaces `cv2.findFundamentalMat(pts1, pts2, cv2.FM_RANSAC, thresh, 0.99)` inside
 * `filter_matches_ransac` (slam/core/features_utils.py:185-200): OpenCV 4.x's classic path
 * (7-point RANSAC for >= 15 matches, LMedS for 8..14, cv::RNG sample stream), scored on the GPU.
 *   pts1, pts2 : float32 [n][2] matched pixel coordinates (host), n >= 8
 *   thresh <= 0 -> 3, confidence outside (0,1) -> 0.99, max_iters <= 0 -> 1000 (cv2 defaults)
 *   mask_out[n] : 1 = inlier;  F_out[9] (may be NULL): row-major, F[8] = 1 or 0
 *   info_out[4] (may be NULL): inliers (-1: no model, cv2 would return mask None),
 *                              iterations the sequential loop runs, 1 if LMedS, winning sample */
int sslam_fmat_ransac_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2,
                           double thresh, double confidence, int max_iters,
                           unsigned char* mask_out, double* F_out, int* info_out);

/* Device-resident form of the same filter, for a tracking step that keeps the matcher's output on the
 * GPU: consumes what `sslam_lightglue_match_dev` wrote and leaves what `filter_matches_ransac` would
 * return (features_utils.py:185-200) on the device; enqueued on ctx's stream, no host round trip.
 *   n_max: bound on the match count;  n_dev: device int32 count (e.g. the matcher's info[0]), clamped to
 *   [0, n_max]; NULL = exactly n_max matches
 *   xy1_dev, xy2_dev: keypoints [*][2] float32;  ij_dev: int32 [n][2] (query, train) index pairs
 *   mask_out_dev[n_max] (may be NULL): 1 = kept;  ij_out_dev[n_max][2] (may be NULL): the kept pairs, in order
 *   F_out_dev[9] double (may be NULL);  info_out_dev[4] int32: pairs kept, iterations, 1 if LMedS,
 *   winning sample (-1: no model -> nothing kept, as the reference's `mask is None`; -2: fewer than 8
 *   matches, all kept unfiltered as the reference does)
 * The context's scratch buffer is (re)allocated when n_max grows: call once with the largest n_max
 * before capturing or pipelining. */
int sslam_fmat_ransac_dev(sslam_ctx* ctx, int n_max, const int32_t* n_dev, const float* xy1_dev,
                          const float* xy2_dev, const int32_t* ij_dev, double thresh, double confidence,
                          int max_iters, unsigned char* mask_out_dev, int32_t* ij_out_dev,
                          double* F_out_dev, int32_t* info_out_dev);

/* --------------------------------------------------------------- PnP-RANSAC
 * Replaces `cv2.solvePnPRansac(pts3d, pts2d, K, None, flags=cv2.SOLVEPNP_ITERATIVE, ...)` inside
 * `solve_pnp_ransac` (slam/core/pnp_utils.py:307-341) and `refine_pose_pnp` (:200-221): OpenCV 4.x's
 * classic path (EPnP on 5-point samples of the cv::RNG stream, float32 reprojection error, final
 * Levenberg-Marquardt on the winner's inliers), scored on the GPU.  Parity with cv2 itself is unpinned
 * (tests/pnp_oracle.py names what could not be confirmed).
 *   pts3d_f32[n*3], pts2d_f32[n*2] (host), n >= 5 (4: OpenCV's P3P branch, not covered; fewer: the caller
 *   returns early);  K9 row-major 3x3 (fx, fy, cx, cy are read; skew ignored as projectPoints does)
 *   Tcw_init16 (may be NULL): only whether it is given matters - with a guess OpenCV starts the final
 *   refinement from the LAST sample's EPnP pose (its RANSAC callback writes every sample into the guess
 *   buffers), without one from the winner's; n == 5: one EPnP on all points, all inliers, no refinement
 *   reproj_px: inlier iff float ||ip - proj||^2 <= (float)(px^2), px rounded to float first
 *   confidence in (0,1); max_iters 0..100000 (0 acts as 1)
 *   mask_out[n]: the RANSAC winner's inliers (1);  Tcw_out16: row-major 4x4 camera-from-world
 *   info_out[4] (may be NULL): inliers (-1: no model, cv2 returns False), samples the sequential loop
 *   ran, winning sample, LM iterations */
int sslam_pnp_ransac_host(sslam_ctx* ctx, int n, const float* pts3d_f32, const float* pts2d_f32,
                          const double* K9, const double* Tcw_init16, double reproj_px, double confidence,
                          int max_iters, unsigned char* mask_out, double* Tcw_out16, int* info_out);

/* Device-resident form (enqueue only, no host round trip): consumes what `sslam_reproject_match_dev`
 * wrote - kp_of_point_dev[n_points], the map's pts3d_dev[n_points*3] doubles and the keypoints
 * kp_xy_dev[*][2] - and compacts the correspondences in map order (the order of the overlay's
 * Matches2D3D), cast to float32 as the reference does.  K9 / Tcw_init16 stay host values (as above).
 *   mask_out_dev[n_points] (may be NULL): inlier flags of the compacted correspondences
 *   Tcw_out_dev[16] double: the pose (identity when there is none);  n_out_dev (may be NULL): the
 *   correspondence count;  info_out_dev[4] int32 as info_out above; fewer than 5 correspondences
 *   (4 included) give info[0] = -1
 * The context's scratch buffer is (re)allocated when n_points or max_iters grows: call once with the
 * largest before capturing or pipelining. */
int sslam_pnp_ransac_dev(sslam_ctx* ctx, int n_points, const int32_t* kp_of_point_dev,
                         const double* pts3d_dev, const float* kp_xy_dev, const double* K9,
                         const double* Tcw_init16, double reproj_px, double confidence, int max_iters,
                         unsigned char* mask_out_dev, double* Tcw_out_dev, int32_t* n_out_dev,
                         int32_t* info_out_dev);

/* ------------------------------------------------- two-view triangulation
 * The numeric body of `triangulate_between_kfs_2view` (slam/core/triangulation_utils.py:143-271):
 * `cv2.triangulatePoints` with P = K T[:3,:] (OpenCV 4.x's DLT, null vector by a one-sided Jacobi SVD of
 * the 4 x 4 matrix itself), X = X4[:3] / w where w is finite and |w| > 1e-12, then the reference's gates
 * in its order.  Every match gets one reason:
 *   0 kept, 1 invalid_w, 2 low_parallax (only with use_parallax_gate: world-frame parallax < parallax_min_deg),
 *   3 bad_depth (not min_depth <= z <= max_depth in both views), 4 behind_cam (z <= 1e-6 in a view),
 *   5 high_reproj (max(e1, e2) > reproj_px_max).  fp64 throughout.
 *   pts1, pts2 : float32 [n][2] matched pixels (host), used as doubles;  n == 0 is legal
 *   K9 row-major 3x3;  T1_16, T2_16 : row-major 4x4 camera-from-world of the two views
 *   X_out[n*3] : the kept points, compacted in match order;  idx_out[n] : their match indices
 *   info_out[8] : kept, then the counts of reasons 0 .. 5, then n
 *   reason_out[n] (may be NULL) : the reason per match;  diag_out[n*5] (may be NULL) : parallax in degrees
 *   (NaN with the gate off), z1, z2, e1, e2 per match (+inf error behind a camera, NaN where w is invalid) */
int sslam_triangulate_2view_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2,
                                 const double* K9, const double* T1_16, const double* T2_16,
                                 double min_depth, double max_depth, int use_parallax_gate,
                                 double parallax_min_deg, double reproj_px_max, double* X_out,
                                 int32_t* idx_out, int32_t* info_out, int32_t* reason_out,
                                 double* diag_out);

/* Device-resident form (enqueue only, no host round trip): consumes what `sslam_fmat_ransac_dev` left -
 * the kept pairs ij_dev[*][2] and their count n_dev (its info[0]; clamped to [0, n_max], so a negative
 * count is an empty input; NULL = exactly n_max) - on the keypoint arrays xy1_dev / xy2_dev [*][2] of the
 * two frames.  T1_dev, T2_dev: DEVICE double[16] (a pose `sslam_pnp_ransac_dev` wrote can be passed as it
 * is); K9 and the thresholds are host values.
 *   X_out_dev[n_max*3], ij_out_dev[n_max][2] (may be NULL): the kept points and their (query, train) pairs,
 *   in order;  info_out_dev[8] int32 as info_out above;  reason_out_dev[n_max] / diag_out_dev[n_max*5]
 *   (may be NULL) as above
 * The context's scratch buffer is (re)allocated when n_max grows: call once with the largest n_max
 * before capturing or pipelining. */
int sslam_triangulate_2view_dev(sslam_ctx* ctx, int n_max, const int32_t* n_dev, const float* xy1_dev,
                                const float* xy2_dev, const int32_t* ij_dev, const double* K9,
                                const double* T1_dev, const double* T2_dev, double min_depth,
                                double max_depth, int use_parallax_gate, double parallax_min_deg,
                                double reproj_px_max, double* X_out_dev, int32_t* ij_out_dev,
                                int32_t* info_out_dev, int32_t* reason_out_dev, double* diag_out_dev);

/* ------------------------------------------------ multi-view triangulation
 * The numeric body of `multi_view_triangulation` / `MultiViewTriangulator` (slam/core/multi_view_utils.py, the
 * module the reference's tests call and its tree no longer holds; PARITY UNPINNED), for n_tracks tracks in one
 * call.  Observations are CSR: track i owns observations track_off[i] .. track_off[i+1]-1, observation o is the
 * pixel obs_uv[o] (float32, used as doubles) in view obs_view[o] of the n_views views Tcw[n_views][16]
 * (row-major camera-from-world).  Per view P = K Tcw[:3]; per track the rows u P[2] - P[0], v P[2] - P[1] of its
 * observations stack to A [2V, 4], Xh is the unit right singular vector of A's smallest singular value (A is
 * reduced to its 4 x 4 triangular factor by Givens rotations, then the one-sided Jacobi SVD of the two-view
 * entry; no cap on V), X = Xh[:3] / w, z_k = (Tcw_k X)[2].  Every track gets one reason, decided in this order:
 *   1 too_few_views (V < 2), 2 invalid_w (w not finite or |w| <= 1e-12), 3 bad_depth (some z_k outside
 *   [min_depth, max_depth]), 4 behind_cam (some z_k <= 1e-6), 5 high_reproj (the MEAN over the track's views of
 *   the pixel error ||K (Tcw_k X) / z_k - (u_k, v_k)|| exceeds max_rep_err), else 0 kept.  fp64 throughout.
 *   X_out[n_tracks*3] : the kept points, compacted in track order;  idx_out[n_tracks] : their track indices
 *   info_out[8] : kept, then the counts of reasons 0 .. 5, then n_tracks;  n_tracks == 0 is legal
 *   reason_out[n_tracks] (may be NULL) : the reason per track;  diag_out[n_tracks*3] (may be NULL) : mean pixel
 *   error, smallest and largest z_k per track (NaN where there is no point; +inf error behind a camera)
 * An offset array that decreases or a view index outside [0, n_views) is an error. */
int sslam_triangulate_tracks_host(sslam_ctx* ctx, int n_tracks, int n_views, const int32_t* track_off,
                                  const int32_t* obs_view, const float* obs_uv, const double* K9,
                                  const double* Tcw, double min_depth, double max_depth, double max_rep_err,
                                  double* X_out, int32_t* idx_out, int32_t* info_out, int32_t* reason_out,
                                  double* diag_out);

/* ------------------------------------------------ landmark pairs within a radius
 * Every (i, j), i < j, of pos[n][3] (double) with dx^2 + dy^2 + dz^2 <= radius^2 in fp64 - what
 * `cKDTree(pos).query_pairs(radius)` returns, the input of `Map.fuse_closeby_duplicate_landmarks`
 * (slam/core/landmark_utils.py:138-161).  A non-finite coordinate pairs with nothing.
 *   pairs_out[cap][2] (host) : the first min(*count_out, cap) pairs found, in NO particular order (sort them)
 *   count_out : the exact number of pairs, also when it exceeds cap - call again with a buffer of that size
 * `_host` takes the positions from host memory, `_dev` from device memory (the Map's device mirror). */
int sslam_close_pairs_host(sslam_ctx* ctx, int n, const double* pos, double radius, int64_t cap,
                           int32_t* pairs_out, int64_t* count_out);
int sslam_close_pairs_dev(sslam_ctx* ctx, int n, const double* pos_dev, double radius, int64_t cap,
                          int32_t* pairs_out, int64_t* count_out);

/* ------------------------------------------------ two-view relative pose
 * Replaces `cv2.recoverPose(E, pts_ref, pts_cur, K)` in `recover_pose_from_fundamental`
 * (slam/core/two_view_bootstrap.py:207-208) and in the tracking-lost fallback (slam/monocular/main_revamped.py:514):
 * OpenCV 4.x's five-point.cpp restated.  Pixels are widened to double and normalised (x - cx) / fx, (y - cy) / fy;
 * `decomposeEssentialMat` (3 x 3 one-sided Jacobi SVD, U = -U / Vt = -Vt where a determinant is negative,
 * R1 = U W Vt, R2 = U W^T Vt, t = U[:,2]); the candidates [R1|t] [R2|t] [R1|-t] [R2|-t] against [I|0]; every
 * match triangulated by the DLT of `cv2.triangulatePoints` into Q and judged per candidate:
 * Q2 Q3 > 0, then Q /= Q3 and Q2 < distance_thresh, then Q = P Q and 0 < Q2 < distance_thresh (a zero Q3 gives
 * inf / NaN and every comparison with those is false).  The winner by OpenCV's own >= chain, candidate 1 first.
 * fp64 throughout.  Parity with cv2 itself is unpinned (tests/relative_pose_ref.py names what could not be confirmed).
 *   pts1, pts2 : float32 [n][2] matched pixels (host);  n == 0 is legal: all counts zero, candidate 1 wins
 *   E9, K9 row-major 3x3 (fx, fy, cx, cy are read);  distance_thresh : cv2's default is 50
 *   mask_in[n] (may be NULL) : each candidate's mask is mask_in & (good ? 255 : 0) bytewise - a 0/1 mask stays 0/1;
 *   without it the mask is 255 / 0
 *   R_out9, t_out3, mask_out[n] : the winner's R, its +-t and its mask
 *   info_out[8] : good (the winner's non-zero count), n, winner 0..3, good1, good2, good3, good4, 0 */
int sslam_recover_pose_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, const double* E9,
                            const double* K9, double distance_thresh, const unsigned char* mask_in,
                            double* R_out9, double* t_out3, unsigned char* mask_out, int32_t* info_out);

/* `triangulation_metrics` (slam/core/two_view_bootstrap.py:127-156) and `_triangulate_points_cv` (:314-326):
 * `cv2.undistortPoints` without distortion ((x - cx) * (1 / fx) in double, rounded to float32 as OpenCV 4.x does for
 * float32 input), the DLT against [I|0] and [R|t], X = Xh[:3] / (Xh[3] + 1e-12), z1 = X[2], z2 = (R X + t)[2],
 * cos = v1.v2 / (|v1||v2| + 1e-12) with v1 = X, v2 = X + R^T t, clipped to [-1, 1].
 *   sel[n] (may be NULL: every match) : the matches with a non-zero byte take part, compacted in match order
 *   (how the reference passes pts[inl]); N = their number, at most 16384 (more is an error)
 *   K9, R9 row-major 3x3, t3
 *   metrics_out[2] : count(z1 > 0 and z2 > 0) / N, degrees(median(arccos(cos))) - for an even N the mean of the
 *   two middle values, exact;  info_out[4] : N, the count in front, 0, 0.  N < 2 gives metrics 0, 0 and
 *   info[0] = 0 (the reference's early return).  Behaviour on NaN inputs is unspecified.
 *   X_out[N*3], z_out[N*2] (may be NULL) : the points and their two depths, in selected order */
int sslam_two_view_metrics_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2,
                                const unsigned char* sel, const double* K9, const double* R9, const double* t3,
                                double* metrics_out, int32_t* info_out, double* X_out, double* z_out);

/* ------------------------------------------------------- homography RANSAC
 * Replaces `cv2.findHomography(pts1, pts2, cv2.RANSAC, thresh)` as the two-view gate calls it
 * (slam/core/two_view_bootstrap.py:230, :294; the tracking fallbacks slam/monocular/main.py:409, main4.py:458): OpenCV 4.x's
 * classic path - 4-point normalised DLT, cv::RNG sample stream, collinearity and orientation tests on every draw, float error
 * of the forward transfer, the loop's mask kept, then one DLT on the inliers and at most 10 Levenberg-Marquardt iterations
 * on H's first eight entries.  fp64 (the error in float, as in OpenCV).  Parity with cv2 itself is unpinned
 * (tests/homography_ref.py names what could not be confirmed).
 *   pts1, pts2 : float32 [n][2] source / destination pixels (host), 4 <= n <= 16384 (anything else is an error);
 *   n == 4: one DLT on the four matches, mask all ones, no refinement
 *   thresh <= 0 -> 3, confidence outside (0,1) -> 0.995, max_iters clamped to [1, 2000]
 *   mask_out[n] : 1 = inlier of the loop's winning sample;  H_out[9] (may be NULL): row-major, H[8] = 1, zeros without a model
 *   info_out[4] (may be NULL): inliers (-1: no model, cv2 would return (None, None)), iterations the sequential loop
 *                              runs (0 for n == 4), 0, winning sample
 * Two calls on the same input give the same bits. */
int sslam_homography_ransac_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, double thresh,
                                 double confidence, int max_iters, unsigned char* mask_out, double* H_out,
                                 int32_t* info_out);

/* ---------------------------------------------------- essential-matrix RANSAC
 * Replaces `cv2.findEssentialMat(pts0, pts1, K, cv2.RANSAC, 0.999, thresh)` as the tracking-lost fallback calls it
 * (slam/monocular/main_revamped.py:512, main.py:402, main4.py:457): OpenCV 4.x's classic path - pixels widened to double
 * and normalised (x - cx) / fx, (y - cy) / fy, the threshold divided by (fx + fy) / 2, the cv::RNG sample stream (five
 * distinct indices, no subset test), Nister's five-point solver (up to ten models per sample, each of unit Frobenius norm,
 * scored in order), the Sampson distance in double stored as float, the budget re-estimated after every improvement, no
 * refit and no polish.  fp64.  Parity with cv2 itself is unpinned (tests/essential_ref.py names what could not be
 * confirmed).  The mask and E feed `sslam_recover_pose_host` as they are.
 *   pts1, pts2 : float32 [n][2] matched pixels (host), 5 <= n <= 16384 (anything else is an error);
 *   n == 5: one solve on the five matches, mask all ones, every model returned
 *   K9 : row-major 3x3 (fx, fy, cx, cy are read)
 *   prob outside (0,1) -> 0.999, thresh <= 0 -> 1, max_iters <= 0 -> 1000, above 2000 -> 2000 (the scratch slab holds
 *   max_iters x 10 models)
 *   mask_out[n] : 1 = inlier of the winning model;  E_out[90] (may be NULL): the winner row-major in E_out[0..9), the
 *   rest zero; for n == 5 every model, stacked; zeros without a model
 *   info_out[4] (may be NULL): inliers (-1: no model, cv2 would return (None, None)), iterations the sequential loop
 *                              runs (0 for n == 5), the winning model's index within its sample (for n == 5 the number
 *                              of models), winning sample
 * Two calls on the same input give the same bits. */
int sslam_essential_ransac_host(sslam_ctx* ctx, int n, const float* pts1, const float* pts2, const double* K9,
                                double prob, double thresh, int max_iters, unsigned char* mask_out,
                                double* E_out, int32_t* info_out);

/* ------------------------------------------------------- lens undistortion
 * Replaces `cv2.initUndistortRectifyMap(K, D, None, new_K, (W0, H0), cv2.CV_32FC1)` and the per-frame
 * `cv2.remap(img, mapx, mapy, cv2.INTER_LINEAR)` (slam/monocular/main_revamped.py:311-316, :324): the maps are computed
 * once on the device in fp64 (OpenCV's model: inv(newK R), the rational radial factor, two tangential terms; rounded to
 * float32), turned into cv2.convertMaps' fixed-point form (int16 pixel + 5-bit fractions, round half to even; a non-finite
 * coordinate or one beyond the int32 range of v * 32 becomes a record outside every source) and kept there; a remap is one
 * integer-only gather kernel: weights (32 - fx)(32 - fy) 32 ... that sum to 2^15, dst = (sum + 2^14) >> 15, every sample
 * outside the source counts as 0 (BORDER_CONSTANT, value 0).  Parity with cv2 itself is unpinned (tests/undistort_ref.py
 * names what could not be confirmed). */
typedef struct sslam_undistort sslam_undistort;
/* cv2.initUndistortRectifyMap(K, D, R, newK, (W, H), CV_32FC1), then cv2.convertMaps' fixed-point form, kept on the device.
 * D: n_dist in {0, 4, 5, 8} doubles (k1 k2 p1 p2 [k3 [k4 k5 k6]]); R9 NULL = identity; 1 <= W, H <= 16384. */
int sslam_undistort_create(sslam_ctx* ctx, const double* K9, const double* D, int n_dist, const double* R9,
                           const double* newK9, int W, int H, sslam_undistort** out);
/* the same instance from the caller's float32 maps [H][W] (host): cv2.remap(img, mapx, mapy, INTER_LINEAR) with any maps */
int sslam_undistort_create_from_maps(sslam_ctx* ctx, const float* mapx, const float* mapy, int W, int H,
                                     sslam_undistort** out);
int sslam_undistort_destroy(sslam_undistort* u);
/* any pointer may be NULL: float32 maps [H*W]; ixy int16 [H*W*2]; alpha uint16 [H*W] (= fy * 32 + fx) */
int sslam_undistort_maps_read(sslam_undistort* u, float* mapx, float* mapy, int16_t* ixy, uint16_t* alpha);
/* src uint8 [Hs][Ws][C], C in {1, 3, 4}, 1 <= Hs, Ws <= 16384; dst uint8 [H][W][C]; BORDER_CONSTANT, value 0.
 * _dev: device pointers, dst 16-byte aligned (as sslam_malloc returns it); enqueue only. */
int sslam_undistort_remap_host(sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst);
int sslam_undistort_remap_dev(sslam_undistort* u, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst);

/* ------------------------------------------------ pyramidal Lucas-Kanade
 * Replaces `cv2.cvtColor(img, cv2.COLOR_BGR2GRAY)` and `cv2.calcOpticalFlowPyrLK(prev, next, pts, None, winSize, maxLevel,
 * criteria, flags, minEigThreshold)` for 8-bit images, and the forward-backward gate of the KLT front end
 * (slam/monocular/main4.py:396-433).  An instance keeps the pyramids of two frames on the device: grey, the pyrDown levels
 * (padded by winSize, BORDER_REFLECT_101) and the unscaled int16 Scharr pair of every level (padded with zeros); a push builds
 * one frame's pyramid ONCE and the frame that was "current" becomes "previous".  The tracker is OpenCV's fixed-point scheme
 * (2^14 bilinear weights, int16 patches); its window sums are exact integers converted to float32 once.  Parity with cv2
 * itself is unpinned (tests/klt_ref.py names what could not be confirmed).
 * Limits: 1 <= w, h <= 16384; window sides odd, 3..31 (the patch of one point is held in LDS; the integer sums stay below 2^53
 * and are exact); maxLevel 0..10; 1 <= n <= max_points <= 2^20. */
typedef struct sslam_klt sslam_klt;
int sslam_klt_create(sslam_ctx* ctx, int max_w, int max_h, int max_points, int win_w, int win_h, int max_level,
                     sslam_klt** out);
int sslam_klt_destroy(sslam_klt* k);
/* img uint8 [h][w][c], c in {1, 3 (BGR), 4 (BGRA)}, w <= max_w, h <= max_h.  _host returns when the image has been read;
 * _dev: device pointer, enqueue only (the image must stay untouched until the stream has passed the call). */
int sslam_klt_push_host(sslam_klt* k, const uint8_t* img, int h, int w, int c);
int sslam_klt_push_dev(sslam_klt* k, const uint8_t* img, int h, int w, int c);
/* the grey conversion alone: gray uint8 [h][w] (host) */
int sslam_klt_gray_host(sslam_ctx* ctx, const uint8_t* img, int h, int w, int c, uint8_t* gray);
/* previous -> current (reverse = 0) or current -> previous (reverse = 1).  prev_pts [n][2] float32; init_pts [n][2] is read
 * under OPTFLOW_USE_INITIAL_FLOW (flags & 4) and may be NULL otherwise; flags & 8 = OPTFLOW_LK_GET_MIN_EIGENVALS;
 * (criteria_type, max_count, epsilon) as cv2's TermCriteria (COUNT = 1, EPS = 2; clamped as OpenCV clamps them).
 * Out: next_pts [n][2] float32, status [n] uint8, err [n] float32 (0 where OpenCV leaves it unwritten).
 * _dev: device pointers, enqueue only. */
int sslam_klt_track_host(sslam_klt* k, int reverse, int n, const float* prev_pts, const float* init_pts, int flags,
                         int criteria_type, int max_count, double epsilon, double min_eig_threshold, float* next_pts,
                         uint8_t* status, float* err);
int sslam_klt_track_dev(sslam_klt* k, int reverse, int n, const float* prev_pts, const float* init_pts, int flags,
                        int criteria_type, int max_count, double epsilon, double min_eig_threshold, float* next_pts,
                        uint8_t* status, float* err);
/* main4.py:402-433 in one call: forward, backward from the forward result (all points), the masks status == 1,
 * err < err_thresh, st_back == 1 && |back - prev| < fb_thresh (float32, thresholds rounded to float32), and the kept pairs
 * compacted in point order.  Out: pts0 / pts1 [n][2] float32 of which the first counts[4] pairs are written;
 * counts[5] = raw, st1, err_ok, fb_ok, kept; optional (may be NULL) next_pts [n][2] and mask [n] uint8 (bit 0 status,
 * bit 1 err, bit 2 forward-backward, bit 3 kept).  _dev: device pointers, everything stays on the device, enqueue only. */
int sslam_klt_track_fb_host(sslam_klt* k, int n, const float* prev_pts, int criteria_type, int max_count, double epsilon,
                            double min_eig_threshold, double err_thresh, double fb_thresh, float* next_pts, float* pts0,
                            float* pts1, int* counts, uint8_t* mask);
int sslam_klt_track_fb_dev(sslam_klt* k, int n, const float* prev_pts, int criteria_type, int max_count, double epsilon,
                           double min_eig_threshold, double err_thresh, double fb_thresh, float* next_pts, float* pts0,
                           float* pts1, int* counts, uint8_t* mask);
/* test hooks.  info: the effective maxLevel and the size of the current (previous = 0) or previous (1) frame.
 * levels_read: one level of it back to the host, any pointer may be NULL: img uint8 [h_l][w_l] (level 0 is the grey image),
 * dx / dy int16 [h_l][w_l]. */
int sslam_klt_info(sslam_klt* k, int previous, int* top_level, int* w, int* h);
int sslam_klt_levels_read(sslam_klt* k, int previous, int level, uint8_t* img, int16_t* dx, int16_t* dy);

/* ------------------------------------------- 2D-3D association for tracking
 * Replaces the per-point loop of `reproject_and_match_2d3d` (slam/core/pnp_utils.py:224-304) for
 * float descriptors: projection (`_project_points` :127-141), radius search (cKDTree :238, :265),
 * min L2 over the point's last six observation descriptors (:107-120) and the greedy `used_kps`
 * pass in map order (:260-286).
 *   pts3d[n_points*3] float64 world points in `world_map.points` order
 *   obs_cnt[n_points]: 0..6 = descriptors among the point's last six observations; 0 also for a point
 *     whose LAST observation has none (the reference skips it, :270-272)
 *   obs_desc[n_points*6*128]: those descriptors, valid ones first
 *   K9 row-major 3x3, Tcw16 row-major 4x4 (camera-from-world), kp_xy[n_kp*2], des[n_kp*128] float32
 *   kp_of_point[n_points]: out, matched keypoint index or -1;  uv_out[n_points*2] (may be NULL)
 *   info_out[2] (may be NULL): matches, candidate points */
int sslam_reproject_match_host(sslam_ctx* ctx, int n_points, const double* pts3d,
                               const int32_t* obs_cnt, const float* obs_desc, const double* K9,
                               const double* Tcw16, int n_kp, const float* kp_xy, const float* des,
                               int img_w, int img_h, double radius_px, double max_dist,
                               int32_t* kp_of_point, float* uv_out, int32_t* info_out);

/* Device-resident variant (enqueue only): map arrays and keypoints / descriptors are device pointers
 * (an incrementally maintained SoA map - slam/core/landmark_utils.py of the overlay - keeps the
 * former on the GPU, sslam_aliked_extract_dev writes the latter); K9 / Tcw16 stay host values.
 * kp_of_point[n_points], uv_out (may be NULL), info_out[4] = {matches, candidate-list overflow flag,
 * candidate points, 0} are device buffers. */
int sslam_reproject_match_dev(sslam_ctx* ctx, int n_points, const double* pts3d,
                              const int32_t* obs_cnt, const float* obs_desc, const double* K9,
                              const double* Tcw16, int n_kp, const float* kp_xy, const float* des,
                              int img_w, int img_h, double radius_px, double max_dist,
                              int32_t* kp_of_point, float* uv_out, int32_t* info_out);

/* The Hamming branch of the same function for binary descriptors (`des_cur.dtype == np.uint8`: ORB 32 bytes,
 * AKAZE 61): `_desc_distance` (:78-112) takes cv2.norm(a, b, NORM_HAMMING), the threshold is `max_hamm`.
 * Projection, radius search and the greedy pass are the float entries'; only the pair score differs: the
 * minimum over the point's stored rows of popcount(obs ^ des), exact.
 *   obs_desc_u8[n_points*6*64] uint8: the `desc_bytes`-wide rows among the point's last six observations,
 *     valid ones first, every row zero from desc_bytes to 64;  obs_cnt as above
 *   des_u8[n_kp*desc_bytes] contiguous rows (what sslam_orb_detect_* writes as desc);  desc_bytes 2..64
 *   max_hamm: a decision with best distance == max_hamm is accepted (the reference rejects `best_d > thr`)
 *   Equal minima: the LOWEST keypoint index wins.  The reference takes the first in cKDTree's traversal
 *   order, which is unspecified; the two can differ only on a decision that is accepted and tied.
 *   The other arguments, the status and info_out are those of sslam_reproject_match_host. */
int sslam_reproject_match_hamming_host(sslam_ctx* ctx, int n_points, const double* pts3d,
                                       const int32_t* obs_cnt, const uint8_t* obs_desc_u8,
                                       const double* K9, const double* Tcw16, int n_kp,
                                       const float* kp_xy, const uint8_t* des_u8, int desc_bytes,
                                       int img_w, int img_h, double radius_px, double max_hamm,
                                       int32_t* kp_of_point, float* uv_out, int32_t* info_out);

/* Device-resident variant (enqueue only), as sslam_reproject_match_dev; obs_desc_u8 16-byte aligned.
 *   n_kp_dev (may be NULL): device int32, the keypoint count a detector left (sslam_orb_detect_dev's
 *   n_out); clamped to [0, n_kp] and read by the kernels, so no synchronisation between detector and
 *   association.  Rows at and beyond the count are never matched. */
int sslam_reproject_match_hamming_dev(sslam_ctx* ctx, int n_points, const double* pts3d,
                                      const int32_t* obs_cnt, const uint8_t* obs_desc_u8,
                                      const double* K9, const double* Tcw16, int n_kp,
                                      const float* kp_xy, const uint8_t* des_u8, int desc_bytes,
                                      int img_w, int img_h, double radius_px, double max_hamm,
                                      int32_t* kp_of_point, float* uv_out, int32_t* info_out,
                                      const int32_t* n_kp_dev);

/* ------------------------------------------------------- brute-force matcher
 * Replaces `cv2.BFMatcher(norm, crossCheck).match(des0, des1)` as `feature_matcher` calls it on the OpenCV branch
 * (slam/core/features_utils.py:173-178; the matcher is built at :54-55 with NORM_HAMMING for ORB / AKAZE, NORM_L2 for
 * SIFT, crossCheck=True): the nearest train row of every query row, with crossCheck only the mutual pairs.
 *   norm : 6 = NORM_HAMMING: q, t are uint8 [rows][D], D = 1..256 bytes; d = popcount of the XOR, exact
 *          4 = NORM_L2: q, t are float32 [rows][D], D = 1..512; d = sqrtf(sum_k (a_k - b_k)^2) in float32, the difference
 *              form, one accumulator per pair, k ascending, acc = fmaf(diff, diff, acc), a correctly rounded root
 *          (cv2's values; anything else is refused)
 *   nearest = strictly smallest d, the lowest index on a tie (for L2 compared AFTER the root); a NaN distance, or one not
 *   below FLT_MAX, never wins, and a row without a winner has no match
 *   cross_check 0: one match per query row that has a winner;  else: only where the train row's nearest query is that row
 *   M, N : rows of q and t, 0..65536 each (M == 0 or N == 0: k_out = 0, no device work)
 *   ij_out[M][2] int32 (queryIdx, trainIdx), ascending queryIdx;  dist_out[M] float32;  k_out : the match count
 * The M x N distances are never stored: scratch is 8 (M + N) bytes of the context's buffer.  The outputs are bitwise the
 * same from run to run. */
int sslam_bf_match_host(sslam_ctx* ctx, int norm, int cross_check, int D, const void* q, int M, const void* t, int N,
                        int32_t* ij_out, float* dist_out, int32_t* k_out);
/* Device-pointer variant; enqueue only.  M, N bound the rows of the input arrays; m_dev / n_dev (device int32[1], may be
 * NULL) carry the actual counts when they are only known on the device (written by sslam_aliked_extract_dev), clamped to
 * [0, bound]: a negative count is an empty set.  Rows beyond the counts are never read.
 *   ij_out_dev[M][2], dist_out_dev[M];  info_out_dev[4] int32 = {K, m, n, 0}
 * ij_out_dev and info_out_dev[0] are what sslam_fmat_ransac_dev takes as ij_dev / n_dev, as sslam_lightglue_match_dev's are.
 * The context's scratch buffer is (re)allocated when M + N grows: call once with the largest bounds before capturing or
 * pipelining. */
int sslam_bf_match_dev(sslam_ctx* ctx, int norm, int cross_check, int D, const void* q_dev, int M, const int32_t* m_dev,
                       const void* t_dev, int N, const int32_t* n_dev, int32_t* ij_out_dev, float* dist_out_dev,
                       int32_t* info_out_dev);

/* k nearest neighbours: `cv2.BFMatcher(norm).knnMatch(des0, des1, k)` without crossCheck, k = 1..8 (anything else is
 * refused).  norm, D, M, N, the distances and their limits are those of sslam_bf_match_host: the kernels share one
 * arithmetic chain (csrc/bf_tile.hpp), so a distance here has the bits it has there.
 *   The neighbours of query row i are its valid train rows (d < FLT_MAX; a NaN never is) in ascending order of the key
 *   (float32 d, train index) - the lower index first on a tie -, the first min(k, number of valid rows) of them.  The order
 *   is total: the result does not depend on `splits`, and is bitwise the same from run to run.
 *   idx_out[M][k] int32, padded with -1;  dist_out[M][k] float32, padded with +inf;  cnt_out[M] int32 neighbours per row
 *   splits : the train tiles (64 rows each) of a row tile are shared out among this many workgroups.  0: chosen by the
 *            host plan (csrc/bf_knn_plan.hpp) so that the grid fills the device about twice; 1..ceil(N / 64) is honoured;
 *            anything else is refused
 *   M == 0: nothing is written.  N == 0: every row gets cnt 0 and the padding, no device work.
 * The M x N distances are never stored.  Scratch: 8 * splits * M * K bytes of the context's buffer, K the smallest of
 * 2 / 4 / 8 that is >= k.  Not built: k > 8, masks, radiusMatch, train collections, NORM_L1 / NORM_HAMMING2 / NORM_L2SQR. */
int sslam_bf_knn_match_host(sslam_ctx* ctx, int norm, int D, const void* q, int M, const void* t, int N, int k, int splits,
                            int32_t* idx_out, float* dist_out, int32_t* cnt_out);
/* Device-pointer variant; enqueue only (no allocation, no synchronisation).  m_dev / n_dev as for sslam_bf_match_dev:
 * clamped to [0, bound], negative = empty, rows beyond the counts are never read.  Rows of the outputs at and beyond the
 * device count m are NOT written.
 *   idx_out_dev[M][k], dist_out_dev[M][k], cnt_out_dev[M];  info_out_dev[4] int32 = {m, n, k, splits used}
 * The context's scratch buffer is (re)allocated when splits * M * K grows: call once with the largest bounds before capturing
 * or pipelining. */
int sslam_bf_knn_match_dev(sslam_ctx* ctx, int norm, int D, const void* q_dev, int M, const int32_t* m_dev,
                           const void* t_dev, int N, const int32_t* n_dev, int k, int splits, int32_t* idx_out_dev,
                           float* dist_out_dev, int32_t* cnt_out_dev, int32_t* info_out_dev);

/* Lowe's ratio test on the two nearest neighbours: query row i is kept iff it has two neighbours and
 * (double)d1 < ratio * (double)d2 - ONE fp64 multiply, bit for bit Python's `m.distance < ratio * n.distance` on the
 * DMatch floats of knnMatch(k = 2); an equality is dropped.  ratio must be finite and > 0.
 *   ij_out[M][2] int32 (queryIdx, trainIdx of the nearest), ascending queryIdx;  dist_out[M] float32 = d1;  k_out: the count
 * splits, limits and scratch (K = 2) as for sslam_bf_knn_match_host. */
int sslam_bf_ratio_match_host(sslam_ctx* ctx, int norm, int D, const void* q, int M, const void* t, int N, double ratio,
                              int splits, int32_t* ij_out, float* dist_out, int32_t* k_out);
/* Device-pointer variant; enqueue only.  The outputs have the layout sslam_bf_match_dev leaves - ij_out_dev[M][2],
 * dist_out_dev[M], info_out_dev[4] = {K, m, n, 0} -, so ij_out_dev and info_out_dev are what sslam_fmat_ransac_dev takes as
 * ij_dev / n_dev with nothing read back in between. */
int sslam_bf_ratio_match_dev(sslam_ctx* ctx, int norm, int D, const void* q_dev, int M, const int32_t* m_dev,
                             const void* t_dev, int N, const int32_t* n_dev, double ratio, int splits, int32_t* ij_out_dev,
                             float* dist_out_dev, int32_t* info_out_dev);

/* ----------------------------------------------------------------------- ORB
 * Replaces `cv2.ORB_create(nfeatures, scaleFactor, nlevels, edgeThreshold, 0, 2, scoreType, 31, fastThreshold)
 * .detectAndCompute(img, None)` for 8-bit images, the detector of the reference's default configuration
 * (`--detector orb --matcher bf`, slam/core/features_utils.py:33-55): grey, the INTER_LINEAR_EXACT pyramid (every level
 * stored with a reflect-101 border of max(edgeThreshold, 22, 4) + 1), FAST-9/16 with OpenCV's corner score, strict
 * 8-neighbour non-maximum suppression, the border filter, retainBest by FAST score (ties kept), the Harris response (block 7,
 * k = 0.04, exact integer sums, float32 tail) and retainBest to the level's quota (ties kept), the intensity-centroid angle
 * through fastAtan2's polynomial, and the 256-bit rotated BRIEF on the 7x7 sigma-2 blurred level.  tests/orb_ref.py restates
 * every stage and names what could not be confirmed without cv2 (parity is unpinned); the kernels equal it bit for bit.
 * THE STATED DEVIATION: for patchSize 31 OpenCV samples a learned table of 256 pairs, which is not available here.  The
 * default pattern is the one OpenCV generates for every other patch size (makeRandomPattern: cv::RNG(0x34985739), 512 points,
 * x then y of each from uniform(-15, 16)) - the orb_default_pattern entry below returns it: keypoints are meant to equal
 * cv2's, descriptors are self-consistent (all frame-to-frame matching needs) but NOT interchangeable with descriptors that cv2
 * computed.  `pattern_or_null`: int8 [512][2] (x, y), every coordinate in -15..15, for a user who has the learned table.
 * THE ORDER: level ascending, then response descending, then y, then x (OpenCV's own order within a level is unspecified).
 * Accepted: nfeatures 1..2^20, scale_factor in (1, 2] (rounded to float32 first, as cv2's binding passes it), nlevels 1..16,
 * edge_threshold >= 3, score_type 0 (HARRIS_SCORE) or 1 (FAST_SCORE), fast_threshold 1..254, 1 <= max_w, max_h <= 16384;
 * firstLevel 0, WTA_K 2 and patchSize 31 are the only forms and have no argument.  A level with a side below
 * 2 edge_threshold + 1 yields no keypoints (neither does any later one); that is not an error.
 * Ties at a cut are never dropped, so a call can return more than nfeatures rows: capacity = the sum over the levels of
 * ceil(w_l / 2) ceil(h_l / 2) at max_w x max_h (strict NMS leaves no two 8-adjacent survivors) bounds the rows of every
 * output array of every call.  An instance holds 76 bytes of device memory per row of it (20 of candidate and key arrays,
 * 56 of the host entry's outputs) beside the two pyramids: 28 MB at 1241 x 376, about 0.5 GB at 4096 x 2160.  The output
 * position of a keypoint is found by counting the keys of its level below its own, n^2 / 64 comparisons per wavefront for n
 * survivors in a level: microseconds at quota size (1303 in level 0 at nfeatures 6000), and the worst case - an image whose
 * ties fill a level's NMS bound, 116 000 at 1241 x 376 - is 1.3e10 comparisons; bounded, not measured. */
typedef struct sslam_orb sslam_orb;
int sslam_orb_create(sslam_ctx* ctx, int max_w, int max_h, int nfeatures, double scale_factor, int nlevels,
                     int edge_threshold, int score_type, int fast_threshold, const int8_t* pattern_or_null, sslam_orb** out);
int sslam_orb_destroy(sslam_orb* o);
int sslam_orb_capacity(sslam_orb* o, int* cap);
int sslam_orb_default_pattern(int8_t* pattern_out);      /* int8 [512][2]; needs no device */
/* img uint8 [h][w][c], c in {1, 3 (BGR), 4 (BGRA)}, w <= max_w and h <= max_h (a larger image is refused, never clipped).
 * Out, each with `capacity` rows of which the first *n_out are written (the host entry may also leave unspecified bytes in
 * later rows): xy float32 [cap][2] level pixel * scale; aux float32 [cap][4] = size (31 * scale), angle (degrees), response,
 * octave; desc uint8 [cap][32].  One synchronisation, at the end. */
int sslam_orb_detect_host(sslam_orb* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out,
                          uint8_t* desc_out, int32_t* n_out);
/* Device-pointer variant; enqueue only, no synchronisation.  n_out_dev: device int32[1], the count as
 * sslam_bf_match_dev reads its m_dev / n_dev; desc_out_dev is its q_dev / t_dev with D = 32 and xy_out_dev is
 * sslam_fmat_ransac_dev's xy1 / xy2, so ORB -> brute-force match -> F-matrix filter runs without a host round trip.
 * The matcher's row bounds M, N stop at 65536 while `capacity` is the NMS worst case (361 991 rows at 1241 x 376): hand it
 * M = N = min(capacity, 65536), and the same as the filter's n_max.  The matcher clamps the device count to its bound, so of a
 * frame with more keypoints than that (ties on a large frame; a quota never reaches it) only the first 65536 rows in output
 * order - the finest levels - are matched; the rows beyond stay in the arrays and in the count, unmatched. */
int sslam_orb_detect_dev(sslam_orb* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev, float* aux_out_dev,
                         uint8_t* desc_out_dev, int32_t* n_out_dev);
/* test hooks, after a call.  level_info: info8 = {w, h, stored stride, stored rows, stored (0 / 1), quota, candidate
 * capacity, border} of a level of the last frame.  stage_read: a stored level back to the host, any pointer may be NULL:
 * img / blur uint8 [rows][stride] (border included), cand int32 [capacity][4] = x, y, FAST score, response bits (float32;
 * a quiet NaN where the first cut dropped the candidate) of the *ncand candidates after NMS and the border filter in
 * arrival order, cuts[2] = the first cut (a FAST score; 0: nothing dropped, 256: everything) and the bits of the second
 * (a float32 response; -inf: nothing dropped). */
int sslam_orb_level_info(sslam_orb* o, int level, int* info8);
int sslam_orb_stage_read(sslam_orb* o, int level, uint8_t* img, uint8_t* blur, int32_t* cand, int32_t* ncand, int32_t* cuts);

/* ---------------------------------------------------------------------- SIFT
 * Replaces `cv2.SIFT_create(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma).detectAndCompute(img, None)`
 * for 8-bit images, the float-descriptor detector of the reference's OpenCV branch (`--detector sift`,
 * slam/core/features_utils.py:33-55): grey, the doubled base image (firstOctave -1), the Gaussian scale space of
 * nOctaveLayers + 3 layers per octave (each layer blurred from the one before it, reflect-101), the DoG, the 26-neighbour
 * extrema with ties, adjustLocalExtrema with the contrast and edge tests, the 36-bin orientation histogram with its peaks,
 * removeDuplicatedSorted, retainBest(nfeatures) with ties kept (0: no cut), and the 4 x 4 x 8 descriptor as float32 rows of
 * 128 integer values.  tests/sift_ref.py restates every stage and names what could not be confirmed without cv2 (parity is
 * unpinned); the kernels equal it bit for bit.
 * THE DEFINED ARITHMETIC: float32, one IEEE operation at a time; exp, pow, cos, sin are the float64 function of the float32
 * argument rounded once; the two histograms are sums of 64-bit integers at the scale 2^32 (exact and order-free), converted
 * back to float32 once - a stated departure from OpenCV's build-dependent float accumulation.
 * THE ORDER: KeyPoint_LessThan's - x, y ascending, size descending, angle ascending (OpenCV's own order after retainBest is
 * unspecified).  Duplicates (same pt, size, angle) are dropped before the quota; ties at the quota are kept, so a call can
 * return more than nfeatures rows.
 * Accepted: nfeatures 0..2^20, n_octave_layers 1..8, contrast_threshold > 0, edge_threshold > 0, sigma in (0.5, 8],
 * 1 <= max_w, max_h <= 16384; descriptorType CV_32F and enable_precise_upscale false are the only forms and have no argument.
 * An octave with a side <= 10 yields nothing and an image too small for an octave yields no keypoint; neither is an error.
 * CAPACITIES: extrema have no NMS-style bound (ties are candidates).  An instance holds max_candidates extrema (0: one per
 * 32 pixels of the doubled max_w x max_h frame, at least 1024) and max_keypoints rows (0: the same, or max(4 nfeatures,
 * 16384) if that is less) - the keypoints after the orientation, before duplicates and the quota, which bound the rows of
 * every output array.  A frame that exceeds either is VOIDED, never truncated: the device count is 0, a sticky per-instance
 * word is set (sslam_sift_overflow: bit 0 candidates, bit 1 rows; it is never cleared) and the host entry returns 3 with a
 * message that names the counts the frame needed.
 * DEVICE MEMORY, by arithmetic: 2 L + 5 float planes of the doubled frame x 4/3 (Gaussian and DoG slabs) + 2 planes of
 * temporaries, 208 bytes per candidate and 576 per row: about 0.15 GB at 1241 x 376 and 2.6 GB at 4096 x 2160 at nfeatures
 * 6000 (3.2 GB at nfeatures 0, where the rows default to the candidates).  SSLAM_MAX_IMAGE_H / _W shrink it, as for ORB. */
typedef struct sslam_sift sslam_sift;
int sslam_sift_create(sslam_ctx* ctx, int max_w, int max_h, int nfeatures, int n_octave_layers, double contrast_threshold,
                      double edge_threshold, double sigma, int max_candidates, int max_keypoints, sslam_sift** out);
int sslam_sift_destroy(sslam_sift* o);
int sslam_sift_capacity(sslam_sift* o, int* rows, int* candidates_or_null);
int sslam_sift_overflow(sslam_sift* o, int* word);       /* the sticky word; synchronises the stream */
/* img uint8 [h][w][c], c in {1, 3 (BGR), 4 (BGRA)}, w <= max_w and h <= max_h (a larger image is refused, never clipped).
 * Out, each with `rows` rows of which the first *n_out are written: xy float32 [rows][2]; aux float32 [rows][3] = size,
 * angle (degrees), response; octave int32 [rows], cv2's packed field (octave byte -1 = 255 for the doubled octave, layer
 * << 8, cvRound((xi + 0.5) 255) << 16); desc float32 [rows][128].  Two synchronisations (the count, then the rows). */
int sslam_sift_detect_host(sslam_sift* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out,
                           int32_t* octave_out, float* desc_out, int32_t* n_out);
/* Device-pointer variant; enqueue only, no synchronisation.  n_out_dev: device int32[1], the count as sslam_bf_match_dev
 * reads its m_dev / n_dev; desc_out_dev is its q_dev / t_dev with NORM_L2 and D = 128 and xy_out_dev is
 * sslam_fmat_ransac_dev's xy1 / xy2, so SIFT -> brute-force match -> F-matrix filter runs without a host round trip.  The
 * matcher's row bounds stop at 65536: hand it M = N = min(rows, 65536), as for ORB.  A voided frame writes the count 0. */
int sslam_sift_detect_dev(sslam_sift* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev, float* aux_out_dev,
                          int32_t* octave_out_dev, float* desc_out_dev, int32_t* n_out_dev);
/* test hooks, after a call.  octave_info: info8 = {w, h, octaves computed, Gaussian layers, has an interior (0 / 1), the
 * integer contrast threshold, max_candidates, max_keypoints} of an octave of the last frame (w = h = 0 beyond the last).
 * stage_read: any pointer may be NULL: gauss float32 [L + 3][h][w] and dog float32 [L + 2][h][w] of the octave; of the whole
 * frame, in arrival order: cand int32 [max_candidates][4] = octave, layer, r, c; ref int32 [max_candidates][8] = passed
 * (0 / 1), r, c, layer after the refinement, the packed octave field, and the float32 bits of x, y, size in the frame of the
 * doubled image; hist float32 [max_candidates][40] = the smoothed orientation histogram and, at [36], the response (rows of
 * candidates that did not pass are unspecified); counts[4] = extrema, keypoints before duplicates, output rows, 0. */
int sslam_sift_octave_info(sslam_sift* o, int octave, int* info8);
int sslam_sift_stage_read(sslam_sift* o, int octave, float* gauss, float* dog, int32_t* cand, int32_t* ref, float* hist,
                          int32_t* counts);

/* --------------------------------------------------------------------- AKAZE
 * Replaces `cv2.AKAZE_create(descriptor_type, descriptor_size, descriptor_channels, threshold, nOctaves, nOctaveLayers,
 * diffusivity, max_points).detectAndCompute(img, None)` for 8-bit images, the third detector of the reference's OpenCV
 * branch (`--detector akaze`, slam/core/features_utils.py:33-55): grey / 255, the nonlinear scale space (Gaussian level 0,
 * kcontrast as the 70th percentile of the Scharr magnitude, per level the PM-G2 conductivity and the FED cycle of explicit
 * diffusion steps, halving at a new octave), the scaled-Scharr Hessian determinant, strict 3 x 3 maxima above `threshold`,
 * suppression across the same and the adjacent levels, the 2-D subpixel refinement, retainBest(max_points) with ties kept
 * (-1: no cut), the SURF-style main orientation and the full 3-channel M-LDB descriptor: 486 bits in uint8 rows of 61.
 * tests/akaze_ref.py restates every stage and names what could not be confirmed without cv2 (parity is unpinned); the
 * kernels equal it bit for bit.
 * THE DEFINED ARITHMETIC: float32, one IEEE operation at a time; sqrt correctly rounded; cos, sin the float64 function rounded
 * once; fastAtan2 ORB's polynomial; filter taps ascending through a float32 intermediate; the orientation windows and the
 * M-LDB cell sums are 64-bit integers at the scale 2^32 (exact and order-free) - stated departures from OpenCV's
 * build-dependent accumulation.  SUPPRESSION is a predicate: a candidate is dropped iff a candidate of its own or an adjacent
 * level within its radius (esigma * 1.5, full-resolution pixels) has a larger response, or an equal one and a lower (level,
 * row, column); OpenCV's scan depends on the order it meets the candidates.
 * THE ORDER: class_id (the level's index) ascending, then the candidate's row, then its column.
 * Accepted: descriptor_type 5 (DESCRIPTOR_MLDB), descriptor_size 0, descriptor_channels 3, diffusivity 1 (DIFF_PM_G2) -
 * anything else is refused with status 2 and a message naming the value, before any HIP call - threshold finite and > 0,
 * n_octaves 1..8, n_octave_layers 1..8, max_points -1 or 1..2^20, 1 <= max_w, max_h <= 16384.  An octave other than 0 below
 * 80 x 40 ends the pyramid; a frame without a pixel inside level 0's border (a side <= 10) yields no keypoint; neither is an
 * error.
 * CAPACITIES: an instance holds max_candidates candidates (0: one per 8 pixels of max_w x max_h, at least 1024) and
 * max_keypoints rows (0: one per 16 pixels, at least 1024, or max(4 max_points, 16384) if that is less) - the refined
 * keypoints before the quota, which bound the rows of every output array.  A frame that exceeds either is VOIDED, never
 * truncated: the device count is 0, a sticky per-instance word is set (sslam_akaze_overflow: bit 0 candidates, bit 1 rows; it
 * is never cleared) and the host entry returns 3 with a message that names the counts the frame needed.
 * DEVICE MEMORY, by arithmetic: 5 float planes per level (Lt, Lflow, Lx, Ly, Ldet; L levels per octave, octaves x 4/3) + 5
 * full-size temporaries, 20 bytes per candidate and 141 per row: about 0.06 GB at 1241 x 376 and 1.3 GB at 4096 x 2160 with
 * the defaults.  SSLAM_MAX_IMAGE_H / _W shrink it, as for ORB. */
typedef struct sslam_akaze sslam_akaze;
int sslam_akaze_create(sslam_ctx* ctx, int max_w, int max_h, int descriptor_type, int descriptor_size, int descriptor_channels,
                       double threshold, int n_octaves, int n_octave_layers, int diffusivity, int max_points, int max_candidates,
                       int max_keypoints, sslam_akaze** out);
int sslam_akaze_destroy(sslam_akaze* o);
int sslam_akaze_capacity(sslam_akaze* o, int* rows, int* candidates_or_null);
int sslam_akaze_overflow(sslam_akaze* o, int* word);     /* the sticky word; synchronises the stream */
/* img uint8 [h][w][c], c in {1, 3 (BGR), 4 (BGRA)}, w <= max_w and h <= max_h (a larger image is refused, never clipped).
 * Out, each with `rows` rows of which the first *n_out are written: xy float32 [rows][2]; aux float32 [rows][3] = size,
 * angle (degrees), response; lvl int32 [rows][2] = octave, class_id; desc uint8 [rows][61], contiguous, nothing written
 * beyond byte 60 of a row.  Two synchronisations (the count, then the rows). */
int sslam_akaze_detect_host(sslam_akaze* o, const uint8_t* img, int h, int w, int c, float* xy_out, float* aux_out,
                            int32_t* lvl_out, uint8_t* desc_out, int32_t* n_out);
/* Device-pointer variant; enqueue only, no synchronisation.  n_out_dev: device int32[1], the count as sslam_bf_match_dev
 * reads its m_dev / n_dev; desc_out_dev is its q_dev / t_dev with NORM_HAMMING and D = 61 and xy_out_dev is
 * sslam_fmat_ransac_dev's xy1 / xy2.  The matcher's row bounds stop at 65536: hand it M = N = min(rows, 65536), as for ORB.
 * A voided frame writes the count 0. */
int sslam_akaze_detect_dev(sslam_akaze* o, const uint8_t* img_dev, int h, int w, int c, float* xy_out_dev, float* aux_out_dev,
                           int32_t* lvl_out_dev, uint8_t* desc_out_dev, int32_t* n_out_dev);
/* test hooks, after a call.  level_info: info12 = {w, h, levels computed, octaves computed, octave, sigma_size, border, runs in
 * one workgroup (0 / 1), FED steps into the level, level 0 has an interior (0 / 1), max_candidates, max_keypoints} of a level
 * of the last frame (w = h = 0 beyond the last).  stage_read, of a frame with an interior; any pointer may be NULL: lt, lflow
 * (untouched for level 0), lx, ly, ldet float32 [h][w] of the level; of the whole frame: kcontrast8 float32 [8] per octave;
 * in arrival order cand int32 [max_candidates][4] = level, r, c, response bits; cflag int32 [max_candidates] = 0 suppressed,
 * 1 a keypoint, 2 survives but the refinement rejects it; kp uint32 [max_keypoints][8] = the float32 bits of x, y, size,
 * angle, response, then octave, class_id, candidate index (the angle is set for kept rows); kflag int32 [max_keypoints] =
 * kept by the quota; counts[4] = candidates, keypoints before the quota, output rows, 0. */
int sslam_akaze_level_info(sslam_akaze* o, int level, int* info12);
int sslam_akaze_stage_read(sslam_akaze* o, int level, float* lt, float* lflow, float* lx, float* ly, float* ldet, float* kcontrast8,
                           int32_t* cand, int32_t* cflag, uint32_t* kp, int32_t* kflag, int32_t* counts);

/* ------------------------------------------------------ keyframe thumbnails
 * Replaces `cv2.resize(bgr, hw)` + `cv2.imencode('.jpg', th, [cv2.IMWRITE_JPEG_QUALITY, q])` of `make_thumb`
 * (slam/core/keyframe_utils.py:26-30): cv2.resize for uint8 / INTER_LINEAR in OpenCV's fixed-point form, libjpeg's integer
 * Y Cb Cr and 4:2:0 subsampling, an exactly defined integer forward DCT and quantisation with libjpeg's tables for the quality,
 * baseline Huffman coding with the Annex K tables, byte stuffing and the JFIF header - all on the device, eight launches on the
 * context's stream.  A one-channel source gives a one-component JPEG, 3 or 4 channels (B G R [A], alpha dropped) Y Cb Cr.
 * Parity with cv2 itself is unpinned (tests/thumb_ref.py names what could not be confirmed).
 * One instance serves one thumbnail size and quality and any source up to max_src_w x max_src_h.  Refused with a message naming
 * the value, before any device call: quality outside 1..100, a thumbnail side outside 1..4096, a source side outside 1..16384 or
 * larger than the instance's, C not in {1, 3, 4}. */
typedef struct sslam_thumb sslam_thumb;
int sslam_thumb_create(sslam_ctx* ctx, int max_src_w, int max_src_h, int dst_w, int dst_h, int quality, sslam_thumb** out);
int sslam_thumb_destroy(sslam_thumb* t);
/* bytes no encode of this instance can exceed: header + 416 per block (20 + 63 * 26 bits, every byte stuffed) + 2 */
int sslam_thumb_capacity(sslam_thumb* t, int* capacity);
/* src uint8 [Hs][Ws][C] (host) -> the JPEG stream in out[0 .. *nbytes) (host, cap bytes; sslam_thumb_capacity always suffices) */
int sslam_thumb_encode_host(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* out, int cap, int* nbytes);
/* device pointers; enqueue only: out_dev holds sslam_thumb_capacity bytes, the int32 byte count is left at nbytes_dev */
int sslam_thumb_encode_dev(sslam_thumb* t, const uint8_t* src_dev, int Hs, int Ws, int C, uint8_t* out_dev, int32_t* nbytes_dev);
/* the resize alone: dst uint8 [dst_h][dst_w][C] (host), every channel interpolated */
int sslam_thumb_resize_host(sslam_thumb* t, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst);
/* for tests, of the LAST encode (synchronises).  which: 0 the resized image uint8 [dst_h][dst_w][C] (computed now, from the last
 * encode's source, which must still be alive); 1 Y uint8 [yh][yw] padded to the MCU multiple; 2 / 3 Cb / Cr uint8 [yh/2][yw/2];
 * 4 coefficients int16 [blocks][64], zigzag order, blocks in scan order; 5 bit offsets uint32 [blocks] */
int sslam_thumb_stage_read(sslam_thumb* t, int which, void* dst);

/* ------------------------------------------------------- semi-global stereo
 * Replaces `cv2.StereoSGBM_create(...).compute(left, right)` of the reference's stereo prototype
 * (refrences/sfm_lightglue_aliked.py:109-121, :357-361) and the lookup + `cv2.triangulatePoints(Proj, Proj_r, ...)` behind it
 * (:363-396).  8-bit input, MODE_SGBM (single pass, five paths), no speckle filter; integers only, defined stage by stage in
 * tests/stereo_ref.py, which the device equals bit for bit.  Parity with cv2 itself is unpinned (the restatement's UNCONFIRMED).
 * Normalised: P1 <= 0 -> 2; P2 -> max(P2 > 0 ? P2 : 5, P1 + 1); disp12MaxDiff <= 0 -> 1 (the left-right check always runs);
 * uniquenessRatio < 0 -> 10; ftzero = max(preFilterCap, 15) | 1.  The result is int16 [H][W] in sixteenths of a pixel; columns
 * below minDisparity + numDisparities and rejected pixels hold (minDisparity - 1) * 16, as does the whole image when
 * W <= minDisparity + numDisparities (not an error).
 * Refused with a message naming the value, before any device call: mode != 0 (MODE_SGBM), speckleWindowSize > 0, minDisparity < 0,
 * numDisparities not a multiple of 16 in 16..256, blockSize even or outside 1..11, preFilterCap outside 0..63,
 * uniquenessRatio > 100, a side outside 1..16384, a parameter set whose largest block cost
 * (blockSize^2 * ((2 ftzero >> 2) + 63)) + P2 exceeds 32767, a workspace above 4 GiB. */
typedef struct sslam_sgbm sslam_sgbm;
int sslam_sgbm_create(sslam_ctx* ctx, int max_w, int max_h, int minDisparity, int numDisparities, int blockSize, int P1, int P2,
                      int disp12MaxDiff, int preFilterCap, int uniquenessRatio, int speckleWindowSize, int speckleRange, int mode,
                      sslam_sgbm** out);
int sslam_sgbm_destroy(sslam_sgbm* g);
/* left, right uint8 [H][W][channels] (host), channels 1, 3 or 4: 3 and 4 (B G R [A]) are converted to grey first - the
 * prototype's call order, NOT cv2's per-channel cost.  disp int16 [H][W] (host). */
int sslam_sgbm_compute_host(sslam_sgbm* g, const uint8_t* left, const uint8_t* right, int H, int W, int channels, int16_t* disp);
/* device pointers; enqueue only */
int sslam_sgbm_compute_dev(sslam_sgbm* g, const uint8_t* left_dev, const uint8_t* right_dev, int H, int W, int channels,
                           int16_t* disp_dev);
/* for tests, of the LAST compute (synchronises), W1 = max(W - minDisparity - numDisparities, 0).  which: 0 / 1 the prefiltered
 * plane of the left / right image uint8 [H][W]; 2 C, 3 S int16 [H][W1][D]; 4 the disparity before the left-right check, 5 the
 * right view's integer disparity, 6 the checked disparity before the median, each int16 [H][W] */
int sslam_sgbm_stage_read(sslam_sgbm* g, int which, void* dst);
/* The keypoint lift, a keypoint per thread.  xy float32 [n][2]; disp int16 [H][W] (a compute's output).  d = disp[int(y)][int(x)]
 * / 16 in float32; mask = min_disp < d < max_disp, clear for a keypoint outside the image (the prototype would raise or wrap:
 * a stated departure); xy_right = (x - d, y); X = v[:3] / v[3] of the DLT null vector of (P_left, P_right) as
 * sslam_triangulate_2view computes it, |v[3]| <= 1e-12 clears the mask, X is NaN where the mask is clear.  xy_right_in != NULL:
 * the right pixels are given (disp is not read, d = x - x_right, every keypoint is a candidate).  P_left12 / P_right12 are host
 * 3 x 4 row-major, both NULL: no triangulation (X_out must be NULL).  d_out, xy_right_out, X_out may be NULL.
 * _dev: device pointers, enqueue only; n_dev (may be NULL) is a device-resident count clamped to [0, n_max], nothing is written
 * beyond it. */
int sslam_stereo_lift_host(sslam_ctx* ctx, int n, const float* xy, const float* xy_right_in, const int16_t* disp, int H, int W,
                           const double* P_left12, const double* P_right12, double min_disp, double max_disp, float* d_out,
                           float* xy_right_out, double* X_out, uint8_t* mask_out);
int sslam_stereo_lift_dev(sslam_ctx* ctx, int n_max, const int32_t* n_dev, const float* xy_dev, const float* xy_right_in_dev,
                          const int16_t* disp_dev, int H, int W, const double* P_left12, const double* P_right12, double min_disp,
                          double max_disp, float* d_out_dev, float* xy_right_out_dev, double* X_out_dev, uint8_t* mask_out_dev);

/* ------------------------------------------------------------------ ALIKED
 * Replaces `ALIKED(max_num_keypoints=...).eval().to(device)` at
 * slam/core/features_utils.py:25 and `_bgr_to_tensor` + `detector.extract` +
 * `rbd` + descriptor re-normalisation at features_utils.py:92-100, :219-222.
 * `weights` = blob from opencv-simpleslam_amd/weights.py::pack_aliked.
 * max_h/max_w bound the input image, max_kpts the keypoints per call. */
int sslam_aliked_create(sslam_ctx* ctx, const float* weights, size_t n_floats, int max_h, int max_w,
                        int max_kpts, sslam_aliked** out);
/* An instance whose _extract_batch_dev entry takes up to max_frames (<= 16) frames per call: one workspace block
 * per frame (about 0.75 GB each at the full 1056 x 1056 network capacity). */
int sslam_aliked_create_batched(sslam_ctx* ctx, const float* weights, size_t n_floats, int max_h, int max_w,
                                int max_kpts, int max_frames, sslam_aliked** out);
int sslam_aliked_destroy(sslam_aliked* al);
/* img: uint8 HWC, C = 3 (BGR as cv2.imread gives), 1 (gray) or 4 (BGRA).
 * xy_out[2*max_kpts] (x, y) in input-image pixels, desc_out[128*max_kpts]
 * unit-norm rows, score_out[max_kpts] (may be NULL), n_out = keypoints found
 * (<= max_kpts; threshold mode, ordered as upstream: raster order, or by
 * descending score when more than max_kpts pass the detection threshold; -1 on the _dev entries: range overflow, below). */
int sslam_aliked_extract_host(sslam_aliked* al, const uint8_t* img, int H, int W, int C, int max_kpts,
                              float* xy_out, float* desc_out, float* score_out, int32_t* n_out);
/* Device-pointer variant (all pointers device, n_out[1] device int32); enqueue only. */
int sslam_aliked_extract_dev(sslam_aliked* al, const uint8_t* img, int H, int W, int C, int max_kpts,
                             float* xy_out, float* desc_out, float* score_out, int32_t* n_out);
/* n_frames frames of ONE size through ONE launch sequence (the reference extracts frame by frame,
 * features_utils.py:92-100; a frame stream hands over several at once): imgs / xy_out / desc_out / score_out / n_out
 * are host arrays of n_frames device pointers (score_out, or any of its entries, may be NULL).  Every kernel carries
 * the frame in a grid dimension, so the ~50 launches of a frame become ~50 per BATCH and the small stages (1/8 and
 * 1/32 resolution maps, selection, descriptor head) fill the chip; a frame's arithmetic does not depend on the batch:
 * results are those of n_frames sslam_aliked_extract_dev calls, bit for bit.  Enqueue only. */
int sslam_aliked_extract_batch_dev(sslam_aliked* al, int n_frames, const uint8_t* const* imgs, int H, int W, int C,
                                   int max_kpts, float* const* xy_out, float* const* desc_out,
                                   float* const* score_out, int32_t* const* n_out);
/* RANGE.  The dense stages, the deformable layers and the descriptor head carry their operands as fp16 (hi, lo) plane pairs
 * (the split-precision matrix path): a FINITE activation with |value| >= 65520 does not fit.  Such a value raises the frame's
 * flag on the device; the frame's keypoint count n_out then reads -1 (sslam_lightglue_match_dev treats a negative count as an
 * empty frame), sslam_aliked_extract_host fails with a message, and the instance keeps a sticky word that this call returns
 * and clears (synchronises the stream) - for callers of the _dev / _batch_dev entries that do not read the counts.
 * sslam_aliked_create refuses weights (BN scales folded) that do not fit.  No trained checkpoint comes near the limit; the
 * guard exists so that a silent inf / NaN descriptor cannot happen. */
int sslam_aliked_range_overflow(sslam_aliked* al, int* flag_out);
/* Replay the launch sequence of sslam_aliked_extract_dev as a cached hipGraph (one graph per distinct
 * argument tuple; for callers that cycle through a fixed set of buffers).  Same results, ~10 us of
 * host time per call instead of ~45 launches. */
int sslam_aliked_use_graphs(sslam_aliked* al, int enable);
/* Test hook: copy an internal buffer to the host (see aliked_kernels.hip). */
int sslam_aliked_debug_read(sslam_aliked* al, int which, void* dst, size_t bytes);

/* ------------------------------------------------------------------ LightGlue
 * Replaces `LightGlue(features='aliked').eval().to(device)` at
 * slam/core/features_utils.py:26 and the forward + confidence filter at
 * features_utils.py:157-169.  `weights` is the fp32 blob produced by
 * opencv-simpleslam_amd/weights.py::pack_lightglue from an upstream state dict
 * (host pointer, copied).  max_kpts bounds M and N of every later call. */
int sslam_lightglue_create(sslam_ctx* ctx, const float* weights, size_t n_floats, int max_kpts,
                           sslam_lightglue** out);
/* Same, with workspace for up to max_pairs (1..16) pairs per sslam_lightglue_match_batch_dev call.
 * sslam_lightglue_create == max_pairs 1.  Workspace is ~60 MB per pair at max_kpts 2048. */
int sslam_lightglue_create_batched(sslam_ctx* ctx, const float* weights, size_t n_floats, int max_kpts,
                                   int max_pairs, sslam_lightglue** out);
int sslam_lightglue_destroy(sslam_lightglue* lg);
int sslam_lightglue_capacity(sslam_lightglue* lg, int* kc_out);
int sslam_lightglue_batch_capacity(sslam_lightglue* lg, int* pairs_out);
/* Upstream conf: depth_confidence 0.95, width_confidence 0.99, filter_threshold
 * 0.1; prune_min_kpts = pruning_keypoint_thresholds[device] (-1 on CPU: pruning
 * evaluated after every layer; pass a value >= max_kpts to disable). */
int sslam_lightglue_set_conf(sslam_lightglue* lg, float depth_confidence, float width_confidence,
                             float filter_threshold, int prune_min_kpts);
/* Arithmetic of the 9 transformer layers.  0: every contraction on the exact-fp32 matrix-core
 * instruction (v_mfma_f32_32x32x2_f32).  1: fp16 hi/lo split operands, three
 * v_mfma_f32_32x32x16_f16 per product, fp32 accumulation (~2^-22 relative error per product).
 * 2 (DEFAULT since r05): as 1, but attention carries the softmax weights P as ONE fp16 plane in P.V (two MFMAs per product
 * there, the row sum over the rounded weights): -12 % attention time.  On north_star's bar (match indices, floats within 1e-3)
 * modes 1 and 2 are indistinguishable over 131 199 oracle matches - the same two score-at-threshold events, score error
 * 4.4e-5 / 1.06e-4 (profiles/r05_flip_soak.md); token states 2.4e-5 from exact in mode 2, 4e-6 in mode 1.
 * final_proj and the similarity GEMM run on the same split-operand pipe in modes 1 and 2 (exact-fp32 instruction in
 * mode 0); the dual softmax, the arg-max and the score arithmetic are fp32 in every mode. */
int sslam_lightglue_set_precision(sslam_lightglue* lg, int mode);
/* xy0[M*2], desc0[M*128], xy1[N*2], desc1[N*128] float32.
 * ij_out[2*min(M,N)] int32 (queryIdx, trainIdx) pairs, ascending queryIdx;
 * score_out[min(M,N)]; only matches with score > filter_threshold AND
 * score > min_conf (features_utils.py:167-169) are emitted.
 * M == 0 or N == 0 -> k_out = 0 (features_utils.py:118-124). */
int sslam_lightglue_match_host(sslam_lightglue* lg, const float* xy0, const float* desc0, int M,
                               const float* xy1, const float* desc1, int N, float min_conf,
                               int32_t* ij_out, float* score_out, int32_t* k_out,
                               int32_t* stop_layer_out);
/* The same with the 'image_size' of each feature set (size0 / size1: host float[2] = (W, H), or NULL): LightGlue then
 * normalises the keypoints by the image size instead of their bounding box - what happens when the features
 * come straight from `extractor.extract`, i.e. the reference's legacy pair entry `_lightglue_detect_and_match`
 * (slam/core/features_utils.py:233-247; cvg/LightGlue `normalize_keypoints(kpts, size)`). */
int sslam_lightglue_match_host_sized(sslam_lightglue* lg, const float* xy0, const float* desc0, int M, const float* size0,
                                     const float* xy1, const float* desc1, int N, const float* size1, float min_conf,
                                     int32_t* ij_out, float* score_out, int32_t* k_out, int32_t* stop_layer_out);
/* Device-pointer variant; enqueue only.  M, N bound the rows of the input arrays; m_dev /
 * n_dev (device int32[1], may be NULL) carry the actual keypoint counts when they are only
 * known on the device (written by sslam_aliked_extract_dev), so an extract -> match chain
 * needs no host round trip.  info_out[4] (device) = {K, stop_layer, n0, n1 after pruning}; K = -1: range
 * overflow of the split-precision path (see sslam_lightglue_range_overflow). */
int sslam_lightglue_match_dev(sslam_lightglue* lg, const float* xy0, const float* desc0, int M,
                              const float* xy1, const float* desc1, int N, const int32_t* m_dev,
                              const int32_t* n_dev, float min_conf, int32_t* ij_out, float* score_out,
                              int32_t* info_out);
/* Batch variant: n_pairs independent pairs in ONE enqueue (every launch covers all pairs, so the chip
 * is filled without splitting the keys of a pair and the launch sequence is paid once per batch).
 * This is what a frame stream calls: the reference matches one (t-1, t) pair per frame
 * (slam/monocular/main_revamped.py:321-328); consecutive pairs are independent.
 * Host arrays of n_pairs entries: xy0[p] / desc0[p] / xy1[p] / desc1[p] device pointers, M[p] / N[p]
 * row bounds, m_dev[p] / n_dev[p] device counts (the arrays or single entries may be NULL).
 * Outputs (device): pair p writes ij_out + p*out_stride*2, score_out + p*out_stride, info_out + 4p;
 * out_stride >= min(M[p], N[p]).  Each pair's result is the one sslam_lightglue_match_dev gives.
 * Images of one call with equal source pointers (and bound) are recognised as one frame, whose part of the forward that
 * depends on one image alone is then computed once; results are unchanged. */
int sslam_lightglue_match_batch_dev(sslam_lightglue* lg, int n_pairs, const float* const* xy0,
                                    const float* const* desc0, const int32_t* const* m_dev, const int32_t* M,
                                    const float* const* xy1, const float* const* desc1,
                                    const int32_t* const* n_dev, const int32_t* N, float min_conf,
                                    int32_t* ij_out, float* score_out, int32_t* info_out, int out_stride);
/* Replay the launch sequence of sslam_lightglue_match_dev / _batch_dev as a cached hipGraph (one graph
 * per distinct argument tuple; ~190 launches become one hipGraphLaunch).  Same results. */
int sslam_lightglue_use_graphs(sslam_lightglue* lg, int enable);
/* The split-precision path carries fp32 values as fp16 plane pairs: a FINITE activation with
 * |value| >= 65520 does not fit (the exact-fp32 path, precision 0, has no such limit).  Such a value is flagged
 * on the device PER PAIR (and saturated or turned non-finite, never silently wrapped): that pair's match count
 * info_out[0] becomes -1, so the verdict travels with the result (sslam_fmat_ransac_dev clamps it to 0 matches);
 * sslam_lightglue_match_host fails with a message.  The instance also keeps a sticky word of its own (never
 * shared with other instances): callers of the _dev / _batch_dev entries that do not read info_out poll it
 * here (synchronises the stream, returns and clears it). */
int sslam_lightglue_range_overflow(sslam_lightglue* lg, int* flag_out);
/* Measurement hook (bench.py): bracket each attention launch - the dominant kernel - with HIP
 * events on the context stream; _read synchronises and returns their summed duration and count. */
int sslam_lightglue_profile(sslam_lightglue* lg, int enable);
int sslam_lightglue_profile_read(sslam_lightglue* lg, float* total_ms_out, int32_t* launches_out);
/* Test hooks: limit the executed layers; copy an internal buffer to the host.
 * debug_key_split: 0 = by batch size (no split for batched launches, 2 or 4 key ranges for one pair, merged by the fused
 * FFN's tiles; the hand-scheduled assembly attention kernel either way), -5 = the same with the merge as a launch of its
 * own, -4 = that policy on the r02 4-wave kernel, 1 / 2 / 4 = that
 * many key ranges (4-wave kernel), 101 / 102 / 104 = that many (assembly kernel), -1 = no split, r02 4-wave kernel,
 * -3 = no split, the assembly kernel at any batch size (for one split the two kernels give bit-identical results). */
int sslam_lightglue_debug_layers(sslam_lightglue* lg, int layers, int self_only);
int sslam_lightglue_debug_key_split(sslam_lightglue* lg, int ks);
/* Linear-kernel form: -1 by token count (default), 0 = 64-row ring kernels, 1 = batched form (128 x 128 projections +
 * the fused FFN kernel, its tile size by token count), 2 / 3 = batched form with 64- / 32-token FFN tiles forced
 * (a token's FFN arithmetic is the same in both: bit-identical), 5 = batched form with the token heads (early stop /
 * pruning inputs) as a launch of their own instead of in the cross block's fused FFN. */
int sslam_lightglue_debug_big_gemm(sslam_lightglue* lg, int mode);
/* Shared frames of one enqueue (equal xy / desc / count pointers, bound and image size): 1 (default) = the prologue and the
 * self block of layer 0 run once per distinct frame and a copy kernel hands the state to the other images that name it,
 * 0 = every image is computed.  Bit-identical results; the fp32 path (precision 0) always computes every image.
 * _share_info: out[0] = distinct images of the last enqueue, out[1] = 1 when its launch sequence holds that copy kernel. */
int sslam_lightglue_debug_share_frames(sslam_lightglue* lg, int enable);
int sslam_lightglue_debug_share_info(sslam_lightglue* lg, int32_t* out);
/* Precision-study hook (profiles/r04_split_study.md; the product never sets it): drop cross terms of the three-term
 * split products and measure what that does to the matches.  mask: 0x01 / 0x02 K / Q as one fp16 plane in the logits,
 * 0x04 / 0x08 P / V as one plane in the context, 0x10 / 0x20 activation low plane dropped in the projections / the FFN,
 * 0x40 / 0x80 weight low plane dropped there.  0 = the product arithmetic. */
int sslam_lightglue_debug_split_form(sslam_lightglue* lg, int mask);
int sslam_lightglue_debug_read(sslam_lightglue* lg, int which, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SSLAM_HIP_H */
