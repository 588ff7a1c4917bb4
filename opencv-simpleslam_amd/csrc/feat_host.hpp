// feat_host.hpp - the host half that the C entries of the feature detectors (orb_kernels.hip, sift_kernels.hip,
// akaze_kernels.hip) share, written ONCE: the per-call check, the staging of a host image into the context's scratch slab, and
// - for the two detectors whose lists have capacities - the capacity and overflow queries and the whole host entry.  The
// instances stay plain structs; the templates read the members they have in common: ctx, max_w, max_h, cand_cap, kp_cap, ctl
// (which begins with the counters ncand, nkp), sticky, n.  The extern "C" functions stay in their .hip files as thin wrappers.
#pragma once
#include "common.hpp"
#include "feat_plan.hpp"

#include <initializer_list>
#include <type_traits>

namespace sslam {

template <class Instance>
int feat_check_call(const char* who, Instance* o, const void* img, int h, int w, int c) {
    SSLAM_REQUIRE(o != nullptr, "%s: instance is NULL", who);
    SSLAM_REQUIRE(img != nullptr, "%s: img is NULL", who);
    char msg[160];
    if (feat_check_image(w, h, c, o->max_w, o->max_h, msg, sizeof msg)) { set_error("%s: %s", who, msg); return 2; }
    return 0;
}

// the caller's image -> the context's scratch slab, behind what is queued on the context's stream
inline int feat_stage_image(sslam_ctx* ctx, const uint8_t* img, int h, int w, int c, const uint8_t** img_dev) {
    const size_t bytes = (size_t)h * w * c;
    char* b;
    if (int rc = ctx_scratch(ctx, bytes, &b)) return rc;
    SSLAM_HIP_CHECK(hipMemcpyAsync(b, img, bytes, hipMemcpyHostToDevice, ctx->stream));
    *img_dev = (const uint8_t*)b;
    return 0;
}

template <class Instance>
int feat_capacity(const char* who, Instance* o, int* rows, int* candidates) {
    SSLAM_REQUIRE(o != nullptr && rows != nullptr, "%s: NULL argument", who);
    *rows = o->kp_cap;
    if (candidates) *candidates = o->cand_cap;
    return 0;
}

template <class Instance>
int feat_overflow(const char* who, Instance* o, int* word) {
    SSLAM_REQUIRE(o != nullptr && word != nullptr, "%s: NULL argument", who);
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    int32_t v = 0;
    SSLAM_HIP_CHECK(copy_down(o->ctx->stream, &v, o->sticky, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(o->ctx->stream));
    *word = v;
    return 0;
}

// an output array of the host entry: the caller's rows, the instance's rows on the device, the bytes of a row
struct FeatRows { void* host; const void* dev; size_t row_bytes; };
template <class T>
FeatRows feat_rows(T* host, const T* dev, size_t per_row) { return FeatRows{host, dev, per_row * sizeof(T)}; }

// The host entry of SIFT and AKAZE behind the call check: stage the image, `enqueue(img_dev)` the frame into the instance's own
// output arrays, bring down the count and the control block behind the kernels (one synchronisation), refuse a voided frame
// (`noun`: what the instance calls its candidates), then fetch the n rows of every array in `outs`.
template <class Instance, class Enqueue>
int feat_detect_host(const char* who, Instance* o, const uint8_t* img, int h, int w, int c, const char* noun, Enqueue&& enqueue,
                     std::initializer_list<FeatRows> outs, int32_t* n_out) {
    SSLAM_HIP_CHECK(hipSetDevice(o->ctx->device));
    const uint8_t* img_dev;
    if (int rc = feat_stage_image(o->ctx, img, h, w, c, &img_dev)) return rc;
    if (int rc = enqueue(img_dev)) return rc;
    hipStream_t s = o->ctx->stream;
    int32_t n = 0;
    std::remove_pointer_t<decltype(o->ctl)> ctl;
    SSLAM_HIP_CHECK(copy_down(s, &n, o->n, 1));
    SSLAM_HIP_CHECK(copy_down(s, &ctl, o->ctl, 1));
    SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    if (ctl.ncand > o->cand_cap || ctl.nkp > o->kp_cap) {
        set_error("%s: the frame has %d %s and %d keypoints before the quota, the instance holds max_candidates %d and "
                  "max_keypoints %d: the frame is voided, nothing is truncated", who, ctl.ncand, noun, ctl.nkp, o->cand_cap, o->kp_cap);
        *n_out = 0;
        return 3;
    }
    if (n > 0) {
        for (const FeatRows& r : outs) SSLAM_HIP_CHECK(hipMemcpyAsync(r.host, r.dev, (size_t)n * r.row_bytes, hipMemcpyDeviceToHost, s));
        SSLAM_HIP_CHECK(hipStreamSynchronize(s));
    }
    *n_out = n;
    return 0;
}

}  // namespace sslam
