// geom_slab.hpp - what the geometry entries (BA, LM, the F / H / E / PnP RANSACs, triangulation, relative pose, 2D-3D
// association) decide on the host about the context's scratch slab and their sample loop.  Plain C++17 with no HIP include:
// tests/test_geom_slab.py compiles it with the host compiler.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>

namespace sslam {

// One call's view of the scratch slab.  take<T>(count) places the next `count` elements on a 256-byte boundary, at least 8
// guard bytes past the piece before; `bytes` is the slab size so far.  Each family's bind function assigns every slab-backed
// pointer of its kernel arguments with take<T>(count) in one fixed order, and an entry runs it twice: with base == nullptr
// it only measures (every pointer is null, `bytes` is what ctx_scratch must provide), bound to the slab it yields the pieces.
struct Slab {
    char* base = nullptr;
    size_t bytes = 0;
    template <class T>
    T* take(size_t count) {
        const size_t o = bytes;
        bytes = (bytes + count * sizeof(T) + 8 + 255) / 256 * 256;
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};

// The sample loop of a RANSAC entry in three chunks [b0, b1), [b1, b2), [b2, b3): per chunk one launch that solves and
// scores its samples, and between chunks one that replays the sequential loop over them and draws the next chunk's samples.
// A chunk whose first sample lies beyond the (shrinking) budget is two early-exit launches.  The sample stream is replayed by
// ONE lane (cv::RNG is sequential: ~1.4 us per 7-point sample), so the first chunk is small - with the inlier ratios a
// matcher's output has, OpenCV's budget drops to 3 - 5 after the first all-inlier sample, and a 128-sample first chunk spent
// 180 us drawing samples the loop never looks at - and the rest are few and large (`mid`: 128 for F / H / E, 64 for PnP).
// The result does not depend on the bounds.
inline std::array<int, 4> ransac_chunk_bounds(int max_iters, int mid) {
    return {0, std::min(8, max_iters), std::min(mid, max_iters), max_iters};
}

}  // namespace sslam
