// Sizing of the stage-tree tile path's survivor queue (vj_detect_opencv): pure arithmetic, no device.  Compiled
// without HIP too: tests/cv_tq_asan_driver.cpp checks it against brute force under ASan + UBSan.
#pragma once
#include "vj_device.hpp"

#include <algorithm>

namespace vj {

struct CvTqSizing {
    enum Kind { QUEUE, ROWS_ONLY, RESPLIT } kind;
    uint64_t n;   // QUEUE: entries of the queue; RESPLIT: frames per sub-batch from now on
};

// The queue for `nf` frames of a plan with `tile_windows` grid windows per frame on `n_tile_scales` tile scales: room for
// 1 / 2^shift of the tile windows (a few percent survive the prefix).  chain_pass: one sub-queue per scale, end to end
// (cv_tq_first / cv_tq_cap), else one flat queue.  want(n) = ((tile_windows * n) >> shift) + fixed.  forced_cap > 0 (tests): that
// many entries whatever the batch.  A queue of more than CV_TQ_MAX entries: fewer frames per sub-batch (a clamped queue would drop
// the entries of the later scales' sub-queues, which lie past its end), the rows when not even one frame fits.
inline CvTqSizing cv_tq_sizing(uint64_t tile_windows, uint32_t n_tile_scales, uint32_t nf, uint32_t shift, int forced_cap, bool chain_pass,
                               int max_frames) {
    if (forced_cap > 0) return {CvTqSizing::QUEUE, (uint64_t)forced_cap};
    const uint64_t fixed = chain_pass ? (uint64_t)n_tile_scales * 4096u + 4096u : 4096u;
    const uint64_t want = ((tile_windows * (uint64_t)nf) >> shift) + fixed;
    if (want <= CV_TQ_MAX) return {CvTqSizing::QUEUE, want};
    const uint64_t fit = tile_windows ? (((CV_TQ_MAX - fixed + 1u) << shift) - 1u) / tile_windows : 0u;
    if (fit == 0u) return {CvTqSizing::ROWS_ONLY, 0u};
    return {CvTqSizing::RESPLIT, std::min<uint64_t>(fit, (uint64_t)max_frames)};
}

}  // namespace vj
