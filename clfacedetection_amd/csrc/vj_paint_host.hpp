// Host planner of vj_paint / vj_paint_layout that needs no device: the argument checks, the mapping and clipping
// of every region, the slices of whole frames, and per slice the region records bucketed by frame, their overlap lists, their
// scratch offsets and the work units of each launch.  Compiled without HIP too: tests/paint_asan_driver.cpp runs it under
// ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_paint_units.hpp"

#include <vector>

namespace vj {

struct PaintLayout {
    uint32_t mode = 0;
    bool ellipse = false;
    uint32_t color = 0;              // color[c] in byte c
    std::vector<vj_roi> mapped;      // M per region
    std::vector<vj_roi> clipped;     // K per region as (frame, cx0, cy0, w, h); w = h = 0 when empty
    std::vector<int32_t> sizes;      // t, s or kk per region; 0 for FILL
    std::vector<int> touched;        // the frames that hold a region with a K, ascending
    uint64_t scratch_bytes = 0;      // of the call as one slice
};
// Checks `frames` (vj_detect_mixed's rules, and that no two overlap), `regions` and `p`; maps and clips every region.  VJ_ERR_ARG /
// VJ_ERR_LIMIT with vj_last_error naming the row or the field.
int paint_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p, PaintLayout* out);

// The end (an index into lay.touched) of the slice that begins at touched frame `first`: at most `max_frames` frames (0: all).
size_t paint_slice_end(const PaintLayout& lay, size_t first, size_t max_frames);

// The slice of touched frames [first, end): its records — ordered by frame, then by region index; `frame`, `stride` and `row0` are
// the frame's own, the caller replaces those of the host frames it stages —, the overlap lists, and per record the region of the
// call it stands for.
struct PaintSlice {
    std::vector<PaintRegionDev> recs;
    std::vector<uint32_t> overlaps;
    std::vector<int> region;         // index in the call, per record
    std::vector<int> frames;         // lay.touched[first .. end)
    uint32_t n_units = 0, n_pre_units = 0;
    uint64_t scratch_bytes = 0;
};
int paint_plan_slice(const vj_image* frames, const PaintLayout& lay, size_t first, size_t end, PaintSlice* out);

}  // namespace vj
