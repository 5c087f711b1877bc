// Host planner of vj_track / vj_track_layout that needs no device: the argument checks, the two vj_extract
// layouts of a call — the templates T and the search patches S, through vj_extract_host.cpp's planner —, the scratch layout, the
// slices and step 5 of the definition (the box of a match).  Compiled without HIP too: tests/track_asan_driver.cpp runs it under
// ASan + UBSan.
#pragma once
#include "vj_extract_host.hpp"
#include "vj_track_units.hpp"

#include <vector>

namespace vj {

struct TrackLayout {
    std::vector<vj_roi> tmpl_regions, search_regions;   // the rows as vj_extract regions: (src_frame, x, y, w, h), (dst_frame, x, y, w, h)
    ExtractLayout tmpl, search;      // tmpl.src[k] = (src_frame, x0, y0, w0, h0), search.src[k] = (dst_frame, X, Y, Wm, Hm)
    uint32_t t = 0, r = 0;
    uint64_t tmpl_off = 0;           // scratch: n * t * t bytes of templates (t * t is a multiple of 16) ...
    uint64_t search_off = 0;         // ... then n search patches at search.region_pitch = (t + 2 r)^2 rounded up to 16
    uint64_t scratch_bytes = 0;
};
// Checks the call and lays it out.  VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error naming the row or the field.
int track_layout(const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows, const vj_track_params* p, TrackLayout* out);

// The end of the slice that begins at row `first`: rows are taken in order while they name at most `max_frames` distinct frames
// (0: no bound), src and dst counted alike; at least one row.
size_t track_slice_end(const vj_track_row* rows, size_t n_rows, size_t first, size_t max_frames);

// Step 5: the box of row k's match in dst_frame, source pixels.
void track_result(const TrackLayout& lay, size_t k, const TrackMatchDev& m, vj_track_result* out);

}  // namespace vj
