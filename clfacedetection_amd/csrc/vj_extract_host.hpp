// Host planner of vj_extract / vj_extract_layout that needs no device: the argument checks, the mapping of every
// region to source pixels, and the region records, taps and work units of a slice of the call.  Compiled without HIP too:
// tests/extract_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_extract_units.hpp"

#include <vector>

namespace vj {

struct ExtractLayout {
    std::vector<vj_roi> src;       // the mapped source regions, margin included; they may lie outside their frames
    uint32_t out_w = 0, out_h = 0;
    uint32_t C = 1;                // channels of the output
    bool gray = false, planar = false;
    uint32_t rows = 0, row_bytes = 0;   // of one region's output (vj_extract_units.hpp)
    uint64_t region_bytes = 0;     // rows * row_bytes
    uint64_t region_pitch = 0;     // bytes from one region's output to the next: region_bytes (vj_track pads it to a multiple of 16)
    uint64_t bytes = 0;            // n_regions * region_pitch
};
// Checks `frames` (vj_detect_mixed's rules), `regions` and `p`, and maps every region.  VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error
// naming the row or the field.
int extract_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p, ExtractLayout* out);

// One axis of step 1 of the mapping (origin o and length len times factor f, cvRound, then the margin) with its limits; `r` and
// `axis` go into the message.  vj_paint maps its regions with it too.
int extract_map_axis(int r, const char* axis, int o, int len, double f, double margin, int32_t* c0, int32_t* clen);

// The end of the slice that begins at region `first`: regions are taken in order while they name at most `max_frames` distinct
// frames (0: no bound); at least one region.
size_t extract_slice_end(const vj_roi* regions, size_t n_regions, size_t first, size_t max_frames);

// The records of regions [first, first + n), the taps they share — one run per distinct (crop length, output length, rows, area),
// relative to the crop's origin — and the distinct frames they name, in the order of their first use.  src / stride are the
// frame's own; the caller replaces those of the host frames it stages.
struct ExtractSlice {
    std::vector<ExtractRegionDev> recs;
    std::vector<PyrTap> taps;
    std::vector<int> frames;
    uint32_t n_units = 0;
};
int extract_plan_slice(const vj_image* frames, const vj_roi* regions, const ExtractLayout& lay, size_t first, size_t n, ExtractSlice* out);

// vj_extract.cpp (needs the device): regions [first, first + n) of a checked call as one copy into e->d_extract — records, taps and
// the host frames they name, staged in the lane's page-locked buffer — and one launch that writes into d_dst, all on e->stream.
// The caller waits for the stream before the next slice: that one reuses the staging buffer and the device block.  vj_track
// brings its two patch sets with it.
int enqueue_extract_slice(vj_env* e, const vj_image* frames, const vj_roi* regions, const ExtractLayout& lay, size_t first, size_t n,
                          uint8_t* d_dst, ExtractSlice* sl);

}  // namespace vj
