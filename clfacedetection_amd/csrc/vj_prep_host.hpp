// Host planner of vj_preprocess / vj_preprocess_layout that needs no device: the argument checks, every frame's
// destination size and place in the caller's buffer, and the frame records and taps of a slice of the call.  Compiled without HIP
// too: tests/prep_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_atlas_units.hpp"
#include "vj_prep_units.hpp"

#include <map>
#include <tuple>
#include <vector>

namespace vj {

struct PrepSlot {
    uint32_t sw, sh, ch;    // the source frame
    uint32_t dw, dh, pitch; // its output image: pitch = align4(dw)
    uint64_t off;           // its place in the destination buffer: a multiple of 256
};
struct PrepLayout {
    std::vector<PrepSlot> slots;
    uint64_t bytes = 0;     // the end of the last image
    bool equalize = false;
};
// Checks `frames` (vj_detect_mixed's rules) and `p`, sizes every output image and lays them out.  VJ_ERR_ARG / VJ_ERR_LIMIT with
// vj_last_error naming the frame or the field.
int prep_layout(const vj_image* frames, int n_frames, const vj_prep* p, PrepLayout* out);

// A device-resident source that overlaps [dst, dst + bytes): VJ_ERR_ARG naming the frame
int prep_check_overlap(const vj_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes);

// The records of frames [first, first + n) and the taps they share: one run per distinct (source length, destination length, rows,
// area), padded to a multiple of 4 taps with copies of its last one (a lane loads the four taps of its pixels as two 16-byte words).
// src / stride are the frame's own; the caller replaces those of the host frames it stages.  eq: the records equalize_lut reads
// (w, h = the destination size).
struct PrepSlice {
    std::vector<PrepFrameDev> recs;
    std::vector<AtlasFrameDev> eq;
    std::vector<PyrTap> taps;
    uint32_t n_units = 0;
};
int prep_plan_slice(const vj_image* frames, const PrepLayout& lay, size_t first, size_t n, PrepSlice* out);

}  // namespace vj
