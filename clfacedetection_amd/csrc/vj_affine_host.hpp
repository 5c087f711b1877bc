// Host planner of vj_extract_affine / vj_extract_affine_layout that needs no device: the argument checks and the
// limits, the layout, the two matrix helpers, and the region records and work units of a slice of the call.  Compiled without HIP
// too: tests/affine_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_affine_units.hpp"

#include <vector>

namespace vj {

struct AffineLayout {
    uint32_t out_w = 0, out_h = 0;
    uint32_t C = 1;                // channels of the output
    bool gray = false, planar = false;
    uint32_t rows = 0, row_bytes = 0;   // of one region's output (vj_extract_units.hpp)
    uint64_t region_bytes = 0;     // rows * row_bytes
    uint64_t bytes = 0;            // n * region_bytes
};
// Checks `frames` (vj_detect_mixed's rules), `affines` and `p`.  VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error naming the row and the
// field.
int affine_layout(const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p, AffineLayout* out);

// The end of the slice that begins at affine `first`: affines are taken in order while they name at most `max_frames` distinct
// frames (0: no bound); at least one.
size_t affine_slice_end(const vj_affine* affines, size_t n, size_t first, size_t max_frames);

// The records of affines [first, first + n) and the distinct frames they name, in the order of their first use.  src / stride are
// the frame's own; the caller replaces those of the host frames it stages.
struct AffineSlice {
    std::vector<AffineRegionDev> recs;
    std::vector<int> frames;
    uint32_t n_units = 0;
};
int affine_plan_slice(const vj_image* frames, const vj_affine* affines, const AffineLayout& lay, size_t first, size_t n, AffineSlice* out);

// The fixed-point terms of §4.19, as the kernel computes them (the sanitizer driver decodes the units with these).
int32_t affine_rne(double v);                                                   // cvRound: round half to even
inline int32_t affine_col_term(double m, uint32_t x) { return affine_rne((m * (double)x) * 1024.0); }
inline int32_t affine_row_term(double m, double c, uint32_t y) { return affine_rne((m * (double)y + c) * 1024.0) + 16; }

}  // namespace vj
