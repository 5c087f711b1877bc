// Host planner of vj_extract_yuv / vj_extract_affine_yuv and their _layout twins that needs no device.  Nothing is
// planned anew: the frames are checked by vj_yuv_to_bgr's planner, the regions, affines and parameters by vj_extract's and
// vj_extract_affine's on the Y planes as gray frames — the channel count then becomes the one the decode gives —, and the records,
// taps and work units of a slice are theirs with the chroma planes added.  Compiled without HIP too:
// tests/extract_yuv_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_extract_yuv_units.hpp"
#include "vj_extract_host.hpp"
#include "vj_affine_host.hpp"
#include "vj_yuv_host.hpp"

#include <vector>

namespace vj {

// What the decode contributes to a checked call: the Y planes as gray frames (what the two planners see) and the BGR side
struct YuvSource {
    std::vector<vj_image> luma;
    uint32_t channels = 3;         // of the decoded taps: 3 or 4
    bool swap_rb = false;
};
struct ExtractYuvLayout {
    ExtractLayout lay;             // vj_extract's, with C, the rows and the byte counts of the decoded channels
    YuvSource src;
};
struct AffineYuvLayout {
    AffineLayout lay;
    YuvSource src;
};
// VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error naming the frame, the row or the field
int extract_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                       const vj_yuv_params* yp, ExtractYuvLayout* out);
int affine_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                      const vj_yuv_params* yp, AffineYuvLayout* out);

// The records of regions / affines [first, first + n) (extract_plan_slice / affine_plan_slice with the planes of their frames), the
// taps and the distinct frames they name in the order of their first use.  The plane pointers and strides are the frame's own; the
// caller replaces those of the host frames it stages.
struct ExtractYuvSlice {
    ExtractSlice luma;
    std::vector<ExtractYuvRegionDev> recs;
};
struct AffineYuvSlice {
    AffineSlice luma;
    std::vector<AffineYuvRegionDev> recs;
};
int extract_yuv_plan_slice(const vj_yuv_image* frames, const vj_roi* regions, const ExtractYuvLayout& lay, size_t first, size_t n, ExtractYuvSlice* out);
int affine_yuv_plan_slice(const vj_yuv_image* frames, const vj_affine* affines, const AffineYuvLayout& lay, size_t first, size_t n, AffineYuvSlice* out);

}  // namespace vj
