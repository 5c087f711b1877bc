// Host planner of vj_yuv_to_bgr / vj_bgr_to_yuv and their _layout twins that needs no device: the argument checks,
// every frame's place in the caller's buffer, and the frame records of a slice of the call.  Compiled without HIP too:
// tests/yuv_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_yuv_units.hpp"

#include <vector>

namespace vj {

struct YuvSlot {
    uint32_t w, h;
    uint32_t ch;        // of the BGR side of this frame
    uint32_t pitch;     // decode: align4(w * ch), the BGR image's; encode: align4(w), the Y plane's
    uint64_t off;       // the output's place in the destination buffer: a multiple of 256
};
struct YuvLayout {
    std::vector<YuvSlot> slots;
    uint64_t bytes = 0;     // the end of the last output
    uint32_t layout = 0;    // encode: of every output frame
    uint32_t channels = 0;  // decode: of every output image
    bool swap_rb = false;
};
// Check the frames and `p`, lay the outputs out.  VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error naming the frame or the field.
int yuv_decode_layout(const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, YuvLayout* out);
int yuv_encode_layout(const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, YuvLayout* out);

// A device-resident source plane that overlaps [dst, dst + bytes): VJ_ERR_ARG naming the frame
int yuv_decode_check_overlap(const vj_yuv_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes);
int yuv_encode_check_overlap(const vj_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes);

// The records of frames [first, first + n).  The source pointers and strides are the frame's own; the caller replaces those of
// the host frames it stages.
struct YuvSlice {
    std::vector<YuvFrameDev> recs;
    uint32_t n_units = 0;
};
int yuv_decode_plan_slice(const vj_yuv_image* frames, const YuvLayout& lay, size_t first, size_t n, YuvSlice* out);
int yuv_encode_plan_slice(const vj_image* frames, const YuvLayout& lay, size_t first, size_t n, YuvSlice* out);

}  // namespace vj
