// Records the preprocessing kernels (vj_prep.hip) share with the host code that builds them (vj_prep_host.cpp, which
// is compiled without HIP for the sanitizer runs): plain PODs, nothing else.
#pragma once
#include <stdint.h>

#include "vj_cv_roi_units.hpp"

namespace vj {

// One frame of a vj_preprocess call: where its pixels lie (a device address: the caller's device-resident frame, or the frame's
// place in the uploaded block of the call's host frames), where its gray, resized image goes in the caller's buffer and which taps
// resize it.  dst_off is a multiple of 256 and pitch a multiple of 4: a lane stores four pixels as one aligned dword.
struct PrepFrameDev {
    const uint8_t* src;
    uint64_t dst_off;       // byte offset of the output image in the destination buffer
    uint32_t stride;        // bytes per source row
    uint32_t channels;      // 1, 3 (BGR) or 4 (BGRA)
    uint32_t sw, sh;        // source size
    uint32_t dw, dh;        // destination size
    uint32_t pitch;         // bytes per destination row: align4(dw)
    uint32_t xtab, ytab;    // first PyrTap of its columns / rows in PrepArgs::taps (runs padded to 4 taps with their last one)
    uint32_t mode;          // PREP_BILINEAR, PREP_AREA (the source is exactly 2 dw x 2 dh) or PREP_COPY (dw x dh is the source's size)
    uint32_t unit_first;    // first work unit (a PREP_BLOCK_W x PREP_BLOCK_H block of the destination)
    uint32_t hist_slot;     // its histogram and table: PrepArgs::hist + 256 * hist_slot
};
static_assert(sizeof(PrepFrameDev) == 64, "PrepFrameDev is 64 bytes");
enum : uint32_t { PREP_BILINEAR = 0, PREP_AREA = 1, PREP_COPY = 2 };

// Pixels per workgroup: 4 waves, each one row of 64 lanes x 4 pixels at a time, rows k, k + 4, ... of the block.  32 rows keep the
// clearing and merging of a workgroup's LDS histograms (16 KiB) at one pass per 8192 pixels — a 960 x 540 output is 68 workgroups —
// while a frame narrower than 256 pixels wastes only the lanes to its right.
constexpr uint32_t PREP_BLOCK_W = 256, PREP_BLOCK_H = 32;
inline uint64_t prep_units(uint32_t dw, uint32_t dh) {
    return (uint64_t)((dw + PREP_BLOCK_W - 1u) / PREP_BLOCK_W) * (uint64_t)((dh + PREP_BLOCK_H - 1u) / PREP_BLOCK_H);
}

struct PrepArgs {
    const PrepFrameDev* frames;
    uint32_t n_frames;
    uint32_t n_units;
    const PyrTap* taps;
    uint8_t* dst;           // the caller's buffer; every frame's image lies inside [dst, dst + dst_bytes)
    uint64_t dst_bytes;
    uint32_t* hist;         // [n_frames][256], cleared by the caller (null: nothing is counted)
    const uint8_t* lut;     // [n_frames][256] (prep_apply)
};
int launch_prep_resize(const PrepArgs& a, bool hist, void* stream);
int launch_prep_hist(const PrepArgs& a, void* stream);    // -DPREP_UNFUSED_HIST: the histograms from the written images
int launch_prep_apply(const PrepArgs& a, void* stream);

}  // namespace vj
