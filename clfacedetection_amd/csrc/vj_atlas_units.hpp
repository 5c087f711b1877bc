// Records the atlas pack kernel (vj_atlas.hip) and the equalization kernels (vj_equalize.hip, §4.15) share with the
// host code that builds them (vj_atlas_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs, nothing else.
#pragma once
#include <stdint.h>

namespace vj {

// One frame of an atlas: where its pixels lie (a device address: the caller's device-resident frame, or the frame's place in the
// uploaded block of the atlas's host frames) and where its gray image goes.  ox is a multiple of 4 and the slot align4(w) x h
// lies inside the atlas: the kernel stores four pixels as one dword.
struct AtlasFrameDev {
    const uint8_t* src;
    uint32_t stride;        // bytes per source row
    uint32_t channels;      // 1, 3 (BGR) or 4 (BGRA)
    uint32_t w, h;
    uint32_t ox, oy;        // the slot's origin in the atlas
    uint32_t unit_first;    // first work unit (an ATLAS_BLOCK_W x ATLAS_BLOCK_H block of the frame's pixels)
    uint32_t hist_first;    // first histogram unit (EQ_HIST_ROWS whole rows of the frame); 0 where nothing is equalized
};
static_assert(sizeof(AtlasFrameDev) == 40, "AtlasFrameDev is 40 bytes");
// Pixels per workgroup: 4 waves, each one row of 64 lanes x 4 pixels.  A wave reads 256 consecutive gray bytes (768 / 1024 of a BGR /
// BGRA row) and stores 256: whole cache lines in both directions; four rows per workgroup keep the 97 .. 180-row frames the entry
// points are for at 25 .. 45 workgroups each — the launch fills the device from a dozen frames on — while a frame narrower than
// 256 pixels wastes only the lanes to its right, never a whole wave.
constexpr uint32_t ATLAS_BLOCK_W = 256, ATLAS_BLOCK_H = 4;

struct AtlasPackArgs {
    const AtlasFrameDev* frames;
    uint32_t n_frames;
    uint32_t n_units;
    uint8_t* atlas;
    uint32_t atlas_pitch;   // bytes per atlas row: a multiple of 4, >= atlas_w
    uint32_t atlas_w, atlas_h;
    const uint8_t* lut;     // VJ_FLAG_EQUALIZE_HIST: 256 bytes per frame, applied before the store (null: the gray image as it is)
};
int launch_atlas_pack(const AtlasPackArgs& a, void* stream);

// VJ_FLAG_EQUALIZE_HIST / vj_equalize_hist (vj_equalize.hip).  A histogram workgroup counts EQ_HIST_ROWS whole rows
// of one frame, a wave every fourth of them: a 1920 x 1080 frame is 34 workgroups that each merge 256 bins once (one global atomic
// per 240 pixels at worst), a 200 x 150 frame of an atlas five.
constexpr uint32_t EQ_HIST_ROWS = 32;
inline uint32_t eq_hist_units(uint32_t h) { return (h + EQ_HIST_ROWS - 1u) / EQ_HIST_ROWS; }

struct EqualizeArgs {
    const AtlasFrameDev* frames;   // ox, oy are not read: frame i goes to dst + i * dst_frame_bytes
    uint32_t n_frames;
    uint32_t n_units;        // pack units of all frames (equalize_apply's grid)
    uint32_t n_hist_units;   // histogram units of all frames (equalize_hist's grid)
    uint32_t* hist;          // [n_frames][256], cleared by the caller
    uint8_t* lut;            // [n_frames][256]
    uint8_t* dst;            // gray batch: rows of dst_pitch bytes (a multiple of 4, >= align4(w) of every frame), dst_h rows per frame
    uint32_t dst_pitch, dst_h;
    uint64_t dst_frame_bytes;
};
int launch_equalize_hist(const EqualizeArgs& a, void* stream);
int launch_equalize_lut(const EqualizeArgs& a, void* stream);
int launch_equalize_apply(const EqualizeArgs& a, void* stream);

}  // namespace vj
