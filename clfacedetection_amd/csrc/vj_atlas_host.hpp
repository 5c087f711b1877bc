// Host planner of the mixed-size entry points (vj_detect_mixed, vj_detect_opencv_mixed, vj_pack_frames) that needs
// no device: the frame checks, which frames get a batched call of their own, and the atlases that hold the others.  Compiled without
// HIP too: tests/atlas_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_atlas_units.hpp"

namespace vj {

constexpr uint64_t ATLAS_DEFAULT_PX = 1ull << 24;      // vj_mixed_opts::atlas_px == 0: the budget of the level canvases (CV_ROI_CANVAS_PX)
// vj_mixed_opts::own_call_px == 0.  Measured (tests/measure_mixed.py sweep, profiles/mixed_sizes_sweep.json): a batched
// call of its own costs a group about 0.37 ms and then 0.067 ms per 320 x 240 frame (0.45 ms per 1280 x 720 frame), a place on an
// atlas that exists anyway 0.115 ms (0.97 ms) per frame: the two meet near 8 frames of 320 x 240 (0.59 M pixels) and at one frame of
// 1280 x 720 (0.92 M pixels).  The lower of the two, rounded to a power of two.
constexpr uint64_t ATLAS_DEFAULT_OWN_CALL_PX = 1ull << 19;

// The atlas dimensions come from a short ladder, so that the plans keyed by them (the OpenCV profile's region plan by the frame
// width, the clod plans by width and height) repeat from call to call: the next multiple of q = max(32, 2^floor(log2 v) / 4) at or
// above v — four steps per octave, at most a quarter more than asked for per axis.
uint32_t atlas_ladder(uint32_t v);

struct AtlasSize { int w, h, ch; };
// What every frame of a mixed call must be: non-null data, w > 0, h > 0, 1 / 3 / 4 channels, stride >= w * channels; VJ_ERR_ARG
// names the first frame that is not.  *sizes: one entry per frame.
int atlas_check_frames(const vj_image* frames, int n_frames, std::vector<AtlasSize>* sizes);

// Frame indices by (w, h, channels), groups in that order, each in frame order
std::vector<std::vector<int>> atlas_size_groups(const std::vector<AtlasSize>& sizes, const std::vector<int>& idx);

// Routing by group: a group of frames of one (w, h, channels) with at least own_call_px pixels in total (or every group: all_own,
// the flags whose result needs the image alone) gets a batched call of its own; the others are packed, in frame order.
struct AtlasRoute {
    std::vector<std::vector<int>> own;
    std::vector<int> packed;
};
AtlasRoute atlas_route(const std::vector<AtlasSize>& sizes, uint64_t own_call_px, bool all_own);

struct AtlasSlot {
    int frame;                 // index in the call's frame list
    uint32_t ox, oy, w, h;     // the slot is align4(w) x h at (ox, oy); ox a multiple of 4
    uint32_t unit_first;       // its pack units: [unit_first, unit_first + ceil(w / ATLAS_BLOCK_W) * ceil(h / ATLAS_BLOCK_H))
};
// An atlas: frames order[first .. first + n_frames) shelf-packed, tallest first, first shelf with room, no gaps but the rounding of
// slot widths to 4 columns (what no frame covers is never cleared: it cancels in every four-corner difference, tilted rectangles
// included).
struct AtlasPlan {
    size_t n_frames = 0;
    bool oversized = false;    // the first frame's slot does not fit an EMPTY atlas: n_frames = 1, nothing planned — the caller
                               // sends it through a call of its own
    uint32_t w = 0, h = 0, pitch = 0;   // both on the ladder; pitch = w
    std::vector<AtlasSlot> slots;       // in the order taken
    uint32_t n_units = 0;
};
// Plans the next atlas from order[first] on: as many frames, at most max_frames (<= 0: no cap), as their slots stay within budget_px
// pixels in total.  The atlas itself — shelves and ladder rounding included — comes out larger than its slots, typically by a
// third, at worst about three times; what bounds it are the 32-bit offsets of a frame of its size, (w + 1) * (h + 3) < 2^30 and
// h < 65535: an atlas beyond them takes fewer frames.
int atlas_plan(const std::vector<AtlasSize>& sizes, const std::vector<int>& order, size_t first, uint64_t budget_px, int max_frames,
               AtlasPlan* out);

}  // namespace vj
