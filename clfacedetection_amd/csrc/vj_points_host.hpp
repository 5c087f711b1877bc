// Host side of vj_run_windows that needs no device: argument checks, what a scale gives whatever the image
// (setupScale, clod.cpp:371-415, without its loop-side rejections), and the scatter of the verdicts back into the caller's order.
// Ordering the windows by (sub-batch, scale slot) and cutting them into units is the OpenCV profile's: cv_points_order /
// cv_points_build (vj_cv_points_host.hpp).  Compiled without HIP too: tests/clod_windows_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_points_units.hpp"
#include "vj_cv_points_host.hpp"

namespace vj {

// scaled_window_size, equ_rect and scaled_window_area of a scale (clod.cpp:387-388, :404-408): (cl_uint)round(int * f32) — the f32
// product rounded half away from zero —, every rounded value clamped to CV_POINT_WIN_MAX so that no scale overflows an int
struct ClodPointScale {
    int win_w, win_h;
    int ex, ew, eh;        // equ_rect = (ex, ex, ew, eh)
    uint32_t area;         // ew * eh (exact where the window fits a frame the profile accepts; saturated otherwise)
    bool fits;             // the window fits the frame: some position is inside, so the slot needs a table
};
// VJ_ERR_ARG when win_w, win_h or the area is 0 (the reference would divide by zero)
int clod_point_scale(int orig_w, int orig_h, float scale, int W, int H, ClodPointScale* out);

// Everything of the call that can be refused without a device, in the order the header states it: points_check_cascade, the flags
// (a bit other than VJ_FLAG_SIGNED_MEAN / VJ_FLAG_TILTED_AS_UPRIGHT: VJ_ERR_ARG; tilted features without the latter:
// VJ_ERR_UNSUPPORTED), then points_check_lists, whose scales pass clod_point_scale too (vj_cv_points_host.hpp).
// *W, *H, *CH: the frames' geometry (set when n_windows != 0).
int clod_points_check(const vj_cascade* c, const vj_image* frames, int n_frames, const float* scales, int n_scales,
                      const vj_window* windows, uint32_t n_windows, int start_stage, uint32_t flags, const vj_clod_window_result* out,
                      int* W, int* H, int* CH);

// The pass's verdicts (entry k: windows[order[k]]) into the caller's order
void clod_points_scatter(const ClodPointResult* res, const uint32_t* order, size_t m, vj_clod_window_result* out);

}  // namespace vj
