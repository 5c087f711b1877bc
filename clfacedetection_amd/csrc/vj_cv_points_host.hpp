// Host side of the window-list calls that needs no device: the argument checks both profiles share and the
// grouping of the caller's windows by (sub-batch, scale slot) into units; for vj_run_windows_opencv, what a scale gives whatever the
// image and the scatter of the verdicts back into the caller's order (vj_run_windows: vj_points_host.hpp).  Compiled without HIP too: tests/run_windows_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_cv_points_units.hpp"
#include "vj_cv_roi_host.hpp"

#include <cmath>
#include <limits>

namespace vj {

constexpr uint32_t CV_POINTS_MAX = 1u << 27;   // windows per call

// What both window-list entry points refuse without a device, in the order include/vj.h states it (`fn`: the entry point's name,
// for the messages): the cascade and start_stage (negative; non-zero on a stage tree) ...
int points_check_cascade(const char* fn, const vj_cascade* c, int start_stage);
// ... then — n_windows == 0 is VJ_OK before any of these — the pointers, the window count, the frames (cv_frames_uniform), the
// scales (finite and > 0, then scale_ok(k): what else the profile refuses a scale for), the windows' frame and scale indices.
// *W, *H, *CH: the frames' geometry (set when n_windows != 0).  cv_points_check is the two with no refusal of its own.
template <class Scale, class ScaleOk>
int points_check_lists(const char* fn, const vj_image* frames, int n_frames, const Scale* scales, int n_scales, const vj_window* windows,
                       uint32_t n_windows, const void* out, int* W, int* H, int* CH, ScaleOk scale_ok) {
    if (n_windows == 0) return VJ_OK;
    if (!windows || !out || !scales || !frames || n_frames <= 0 || n_scales <= 0) {
        set_error("%s: %u windows need frames, scales and a result array", fn, n_windows);
        return VJ_ERR_ARG;
    }
    if (n_windows > CV_POINTS_MAX) {
        set_error("%s: %u windows; at most %u per call", fn, n_windows, CV_POINTS_MAX);
        return VJ_ERR_LIMIT;
    }
    if (!cv_frames_uniform(frames, n_frames, W, H, CH)) {
        set_error("%s: the frames must be of one size and channel count (1, 3 or 4), with data", fn);
        return VJ_ERR_ARG;
    }
    for (int k = 0; k < n_scales; ++k) {
        if (!(std::isfinite(scales[k]) && scales[k] > 0)) {   // cvSetImagesForHaarClassifierCascade: scale <= 0 is refused (tempcv.cpp:568)
            set_error("%s: scale %d is %.*g; a scale is finite and > 0", fn, k, std::numeric_limits<Scale>::max_digits10, (double)scales[k]);
            return VJ_ERR_ARG;
        }
        const int rc = scale_ok(k);
        if (rc) return rc;
    }
    for (uint32_t i = 0; i < n_windows; ++i) {
        const vj_window& w = windows[i];
        if (w.frame < 0 || w.frame >= n_frames) {
            set_error("%s: window %u names frame %d of %d", fn, i, w.frame, n_frames);
            return VJ_ERR_ARG;
        }
        if (w.scale < 0 || w.scale >= n_scales) {
            set_error("%s: window %u names scale %d of %d", fn, i, w.scale, n_scales);
            return VJ_ERR_ARG;
        }
    }
    return VJ_OK;
}
int cv_points_check(const vj_cascade* c, const vj_image* frames, int n_frames, const double* scales, int n_scales,
                    const vj_window* windows, uint32_t n_windows, int start_stage, const vj_window_result* out, int* W, int* H, int* CH);

// real_window_size and equRect of a scale (tempcv.cpp:608-618): cvRound(orig * scale), clamped to CV_POINT_WIN_MAX so that
// no scale overflows an int; equRect = (cvRound(scale), cvRound(scale), cvRound((orig - 2) * scale) each way), weight_scale = 1 / area
struct CvPointScale {
    int win_w, win_h;
    int ex, ew, eh;
    double weight_scale;
    bool fits;             // the window fits the frame: some position passes the border rule, so the slot needs a table
};
CvPointScale cv_point_scale(int orig_w, int orig_h, double scale, int W, int H);

// The caller's window indices ordered by (sub-batch = frame / max_frames, scale slot), stable within a slot (std::stable_sort on the indices);
// sub_first[b] .. sub_first[b + 1]: the windows of sub-batch b.
void cv_points_order(const vj_window* windows, uint32_t n_windows, int n_frames, int max_frames, std::vector<uint32_t>* order,
                     std::vector<size_t>* sub_first);

// One sub-batch's device lists: point k stands for windows[order[k]] (frame relative to f0, index k), cut into units of up to 64
// windows of one slot.
void cv_points_build(const vj_window* windows, const uint32_t* order, size_t m, int f0, std::vector<CvPointDev>* points,
                     std::vector<CvPointUnit>* units);

// The pass's verdicts (entry k: windows[order[k]]) into the caller's order
void cv_points_scatter(const CvPointResult* res, const uint32_t* order, size_t m, vj_window_result* out);

}  // namespace vj
