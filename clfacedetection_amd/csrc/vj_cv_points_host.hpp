// Host side of vj_run_windows_opencv that needs no device: argument checks, what a scale gives whatever the image,
// the grouping of the caller's windows by (sub-batch, scale slot) and their units, and the scatter of the verdicts back into the
// caller's order.  Compiled without HIP too: tests/run_windows_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_cv_points_units.hpp"
#include "vj_cv_roi_host.hpp"

namespace vj {

constexpr uint32_t CV_POINTS_MAX = 1u << 27;   // windows per call

// Everything of the call that can be refused without a device, in the order the header states it: null pointers, start_stage
// (negative; non-zero on a stage tree), then — n_windows == 0 is VJ_OK before any of these — the frames (cv_frames_uniform), the
// scales (finite, > 0), the windows' frame and scale indices.  *W, *H, *CH: the frames' geometry (set when n_windows != 0).
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
