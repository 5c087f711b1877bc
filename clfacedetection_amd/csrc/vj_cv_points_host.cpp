// Host side of the window-list calls that needs no device: see vj_cv_points_host.hpp.
#include "vj_cv_points_host.hpp"

#include <algorithm>
#include <cmath>

namespace vj {

namespace {
// cvRound of a non-negative product, clamped before the conversion (an int cannot hold every orig * scale)
int round_clamped(double v) { return v < (double)CV_POINT_WIN_MAX ? cv_round(v) : (int)CV_POINT_WIN_MAX; }
}  // namespace

int points_check_cascade(const char* fn, const vj_cascade* c, int start_stage) {
    if (!c) {
        set_error("%s: no cascade", fn);
        return VJ_ERR_ARG;
    }
    if (start_stage < 0) {
        set_error("%s: start_stage %d is negative", fn, start_stage);
        return VJ_ERR_ARG;
    }
    bool is_tree = false;
    for (const auto& st : c->stages) is_tree |= st.next != -1;
    if (is_tree && start_stage != 0) {   // the walk of tempcv.cpp:834-861 starts at the root (assert, :837)
        set_error("%s: a stage tree starts at stage 0 only (start_stage %d)", fn, start_stage);
        return VJ_ERR_ARG;
    }
    return VJ_OK;
}

int cv_points_check(const vj_cascade* c, const vj_image* frames, int n_frames, const double* scales, int n_scales,
                    const vj_window* windows, uint32_t n_windows, int start_stage, const vj_window_result* out, int* W, int* H, int* CH) {
    const char* fn = "vj_run_windows_opencv";
    const int rc = points_check_cascade(fn, c, start_stage);
    if (rc) return rc;
    return points_check_lists(fn, frames, n_frames, scales, n_scales, windows, n_windows, out, W, H, CH, [](int) { return VJ_OK; });
}

CvPointScale cv_point_scale(int orig_w, int orig_h, double scale, int W, int H) {
    CvPointScale s;
    s.win_w = round_clamped(orig_w * scale);
    s.win_h = round_clamped(orig_h * scale);
    s.ex = round_clamped(scale);
    s.ew = round_clamped((orig_w - 2) * scale);
    s.eh = round_clamped((orig_h - 2) * scale);
    // x = 0 passes `x + win_w >= W + 1` iff win_w <= W; then ew * eh <= W * H, which a frame the profile accepts keeps below 2^30
    s.fits = s.win_w <= W && s.win_h <= H;
    s.weight_scale = s.fits ? 1. / (s.ew * s.eh) : 0.0;
    return s;
}

void cv_points_order(const vj_window* windows, uint32_t n_windows, int n_frames, int max_frames, std::vector<uint32_t>* order,
                     std::vector<size_t>* sub_first) {
    max_frames = std::max(max_frames, 1);
    const size_t n_sub = ((size_t)std::max(n_frames, 0) + (size_t)max_frames - 1) / (size_t)max_frames;
    order->resize(n_windows);
    for (uint32_t i = 0; i < n_windows; ++i) (*order)[i] = i;
    std::stable_sort(order->begin(), order->end(), [&](uint32_t a, uint32_t b) {
        const int sa = windows[a].frame / max_frames, sb = windows[b].frame / max_frames;
        return sa != sb ? sa < sb : windows[a].scale < windows[b].scale;
    });
    sub_first->assign(n_sub + 1, n_windows);
    size_t k = 0;
    for (size_t b = 0; b < n_sub; ++b) {
        while (k < n_windows && (size_t)(windows[(*order)[k]].frame / max_frames) < b) ++k;
        (*sub_first)[b] = k;
    }
}

void cv_points_build(const vj_window* windows, const uint32_t* order, size_t m, int f0, std::vector<CvPointDev>* points,
                     std::vector<CvPointUnit>* units) {
    points->resize(m);
    units->clear();
    for (size_t k = 0; k < m; ++k) {
        const vj_window& w = windows[order[k]];
        (*points)[k] = CvPointDev{w.x, w.y, (uint32_t)(w.frame - f0), (uint32_t)k};
        if (units->empty() || units->back().slot != (uint32_t)w.scale || units->back().count == CV_POINT_UNIT)
            units->push_back(CvPointUnit{(uint32_t)k, 0u, (uint32_t)w.scale, 0u});
        ++units->back().count;
    }
}

void cv_points_scatter(const CvPointResult* res, const uint32_t* order, size_t m, vj_window_result* out) {
    for (size_t k = 0; k < m; ++k) out[order[k]] = vj_window_result{res[k].result, 0, res[k].stage_sum};
}

}  // namespace vj
