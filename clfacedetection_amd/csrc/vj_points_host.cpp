// Host side of vj_run_windows that needs no device: see vj_points_host.hpp.  Compiled with -ffp-contract=off.
#include "vj_points_host.hpp"

#include <algorithm>
#include <cmath>

namespace vj {

namespace {
// (cl_uint)round(v) of a non-negative f32 product (clod.cpp:387-388, :404-407): half away from zero; clamped before the conversion
int round_clamped(float v) { return v < (float)CV_POINT_WIN_MAX ? (int)std::round((double)v) : (int)CV_POINT_WIN_MAX; }
}  // namespace

int clod_point_scale(int orig_w, int orig_h, float scale, int W, int H, ClodPointScale* out) {
    ClodPointScale s;
    s.win_w = round_clamped((float)orig_w * scale);
    s.win_h = round_clamped((float)orig_h * scale);
    s.ex = round_clamped(scale);
    s.ew = round_clamped((float)(orig_w - 2) * scale);
    s.eh = round_clamped((float)(orig_h - 2) * scale);
    // ew <= win_w and eh <= win_h (rounding is monotone): a window that fits has ew * eh <= W * H, which a frame the profile
    // accepts keeps below 2^32
    const uint64_t area = (uint64_t)s.ew * (uint64_t)s.eh;
    s.area = (uint32_t)std::min<uint64_t>(area, 0xffffffffull);
    s.fits = s.win_w <= W && s.win_h <= H;
    *out = s;
    if (s.win_w <= 0 || s.win_h <= 0 || area == 0) {
        set_error("vj_run_windows: scale %.9g gives a %d x %d window of area %llu (clod.cpp:430 would divide by zero)", (double)scale,
                  s.win_w, s.win_h, (unsigned long long)area);
        return VJ_ERR_ARG;
    }
    return VJ_OK;
}

int clod_points_check(const vj_cascade* c, const vj_image* frames, int n_frames, const float* scales, int n_scales,
                      const vj_window* windows, uint32_t n_windows, int start_stage, uint32_t flags, const vj_clod_window_result* out,
                      int* W, int* H, int* CH) {
    if (!c) {
        set_error("vj_run_windows: no cascade");
        return VJ_ERR_ARG;
    }
    if (start_stage < 0) {
        set_error("vj_run_windows: start_stage %d is negative", start_stage);
        return VJ_ERR_ARG;
    }
    bool is_tree = false;
    for (const auto& st : c->stages) is_tree |= st.next != -1;
    if (is_tree && start_stage != 0) {   // the walk of tempcv.cpp:834-861 starts at the root (assert, :837)
        set_error("vj_run_windows: a stage tree starts at stage 0 only (start_stage %d)", start_stage);
        return VJ_ERR_ARG;
    }
    if (flags & ~(uint32_t)(VJ_FLAG_SIGNED_MEAN | VJ_FLAG_TILTED_AS_UPRIGHT)) {
        set_error("vj_run_windows: flags 0x%x; a window list takes VJ_FLAG_SIGNED_MEAN and VJ_FLAG_TILTED_AS_UPRIGHT only", flags);
        return VJ_ERR_ARG;
    }
    if (!(flags & VJ_FLAG_TILTED_AS_UPRIGHT))
        for (const auto& nd : c->nodes)
            if (nd.tilted) {
                set_error("vj_run_windows: the cascade has tilted features, which the clod profile evaluates as upright rectangles "
                          "(clod.cpp:448-492) — pass VJ_FLAG_TILTED_AS_UPRIGHT for that, or use vj_run_windows_opencv");
                return VJ_ERR_UNSUPPORTED;
            }
    if (n_windows == 0) return VJ_OK;
    if (!windows || !out || !scales || !frames || n_frames <= 0 || n_scales <= 0) {
        set_error("vj_run_windows: %u windows need frames, scales and a result array", n_windows);
        return VJ_ERR_ARG;
    }
    if (n_windows > CV_POINTS_MAX) {
        set_error("vj_run_windows: %u windows; at most %u per call", n_windows, CV_POINTS_MAX);
        return VJ_ERR_LIMIT;
    }
    if (!cv_frames_uniform(frames, n_frames, W, H, CH)) {
        set_error("vj_run_windows: the frames must be of one size and channel count (1, 3 or 4), with data");
        return VJ_ERR_ARG;
    }
    for (int k = 0; k < n_scales; ++k) {
        if (!(std::isfinite(scales[k]) && scales[k] > 0.0f)) {
            set_error("vj_run_windows: scale %d is %.9g; a scale is finite and > 0", k, (double)scales[k]);
            return VJ_ERR_ARG;
        }
        ClodPointScale sc;
        const int rc = clod_point_scale(c->win_w, c->win_h, scales[k], *W, *H, &sc);
        if (rc) return rc;
    }
    for (uint32_t i = 0; i < n_windows; ++i) {
        const vj_window& w = windows[i];
        if (w.frame < 0 || w.frame >= n_frames) {
            set_error("vj_run_windows: window %u names frame %d of %d", i, w.frame, n_frames);
            return VJ_ERR_ARG;
        }
        if (w.scale < 0 || w.scale >= n_scales) {
            set_error("vj_run_windows: window %u names scale %d of %d", i, w.scale, n_scales);
            return VJ_ERR_ARG;
        }
    }
    return VJ_OK;
}

void clod_points_scatter(const ClodPointResult* res, const uint32_t* order, size_t m, vj_clod_window_result* out) {
    for (size_t k = 0; k < m; ++k) out[order[k]] = vj_clod_window_result{res[k].result, res[k].variance, res[k].stage_sum, 0};
}

}  // namespace vj
