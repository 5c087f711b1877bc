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
    const char* fn = "vj_run_windows";
    const int rc = points_check_cascade(fn, c, start_stage);
    if (rc) return rc;
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
    return points_check_lists(fn, frames, n_frames, scales, n_scales, windows, n_windows, out, W, H, CH, [&](int k) {
        ClodPointScale sc;
        return clod_point_scale(c->win_w, c->win_h, scales[k], *W, *H, &sc);
    });
}

void clod_points_scatter(const ClodPointResult* res, const uint32_t* order, size_t m, vj_clod_window_result* out) {
    for (size_t k = 0; k < m; ++k) out[order[k]] = vj_clod_window_result{res[k].result, res[k].variance, res[k].stage_sum, 0};
}

}  // namespace vj
