// Records the window-list pass of the clod profile (vj_run_windows; vj_points.hip) shares with the host code that
// builds and reads them (vj_points_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs.  The windows and
// their units are the OpenCV profile's (CvPointDev, CvPointUnit: vj_cv_points_units.hpp) — the grouping is profile-agnostic.
#pragma once
#include <stdint.h>
#include "vj_cv_points_units.hpp"

namespace vj {

struct StageDev;
struct NodeRec;

// A verdict: vj_clod_window_result's layout
struct ClodPointResult {
    int32_t result;
    float   variance, stage_sum;
    int32_t reserved;
};
static_assert(sizeof(ClodPointResult) == 16, "ClodPointResult is 16 bytes");
constexpr int32_t CLOD_POINT_OUTSIDE = INT32_MIN;   // == VJ_WINDOW_OUTSIDE

// One scale slot of a call: what setupScale (clod.cpp:371-415) derives from the scale, and its node table
struct ClodPointScaleDev {
    const NodeRec* table;        // the slot's records, built with the frame's stride (null: the window exceeds the frame — never read)
    float    area;               // (float)scaled_window_area = equ_w * equ_h
    uint32_t win_w, win_h;       // scaled_window_size = round(win * scale), at most CV_POINT_WIN_MAX
    uint32_t e_lt, e_dw, e_dh;   // equ_rect: left-top, width, height * stride — ELEMENT offsets from the window origin
};
static_assert(sizeof(ClodPointScaleDev) == 32, "ClodPointScaleDev is 32 bytes");

struct ClodPointArgs {
    const uint32_t* sum;
    const uint64_t* sqsum;
    const ClodPointScaleDev* scales;
    const StageDev* stages;      // as CascadeArgs::stages
    const CvPointDev* points;
    const CvPointUnit* units;    // ordered by scale slot
    ClodPointResult* out;        // n_points entries
    uint32_t n_units, n_points;
    uint32_t n_frames, frame_elems, stride, width, height;
    uint32_t n_stages, n_order;  // n_order: stage trees, as CascadeArgs
    uint32_t start_stage;        // linear cascades (<= n_stages); 0 for stage trees
    uint32_t signed_mean;        // VJ_FLAG_SIGNED_MEAN
    uint32_t total_waves;
};
constexpr int CLOD_POINT_WAVES = 4;   // waves per workgroup
int launch_clod_points_pass(const ClodPointArgs& a, bool trees, bool stage_tree, int n_blocks, void* stream);

}  // namespace vj
