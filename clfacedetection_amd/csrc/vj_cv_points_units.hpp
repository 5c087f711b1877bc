// Records the window-list pass of the OpenCV profile (vj_run_windows_opencv; vj_cv_points.hip) shares with the host
// code that builds and reads them (vj_cv_points_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs.
#pragma once
#include <stdint.h>

namespace vj {

struct StageDev;
struct CvNodeRec;

// One window of the caller's list as the pass sees it: the caller's coordinates as they came (any int32: the border rule is
// evaluated on the device, in 64 bits), the frame within the sub-batch on the device, and where its verdict goes.
struct CvPointDev {
    int32_t  x, y;
    uint32_t frame;
    uint32_t index;          // entry of CvPointArgs::out
};
static_assert(sizeof(CvPointDev) == 16, "CvPointDev is 16 bytes");
// One unit of work: points [first, first + count) of the list, count <= 64, all of scale slot `slot` — one wave, lane = window.
struct CvPointUnit { uint32_t first, count, slot, pad; };
constexpr uint32_t CV_POINT_UNIT = 64;
// A verdict: vj_window_result's layout
struct CvPointResult {
    int32_t result, reserved;
    double  stage_sum;
};
static_assert(sizeof(CvPointResult) == 16, "CvPointResult is 16 bytes");

// One scale slot of a call: what cvSetImagesForHaarClassifierCascade (tempcv.cpp:549-632) derives from the scale, and its node table
struct CvPointScaleDev {
    double   inv_area;           // weight_scale = 1 / (equ_w * equ_h)
    const CvNodeRec* table;      // the slot's records, built with the frame's stride (null: the window exceeds the frame — never read)
    uint32_t win_w, win_h;       // real_window_size = cvRound(orig * scale), at most CV_POINT_WIN_MAX
    uint32_t q0, q1, q2, q3;     // the four corners of equRect, element offsets from the window origin
    uint32_t pad[2];
};
static_assert(sizeof(CvPointScaleDev) == 48, "CvPointScaleDev is 48 bytes");
constexpr uint32_t CV_POINT_WIN_MAX = 1u << 20;   // a larger window is recorded as this: above every frame size, so -1 everywhere

struct CvPointArgs {
    const uint32_t* sum;
    const uint32_t* tilted;      // null: no tilted features
    const uint64_t* sqsum;
    const CvPointScaleDev* scales;
    const StageDev* stages;      // as CvArgs::stages
    const CvPointDev* points;
    const CvPointUnit* units;    // ordered by scale slot
    CvPointResult* out;          // n_points entries
    uint32_t n_units, n_points;
    uint32_t n_frames, frame_elems, stride, width, height;
    uint32_t n_stages, n_order;  // n_order: stage trees, as CvArgs
    uint32_t start_stage;        // linear cascades (<= n_stages); 0 for stage trees
    uint32_t tail_max, tree2;    // as CvArgs
    uint32_t total_waves;
};
int launch_cv_points_pass(const CvPointArgs& a, bool trees, bool stage_tree, int n_blocks, void* stream);

}  // namespace vj
