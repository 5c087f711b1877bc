// The planner of the OpenCV profile (vj_cv_plan.cpp): everything the kernels of a vj_detect_opencv call read, computed on the host
// from (cascade, frame size, parameters, batch-size class, settings).  No HIP type in it: the driver uploads the result
// (upload_cv_plan, vj_cv.cpp), and the sanitizer driver runs it without a device.
#pragma once
#include "vj_tunables.hpp"
#include "vj_cv_roi_host.hpp"   // cv_round

#include <vector>

namespace vj {

// What vj_detect_opencv derives from (cascade, frame size, parameters) and the host keeps: the fields of a plan that the planner
// computes (CvPlan, vj_env_internal.hpp, adds the device copies).
struct CvPlanHost {
    std::vector<CvScaleDev> scales;   // uploaded too; the host copy gives window sizes and scale indices of the result
    StageProgram prog;
    uint32_t n_stages = 0, n_order = 0, n_rows = 0;
    bool trees = false, is_tree = false, has_tilted = false, tree2 = false;
    // LDS-tile path (vj_cv_tile.hip): tiles of one frame per LDS class, the rows of the scales that stay on
    // cv_profile_pass, and the per-frame reject / visited bitmap with one recurrence domain per window row
    uint32_t n_tile_scales = 0, n_rows_rest = 0, bits_frame_words = 0, n_bit_segs = 0;
    int row_blocks = 1;               // workgroups per CU of cv_profile_pass next to the tiles
    uint32_t tree_prefix = 0;         // stage trees: stages of the linear prefix the tiles run (0: the cascade is linear)
    CvChainDev chains = {};           // stage trees: the part after the prefix as chains (n = 0: not of that shape)
    bool prune = false;               // CV_HAAR_DO_CANNY_PRUNING: every scale on cv_profile_pass<..., PRUNE>; a pruning rectangle per scale slot
    uint64_t tile_windows = 0;        // grid windows of the tile scales, per frame
    uint32_t class_first[3] = {0, 0, 0}, class_lds[2] = {0, 0};
    // CV_HAAR_SCALE_IMAGE (VJ_FLAG_CV_SCALE_IMAGE): `scales` are the evaluated LEVELS of the image pyramid, which share ONE node
    // table at factor 1 in the canvas's pitch; every level's place in the canvas, its taps (vj_pyramid.hip) and output factor
    // CV_HAAR_FIND_BIGGEST_OBJECT (VJ_FLAG_CV_FIND_BIGGEST): `scales` are the DESCENDING factors (repeated multiplication by the reciprocal),
    // slot = position in the walk, scale_idx = n_factors - 1 - slot; every scale on cv_biggest_pass (no tiles, no pruning, no pyramid)
    bool find_biggest = false;
    bool scale_image = false;
    bool roc = false;                 // vj_detect_opencv_roc: a scale-image plan whose levels all stay on the row kernel
    std::vector<double> level_factor;   // per scale slot: what a position of the level is multiplied by
    uint32_t canvas_w = 0, canvas_h = 0, canvas_pitch = 0, n_pyr_levels = 0, n_pyr_units = 0;
};

// What a plan holds only to be uploaded: the host keeps no copy after upload_cv_plan.
struct CvPlanTables {
    std::vector<CvNodeRec> table;            // per scale its frame-stride records (scale image: ONE table at factor 1), then the tile scales' tile-pitch copies
    std::vector<StageDev> stages;
    std::vector<UnitDev> rows, tiles, rows_rest, bit_segs;   // rows of every scale / tiles by LDS class / rows of the scales off the tiles / bitmap segments
    std::vector<CvPruneDev> prune;           // CV_HAAR_DO_CANNY_PRUNING: per scale slot
    std::vector<PyrLevelDev> pyr_levels;     // CV_HAAR_SCALE_IMAGE: the pyramid launch's level records
    std::vector<PyrTap> pyr_taps;            // ... per level its columns' taps, then its rows'
};

// maxSize of a vj_detect_opencv_roc call, already resolved: a zero member means the frame (tempcv.cpp:1230-1234)
struct CvMaxSize { int max_w, max_h; };

// icvCreateHidHaarClassifierCascade's flags (tempcv.cpp:410-470) and the tree shape the kernels have a fast form for
struct CvShape {
    bool trees = false, is_tree = false, has_tilted = false, tree2 = false;
    std::vector<uint8_t> two_rects;   // per stage: no node has a third rectangle (:452-457)
};
CvShape cv_shape_of(const vj_cascade* c);

// cvSetImagesForHaarClassifierCascade's node records for one factor (tempcv.cpp:632-768): cvRound-ed rectangles as byte offsets from the
// window origin in a `stride`-wide integral image, f32 weights with rect 0's derived from the others (:752-767; CV_ADJUST_WEIGHTS = 0).
// Nothing here depends on the image beyond its row step.  *max_reach: furthest element a feature touches, from the window origin.
int build_cv_node_recs(const vj_cascade* c, double scale, uint32_t stride, double weight_scale, CvNodeRec* recs, uint64_t* max_reach);

// The stage records of the profile: threshold - 0.0001f, resolved successors, sweep order, the arithmetic mode of a node sum
std::vector<StageDev> build_cv_stage_recs(const vj_cascade* c, const StageProgram& prog, const std::vector<uint32_t>& order,
                                          const std::vector<uint8_t>& two_rects, bool trees, bool is_tree);

// What every plan of the profile starts from: the stage program, its sweep order, the cascade's shape and its stage records.
// VJ_ERR_LIMIT for a cascade without stages or with more than VJ_MAX_STAGES, VJ_ERR_UNSUPPORTED for stage links that form a cycle.
struct CvCascadeHost {
    StageProgram prog;
    std::vector<uint32_t> order;
    CvShape shape;
    std::vector<StageDev> stages;
};
int cv_cascade_host(const vj_cascade* c, CvCascadeHost* out);

// equRect (tempcv.cpp:607-611) of the window at one factor: x = y = cvRound(factor), (orig - 2) * factor rounded each way, and
// weight_scale = 1 / area (the product in int).
struct CvEquRect {
    int ex, ew, eh;
    double inv_area;
};
inline CvEquRect cv_equ_rect(int win_w, int win_h, double factor) {
    const int ex = cv_round(factor), ew = cv_round((win_w - 2) * factor), eh = cv_round((win_h - 2) * factor);
    return CvEquRect{ex, ew, eh, 1. / (ew * eh)};
}
// ... into a scale record (CvScaleDev, CvPointScaleDev): inv_area and the four corners as element offsets in a `stride`-wide image
template <class Rec>
void cv_set_equ_rect(Rec* r, const CvEquRect& q, uint32_t stride) {
    r->inv_area = q.inv_area;
    r->q0 = (uint32_t)q.ex * stride + (uint32_t)q.ex;
    r->q1 = r->q0 + (uint32_t)q.ew;
    r->q2 = (uint32_t)(q.ex + q.eh) * stride + (uint32_t)q.ex;
    r->q3 = r->q2 + (uint32_t)q.ew;
}

// The level k at which `winSize > maxSize` ends the scale-image level loop (tempcv.cpp:1268-1286), -1 when the loop ends on the
// level's size first: what a plan's key records of maxSize.
int cv_max_level_end(const vj_cascade* c, int W, int H, double scale_factor, int max_w, int max_h);

// The plan of a call under the settings `t`: scales, feature tables, stage records, tile / row / bitmap lists, pruning rectangles,
// the pyramid's levels and taps.  small_batch: a call of at most four frames.  roc: a ROC call's maxSize, or nullptr.  *pl and
// *tab come fresh.  VJ_OK, or an error code with vj_last_error set; *pl and *tab are then unusable.
int plan_cv(const Tunables& t, const vj_cascade* c, int W, int H, const vj_cv_params& p, bool small_batch, const CvMaxSize* roc,
            CvPlanHost* pl, CvPlanTables* tab);

}  // namespace vj
