// Internals of the host driver shared by its translation units (vj_env.cpp: the environment; vj_detect*.cpp: the
// clod arithmetic profile's drivers; vj_cv.cpp: the OpenCV arithmetic profile).  Not part of the C ABI.
#pragma once
#include "vj_internal.hpp"
#include "vj_device.hpp"
#include "vj_tunables.hpp"
#include "vj_clod_plan.hpp"
#include "vj_cv_plan.hpp"
#include "vj_cv_roi_host.hpp"
#include "vj_cv_points_host.hpp"
#include "vj_points_host.hpp"
#include "vj_detect_host.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <type_traits>
#include <vector>

namespace vj {

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return VJ_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return VJ_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        // (a buffer never shrinks: alternating sizes reallocate only when a request exceeds every earlier one)
        size_t want = std::max(bytes, (size_t)256);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            p = nullptr;
            return e == hipErrorOutOfMemory ? VJ_ERR_NOMEM : VJ_ERR_HIP;
        }
        cap = want;
        return VJ_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// The capacity a 32-bit device counter's buffer grows to when `need` entries did not fit in `cap`: doubled in 64 bits (a
// 32-bit doubling wraps to 0 past 2^31 and never reaches `need`), at most 2^32 - 1 — the counters are 32-bit, so `need`
// itself never exceeds that.  The allocation that follows fails with VJ_ERR_NOMEM rather than loop when it cannot hold it.
inline uint32_t grown_cap(uint32_t cap, uint64_t need) {
    if (need <= cap) return cap;   // (a capacity of 0 that nothing asked for stays 0: it may mean "path unused")
    uint64_t c = std::max<uint64_t>(cap, 1u);
    while (c < need) c *= 2;
    return (uint32_t)std::min<uint64_t>(c, 0xffffffffull);
}

// A plan of the clod profile: what the planner computed (PlanHost, vj_clod_plan.hpp) and its device copies (upload_plan, vj_env.cpp).
struct Plan : PlanHost {
    DevBuf d_table, d_scales, d_stages, d_units, d_tile_units, d_sp_blocks, d_skip_units, d_skip_segs, d_pos_tab, d_unit_groups;
    int frames_q = 0;  // frames the ScaleDev.q_base/q_cap currently describe
    uint64_t last_used = 0;   // vj_env::plan_tick of the last call that used this plan (LRU eviction)
    void release_device() {
        for (DevBuf* b : {&d_table, &d_scales, &d_stages, &d_units, &d_tile_units, &d_sp_blocks, &d_skip_units, &d_skip_segs, &d_pos_tab, &d_unit_groups}) b->release();
    }
};

// A plan of the OpenCV profile: what the planner computed from (cascade, frame size, parameters) (CvPlanHost, vj_cv_plan.hpp) and its
// device copies (upload_cv_plan, vj_cv.cpp).  Kept per environment like the clod plans, so that a caller that hands over one frame
// per call (main.cpp:145) does not rebuild and upload 42 feature tables every time.
struct CvPlan : CvPlanHost {
    DevBuf d_table, d_scales, d_stages, d_rows;
    DevBuf d_tiles, d_rows_rest, d_bit_segs;   // LDS-tile path (vj_cv_tile.hip)
    DevBuf d_prune;                   // CV_HAAR_DO_CANNY_PRUNING: per scale slot
    DevBuf d_pyr_levels, d_pyr_taps;  // CV_HAAR_SCALE_IMAGE: the pyramid launch's level records and taps
    int tq_shift = -1;                // stage trees on tiles: the prefix survivors' sub-queues hold 1 / 2^shift of the tile windows
                                      // (-1: the environment's start value; lowered for THIS plan when a sub-queue overflows)
    int tq_split_frames = 0;          // frames per sub-batch the tree queue last split a batch to (CV_TQ_MAX; 0: never)
    uint64_t last_used = 0;
    void release_device() {
        for (DevBuf* b : {&d_table, &d_scales, &d_stages, &d_rows, &d_tiles, &d_rows_rest, &d_bit_segs, &d_prune, &d_pyr_levels, &d_pyr_taps}) b->release();
    }
};

// What the region pass (vj_detect_opencv_rois / _chain; vj_cv_roi.hip) derives from (cascade, frame stride, scale factor): the node
// tables depend on the factor and the frame's stride only, never on a region's size, so ONE table per factor — up to the last
// factor of the FRAME (no region inside it takes more) — serves every region of every call; it grows only when a taller frame of the width comes.
struct CvRoiPlan {
    std::vector<CvRoiFactor> factors;        // per factor slot k (scale_idx = k): window, step and feature reach
    StageProgram prog;
    uint32_t n_stages = 0, n_order = 0;
    bool trees = false, is_tree = false, has_tilted = false, tree2 = false;
    DevBuf d_table, d_scales, d_stages;
    // the chain's device hand-off (vj_cv_chain.hip): the enumeration's own factor of every slot, and the table the device's unit
    // builder reads (uploaded when a flagged call first needs it: chain_factors_n slots, 0 after the plan grew)
    std::vector<double> factor_values;
    DevBuf d_chain_factors;
    uint32_t chain_factors_n = 0;
    uint64_t last_used = 0;
    void release_device() {
        for (DevBuf* b : {&d_table, &d_scales, &d_stages, &d_chain_factors}) b->release();
        chain_factors_n = 0;
    }
};

// What a window-list pass (vj_cv_points.hip, vj_points.hip) derives from the cascade alone — the stage records — and
// from (cascade, frame stride, ONE scale): the scale's record and node table.  A call may name any number of scales; each is a plan
// of its own, so that the scales of successive calls (a tracker's jitter set, a ROC's fixed ladder) are built once.
struct PointCascade {
    uint32_t n_stages = 0, n_order = 0;
    bool trees = false, is_tree = false, has_tilted = false, tree2 = false;   // (the clod profile leaves the last two false)
    DevBuf d_stages;
    uint64_t last_used = 0;
    void release_device() { d_stages.release(); }
};
template <class ScaleDev>   // CvPointScaleDev, ClodPointScaleDev
struct PointPlan {
    typedef std::remove_cv_t<std::remove_pointer_t<decltype(ScaleDev::table)>> Node;   // CvNodeRec, NodeRec
    ScaleDev rec = {};            // table = d_table.p once built; win_w / win_h whatever the frame's height
    uint64_t max_reach = 0;       // furthest element a feature or the variance rectangle touches, from the window origin (once built)
    DevBuf d_table;               // built at the first call whose frame the window fits (no window of a larger one is evaluated)
    uint64_t last_used = 0;
    void release_device() { d_table.release(); }
};

}  // namespace vj

namespace vj {

// Everything ONE batch in flight owns: its frames on the device, its counters / detections and their host copies, and
// the events that time it.  vj_detect uses the environment's own lane; a vj_stream owns two, so that the upload of
// batch k+1 can run while the kernels of batch k do.  Integral images, survivor queues and plans are shared: the
// kernels of successive batches are ordered on the environment's stream.

struct Lane {
    DevBuf d_gray, d_counts, d_det;
    // VJ_FLAG_EQUALIZE_HIST (vj_equalize.hip): the sub-batch's frame records, histograms and look-up tables, and
    // its equalized gray frames at the device's pitch (each grows and is reused)
    DevBuf d_eq_frames, d_eq_hist, d_eq_lut, d_eq_gray;
    uint32_t det_cap = 0;
    void* h_pinned = nullptr;        // counters block + the first detections, read back asynchronously
    size_t h_pinned_bytes = 0;
    void* h_stage = nullptr;         // pinned staging of pageable host frames (streams)
    size_t h_stage_bytes = 0;
    hipEvent_t ev[4] = {};
    hipEvent_t pass_ev[VJ_MAX_PASSES + 1] = {};
    hipEvent_t launch_ev[2 * VJ_MAX_LAUNCHES] = {};   // start/stop per launch
    hipEvent_t upload_done = nullptr, integral_done = nullptr, done = nullptr;
    // the batch in flight (enqueue_batch -> finish_batch)
    bool pending = false;
    int nf = 0, first_frame = 0;
    // where the integral kernels read this batch's frames (the lane's d_gray or the caller's device batch), so that a
    // redo can recompute them: the lanes of a vj_stream share the environment's integral images, and by the time a
    // batch turns out to have overflowed its detection buffer the next batch's integrals have replaced its own
    const uint8_t* src_gray = nullptr;
    size_t src_frame_bytes = 0;
    int src_stride = 0, src_channels = 1;
    bool sq_u32 = false;             // this batch's squared integral is in the u32 layout (IntegralArgs::sq_u32); a redo keeps it
    bool shared_integrals = false;
    size_t n_pass = 0;
    int launches = 0;
    bool count = false;
    uint32_t det_copied = 0;         // detections already copied to h_pinned by the asynchronous read-back
    std::vector<vj_launch> linfo;
    int create();
    void destroy();
};

}  // namespace vj

struct vj_env : vj::Tunables {
    int device = 0;
    // Scale groups of the tile kernel: up to this many consecutive step-2 tile scales share one staged tile (1 = one
    // tile per scale).  Not a configure key: read once by vj_env_create (tile_group_from_env; a diagnostic).
    int tile_group = vj::TILE_GROUP_SHIPPED;
    // The tile passes read the squared-sum corners of a scale as dwords where its window area allows (ScaleDev::sq32).  Not a
    // configure key: VJ_SQ32=0, read once by vj_env_create, keeps every scale on the 64-bit form (a diagnostic).
    bool sq32 = true;
    // vj_detect and vj_stream keep the squared integral of a batch as u32, mod 2^32 (IntegralArgs::sq_u32): scales
    // with sq32 read its dwords, the others walk their variance window in strips.  Not a configure key: VJ_SQ_U32=0, read once by
    // vj_env_create, keeps those calls on the u64 layout, and so does VJ_SQ32=0.  Every other entry point uses the u64 layout.
    bool sq_u32 = true;
    hipStream_t stream = nullptr;
    vj::Lane lane0;                  // the batch of a plain vj_detect call
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    hipStream_t stream2 = nullptr;   // second chain of the first part of the cascade
    char name[256] = "";
    int n_cu = 0;
    // image buffers
    vj::DevBuf d_sum, d_sqsum, d_band_sum, d_band_sq, d_band_sqp;
    vj::DevBuf d_tilted;            // tilted integral images (OpenCV profile, cascades with tilted features)
    vj::DevBuf d_tilt_diag, d_tilt_col;   // ... its band totals (launch_tilted_bands)
    vj::DevBuf d_out;               // scratch for device -> host results (vj_grayscale)
    int slack_w = 0, slack_h = 0, slack_frames = 0;   // layout whose slack rows are known to be zero
    void *slack_sum = nullptr, *slack_sq = nullptr;
    bool slack_sq_u32 = false;      // ... of the squared integral in this layout
    // survivor queues + counters + detections
    vj::DevBuf d_q[vj::MAX_PASSES];   // d_q[p]: windows waiting to enter pass p (p >= 1)
    vj::DevBuf d_q2[vj::MAX_PASSES];  // stage trees: the tiles' own queue set (enqueue_cascade: split_sets)
    vj::DevBuf d_skip_bits;           // P2 skip modes: visited-window bitmaps of the frames in flight
    vj::DevBuf d_run_table;           // band-major queue pass: where every first-pass unit's survivors sit in their sub-queue
    vj::DevBuf d_rois, d_roi_units, d_roi_det, d_roi_tiles;   // regions of interest on the device (vj_detect_chain)
    uint32_t roi_tile_cap = 0;
    vj::DevBuf d_group;                          // scratch of the device-side grouping (vj_detect_chain, min_neighbors != 0)
    uint32_t roi_unit_cap = 0, roi_det_cap = 0;
    typedef std::tuple<uint64_t, int, int, int, int, int, int, uint32_t, uint64_t, uint64_t, uint32_t, uint32_t> PlanKey;
    std::map<PlanKey, std::unique_ptr<vj::Plan>> plans;
    // Chain balance per workload (cascade, frame size, parameters, batch-size CLASS): how much tile work goes to the
    // global-gather chain (Plan::tile_split) is found by a short hill climb on the measured cascade time of the workload's
    // first calls and then frozen; vj_env_configure("tile_split", ...) or ("auto_balance", "0") keep the static values.
    // The key names the cascade by CONTENT (two loads of one file share an entry; an exported table fits another process)
    // and the batch size by class (8-15, 16-31, 32-63, >= 64 frames; below 8 — single large frames — the exact count): a
    // service whose batch sizes vary searches four times, not once per size.  Only calls of the class's reference size
    // (n_ref: the first size seen, re-anchored when it stops coming) run candidates and feed the search — times are compared
    // per frame of ONE size —; every other call of the class runs the best split found so far.
    struct Balance {
        float cur = 0, best = 0, best_ms = 0, cand_ms = 0;   // (times: ms per frame)
        int phase = 0;        // 0: measuring the start value, 1: climbing up, 2: climbing down, 3: frozen, 4: measuring the other tile thresholds, 5: probing a whole scale further
        int samples = 0, moved = 0, calls = 0;
        int thr = 0;          // 0: the environment's tile thresholds; 1: scales whose tiles hold >= 384 windows go to tiles too
        bool thr_tried = false, far_tried = false;
        int n_ref = 0;        // frames per call of the calls that sample
        int off_ref = 0;      // calls of other sizes since n_ref was last seen
        bool first_slow = false;   // the candidate's unrated first call was already > 3 % slower than the best
        uint64_t last_used = 0;    // (least recently used entries go first when the table is full)
        uint32_t calls_total = 0, calls_on_candidate = 0;   // every call of the workload / those that ran a split other than the best known
    };
    typedef std::tuple<PlanKey, int> BalanceKey;    // the plan key with the cascade's content hash and split = 0, batch-size class
    std::map<BalanceKey, Balance> balance;
    uint64_t balance_tick = 0;
    typedef std::tuple<uint64_t, int, int, int, int, uint64_t, int, int> CvPlanKey;   // cascade uid, W, H, min size, bits of the scale factor,
                                                                                  // call of <= 4 frames (bit 0) | canny pruning (bit 1) | scale image (bit 2) | find biggest (bit 3)
                                                                                  // | reject levels (bit 4), the level at which a ROC call's maxSize ends the level loop (-1: none)
    std::map<CvPlanKey, std::unique_ptr<vj::CvPlan>> cv_plans;
    typedef std::tuple<uint64_t, int, uint64_t> CvRoiPlanKey;   // cascade uid, frame width (the tables' stride), bits of the scale factor
    std::map<CvRoiPlanKey, std::unique_ptr<vj::CvRoiPlan>> cv_roi_plans;
    vj::DevBuf d_cv_rois, d_cv_roi_units;   // region pass of the OpenCV profile: a sub-batch's regions and work units
    // vj_detect_opencv_chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE; vj_cv_chain.hip): per-frame counts, offsets and the state block;
    // the grouping's keys and per-frame rectangles; units per region and their offsets; the SECOND cascade's detections and counters
    // (the first one's stay in d_cv_det / d_cv_counts until the sub-batch's one synchronisation); events around the hand-off and the pass
    vj::DevBuf d_cv_chain, d_cv_chain_keys, d_cv_chain_staged, d_cv_roi_first, d_cv_det2, d_cv_counts2;
    hipEvent_t cv_chain_ev[3] = {};
    vj_cv_chain_info cv_chain_info = {};    // the last vj_detect_opencv_chain call (vj_cv_chain_info_get)
    // vj_detect_opencv_rois with VJ_FLAG_CV_SCALE_IMAGE (route 2): a canvas's level records, the call's taps, one scale
    // record per level image, the row units, the node table at factor 1 in the canvas's pitch, the stage records; events around the
    // pyramid launch
    vj::DevBuf d_cv_rl_levels, d_cv_rl_taps, d_cv_rl_scales, d_cv_rl_rows, d_cv_rl_table, d_cv_rl_stages;
    hipEvent_t cv_rois_ev[2] = {};
    vj_cv_rois_info cv_rois_info = {};      // the last vj_detect_opencv_rois call (vj_cv_rois_info_get)
    // The window-list calls (vj_points_driver.hpp), per profile: stage records per cascade uid; plans per (cascade uid, frame width, bits of
    // the scale[, tilted-as-upright]).  Under plan_cache_max, least recently used first — except the plans of the call in progress
    typedef std::map<uint64_t, std::unique_ptr<vj::PointCascade>> PointCascades;
    PointCascades cv_point_cascades, clod_point_cascades;
    typedef std::tuple<uint64_t, int, uint64_t> CvPointPlanKey;
    std::map<CvPointPlanKey, std::unique_ptr<vj::PointPlan<vj::CvPointScaleDev>>> cv_point_plans;
    typedef std::tuple<uint64_t, int, uint32_t, int> ClodPointPlanKey;
    std::map<ClodPointPlanKey, std::unique_ptr<vj::PointPlan<vj::ClodPointScaleDev>>> clod_point_plans;
    // ... both profiles, one call at a time: the last call's device times, summed over its sub-batches (vj_run_windows_timing); a
    // sub-batch's windows, units and verdicts and the call's scale records, each buffer sized in bytes per call
    float points_integral_ms = 0, points_pass_ms = 0;
    vj::DevBuf d_points, d_point_units, d_point_scales, d_point_out;
    vj::DevBuf d_cv_det, d_cv_counts;   // vj_detect_opencv: detection list and counters
    vj::DevBuf d_cv_accept, d_cv_tq;    // ... stage trees on tiles: accept bitmap, the queue of the prefix's survivors
    vj::DevBuf d_cv_fail_rows, d_cv_fail_walk;   // ... per-wave fail lists of the chain sweeps (rows kernel / chain pass)
    // CV_HAAR_DO_CANNY_PRUNING / vj_canny (vj_canny.hip): class bytes, union-find parents, strong-root flags, the 0 / 255 edge
    // maps and their integral images (a sub-batch's worth each)
    vj::DevBuf d_canny_cls, d_canny_label, d_canny_flag, d_edges, d_edge_sum, d_cv_prune_bits;   // (+ the tile scales' prune bitmap)
    vj::DevBuf d_pyr, d_pyr_tab;      // CV_HAAR_SCALE_IMAGE: the pyramid canvases of a sub-batch; level table + taps of vj_resize_linear
    vj::DevBuf d_cv_big;              // CV_HAAR_FIND_BIGGEST_OBJECT: a sub-batch's search states (CvBigState), then its frames' candidate counts
    int edge_slack_w = 0, edge_slack_h = 0, edge_slack_frames = 0;   // layout whose slack rows of d_edge_sum are known to be zero
    void* edge_slack_sum = nullptr;
    // vj_detect_mixed / vj_detect_opencv_mixed / vj_pack_frames (vj_mixed.cpp): the 8-bit atlas (grows, reused), the
    // block one copy brings per atlas — its frame records, then its host frames at a 4-byte pitch —, events around the pack launch
    vj::DevBuf d_atlas, d_atlas_src;
    hipEvent_t atlas_ev[2] = {};
    vj_mixed_info mixed_info = {};          // the last mixed call (vj_mixed_info_get)
    // The frame-processing calls (vj_slice.hpp): a call brings each of its slices in one block that grows and is reused —
    // records, taps or lists, then the slice's host frames at a 4-byte pitch through lane0's h_stage —, and has finished with it when
    // it returns.  Calls on an environment do not overlap, so ONE pair of events lies around the copies and launches of whichever
    // call runs; every entry point keeps the time of its last call (vj_*_timing).
    hipEvent_t call_ev[2] = {};
    vj::DevBuf d_prep;      // vj_preprocess (§4.16): [frame records | the records equalize_lut reads | taps | frames]; histograms
                            // and tables: lane0's d_eq_hist / d_eq_lut
    vj::DevBuf d_extract;   // vj_extract (§4.17): [region records | taps | frames]; vj_extract_affine (§4.19): [region records | frames];
                            // vj_extract_yuv / vj_extract_affine_yuv (§4.25): [region records | taps | planes];
                            // vj_paint (§4.20) and vj_paint_yuv (§4.23): [records | overlap lists | touched rows | scratch]
    vj::DevBuf d_yuv;       // vj_yuv_to_bgr / vj_bgr_to_yuv (§4.21): [frame records | planes]
    float prep_ms = 0, extract_ms = 0, affine_ms = 0, paint_ms = 0, paint_yuv_ms = 0, yuv_ms = 0, extract_yuv_ms = 0;
    // vj_track (vj_track.cpp): its scratch — the templates, the search patches, the match records (grows, reused);
    // its slices come through d_extract like vj_extract's —, events around a call [0, 1] and around a match launch [2, 3], their times
    vj::DevBuf d_track;
    hipEvent_t track_ev[4] = {};
    float track_ms = 0, track_match_ms = 0;
    uint64_t plan_tick = 0;
    int cv_tq_shift = 4;              // ... stage trees: the survivors' queue holds 1 / 2^shift of the tile windows (grows on overflow)
};

namespace vj {
// image staging and the integral launches (vj_env.cpp)
int image_channels(const vj_image& im);
int check_single_image(const vj_image* image, int* ch_out);   // VJ_ERR_ARG / VJ_ERR_LIMIT, else the channel count
int ensure_image_buffers(vj_env* e, int W, int H, int frames, bool need_gray, int channels = 1, Lane* lane = nullptr);
// (sq_u32: the squared integral in the u32 layout, for readers that are told so — CascadeArgs::sq_u32; default: u64)
int enqueue_integral(vj_env* e, const uint8_t* d_gray, size_t frame_bytes, int stride, int W, int H, int frames,
                     int channels = 1, bool sq_u32 = false);
int stage_frames(vj_env* e, const vj_image* frames, int n, int W, int H, const uint8_t** d_ptr, size_t* frame_bytes,
                 int* stride, Lane* lane = nullptr, hipStream_t copy_stream = nullptr);
int check_frames(const vj_image* frames, int n_frames, int* W, int* H, int* CH);   // a batch: frames of one size and channel count
int enqueue_tilted(vj_env* e, const uint8_t* d_gray, size_t frame_bytes, int stride, int W, int H, int frames, int channels);
// VJ_FLAG_EQUALIZE_HIST, right after stage_frames: the `frames` staged frames (what stage_frames returned) equalized into the lane's
// gray batch — one memset and three launches on the environment's stream, nothing waited for — and *d_gray, *frame_bytes, *stride,
// *channels (1 from here on) name that batch.
int enqueue_equalize(vj_env* e, Lane* lane, const uint8_t** d_gray, size_t* frame_bytes, int* stride, int* channels, int W, int H, int frames);
// ... the histograms and tables alone, for frame records already on the device (hist_first filled in): what an atlas needs before
// atlas_pack<true>.  *lut: the tables, 256 bytes per frame.
int enqueue_equalize_tables(vj_env* e, Lane* lane, const void* d_frame_recs, uint32_t n_frames, uint32_t n_hist_units, const uint8_t** lut);
// What an entry point that does not equalize answers to the flag: VJ_ERR_UNSUPPORTED, vj_last_error names both; else VJ_OK.
int refuse_equalize(uint32_t flags, const char* entry_point);

// The clod profile's plans and chain-balance search (vj_env.cpp), for its drivers (vj_detect*.cpp).
int get_plan(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, Plan** out, int n_frames = 1 << 20);   // the cached plan
int plan_and_upload(const vj_env* e, const vj_cascade& c, int W, int H, const vj_params& p, Plan* pl, float tile_split,
                    const TileThresholds& thresholds, int n_frames, bool one_pass);   // a plan outside the cache (a stream's own)
int layout_queues(Plan* pl, int frames, uint64_t* total_entries);
struct BalanceChoice { float split; int thr; bool candidate; };
vj_env::Balance* balance_of(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, int n_frames, bool create);
BalanceChoice balance_choice(const vj_env::Balance* b, int n_frames);
void balance_touch(vj_env::Balance* b, int n_frames);
void balance_report(vj_env::Balance* b, float ms, bool try_thresholds);

// What the clod profile's detect drivers share (vj_detect.cpp: batches through the cascade, blocking and streamed; vj_detect_regions.cpp: a second cascade inside regions).
struct RawDet { int frame; uint32_t slot, x, y; };
int ensure_queues(vj_env* e, Plan* pl, int frames);   // lay out the plan's queues for `frames` frames in flight, ensure d_q[1 .. n_pass)
// Upload (or adopt) the frames of one batch and enqueue its integral images.  `copy_stream` != null (vj_stream): the upload runs on that stream and the integral waits for it.
int enqueue_prepare(vj_env* e, Lane* L, Plan* pl, const vj_image* frames, int nf, int W, int H, bool fixed_queue_layout,
                    hipStream_t copy_stream, bool equalize = false, bool sq_u32 = false);
// Enqueue every cascade launch of the batch whose integral images are (being) computed, then the asynchronous read-back.  Nothing here waits for the device.
int enqueue_cascade(vj_env* e, Lane* L, Plan* pl, int W, const vj_params& p);
// What every cascade launch on `pl` reads of the plan, the lane and the integral images of nf frames (the rest zeroed).
void fill_plan_args(const vj_env* e, const Lane* L, const Plan* pl, int nf, int W, const vj_params& p, CascadeArgs& ca);
int finish_batch(vj_env* e, Lane* L, Plan* pl, int f0, int W, int H, const vj_params& p, std::vector<RawDet>* dets,
                 vj_counters* ctr, vj_timing* tm);
// Sort, widen and (optionally) group the decoded detections of a whole call (a region pass: `frame` is the region), then fill_counters: the derived counters for `windows` windows.
int build_result(const Plan* pl, std::vector<RawDet>& dets, uint64_t windows, const vj_params& p, vj_result* out);
void fill_counters(const Plan* pl, uint64_t windows, const vj_params& p, vj_counters* k);
int rects_to_result(const std::vector<vj_rect>& rects, vj_result* out);
uint64_t max_frames_per_subbatch(const vj_env* e, const Plan* pl);
int subbatch_frames(const vj_env* e, const Plan* pl, const Plan* pl2, uint64_t* max_frames);   // ... of every plan of a call: VJ_ERR_LIMIT at 0
void balance_feedback(vj_env::Balance* bal, const vj_env* e, const Plan* pl, const vj_params& p, int n_frames, uint64_t max_frames, vj_timing* timing);

// Room for one more entry in a plan cache bounded by plan_cache_max: the least recently used go first and release their tables (the
// caller has synchronised the stream that may still read them).  An entry with last_used >= keep_tick stays: the run-windows calls
// (vj_run_windows_opencv, vj_run_windows) pass the tick of the call in progress — a call that names more scales than plan_cache_max
// keeps them all while it runs.
template <typename Map>
void cache_make_room(vj_env* e, Map& m, uint64_t keep_tick = ~0ull) {
    while ((int)m.size() >= std::max(1, e->plan_cache_max)) {
        auto lru = m.end();
        for (auto i = m.begin(); i != m.end(); ++i)
            if (i->second->last_used < keep_tick && (lru == m.end() || i->second->last_used < lru->second->last_used)) lru = i;
        if (lru == m.end()) return;
        lru->second->release_device();
        m.erase(lru);
    }
}
}  // namespace vj
