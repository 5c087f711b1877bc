// The planner of the clod profile (vj_clod_plan.cpp): everything the kernels of a vj_detect call read, computed on the host
// from (cascade, frame size, parameters, settings).  No HIP type in it: the driver uploads the result (upload_plan,
// vj_env.cpp), the plan query (vj_plan_tiles) reads it as it is, and the sanitizer driver runs it without a device.
#pragma once
#include "vj_tunables.hpp"

#include <utility>
#include <vector>

namespace vj {

// Everything that depends on (cascade, W, H, params) but not on pixel data: what the host keeps of a plan.
struct PlanHost {
    std::vector<vj_scale_info> scales_all;   // every enumerated scale
    std::vector<ScaleDev> scales;            // accepted scales with nwin > 0
    std::vector<vj_scale_info> scales_info;  // same order as `scales`
    std::vector<std::pair<uint32_t, uint32_t>> tile_reach;   // same order: how far right / down of a window origin the scale's features read
    std::vector<StageDev> stages;
    std::vector<UnitDev> units;              // first-pass units of one frame (global-gather scales), band-major (q_band_px)
    uint32_t unit_cap = UNIT_WINDOWS;        // ... of at most this many windows each: the per-wave queue capacity of the wave count the plan
                                             // was built for (vj_gather_queue.hpp); a launch runs at most the waves whose queues hold one
    std::vector<UnitDev> unit_groups;        // runs of consecutive units of one (band, scale): what a wave of the band-major queue pass draws
    std::vector<UnitDev> tile_units;         // first-pass tiles of one frame, grouped by LDS class
    std::vector<uint32_t> tile_lead;         // per scale: the largest scale of its tile group (itself when not grouped)
    uint32_t class_first[TILE_CLASSES + 1] = {};  // tile_units range of each class
    uint32_t class_lds[TILE_CLASSES] = {};        // dynamic LDS bytes of each class launch
    uint32_t tile_end = 0;                        // stage at which the tile launches stop
    bool tree2 = false;                           // every tree: two nodes, node 1 the only node child of node 0
    bool wave_tail = false;                       // stump cascade whose stages fit the wave-independent tail's blocks
    std::vector<uint32_t> pass_bounds;       // stage indices: pass p runs [b[p], b[p+1])
    uint64_t windows_per_frame = 0;
    uint32_t frame_elems = 0;
    uint32_t max_reach_elems = 0;  // furthest element a window origin + feature corner touches
    bool trees = false;    // some tree has more than one node
    bool general = false;  // stage tree (not a linear chain of stages)
    uint32_t general_prefix = 0;  // stage tree: positions [0, prefix) of the sweep order form a linear chain (pass -> next,
                                  // fail -> reject) that runs on the linear kernels (tiles included)
    // Stage tree cut into linear segments (chains of the sweep order whose rejects all go to one place): pass ps reads
    // queue ps; seg_last[ps]: its survivors are detections; seg_fail[ps]: queue that takes its rejects (0 = none).
    // Empty when the tree does not have that shape: then one general pass (run_stages_general) finishes it.
    std::vector<uint8_t> seg_last, seg_fail;
    // the same chains for the tile kernel, which runs them itself when chain k's rejects feed chain k+1
    uint32_t tile_n_seg = 0, tile_seg_end[4] = {}, tile_seg_chain = 0;
    uint32_t n_order = 0;  // stages reachable from stage 0, in StageDev::order
    uint32_t max_stage_nodes = 0;
    StageProgram prog;
    // P2 skip modes (VJ_FLAG_SKIP_LIST / VJ_FLAG_SKIP_ROW): bitmap geometry and work lists of the two bitmap kernels
    uint32_t skip_mode = 0, pos_mode = 0, skip_frame_words = 0, n_skip_units = 0, n_skip_segs = 0;
    uint32_t n_sp_blocks = 0;
    float tile_split = 0.0f;  // the chain balance this plan was built for (Tunables::split_for)
};

// What a plan holds only to be uploaded: the host keeps no copy after upload_plan.
struct PlanTables {
    std::vector<NodeRec> table;            // per scale: the frame-stride records, its tile-pitch and group-pitch records, the tail's copies
    std::vector<uint32_t> pos_tab;         // VJ_FLAG_GRID_F64: window positions by grid index (ScaleDev::pos_base)
    std::vector<SpBlock> sp_blocks;        // blocks of the tile kernel's wave-independent tail
    std::vector<UnitDev> skip_units, skip_segs;   // P2 skip modes: work lists of the two bitmap kernels
};

// Which scales go to LDS tiles: a class is acceptable for a scale when a tile holds at least min_windows windows, a scale
// whose best tile holds fewer than accept_windows stays on the global-gather path, and staging a tile may cost at most
// max_dwords_per_window.
struct TileThresholds { int min_windows, accept_windows, max_dwords_per_window; };
// The tile thresholds of a plan: the settings', those of small_frame_class (1, 2), or the balance feedback's lower ones (3).
TileThresholds thresholds_for(const Tunables& t, int small);
int small_frame_class(const Tunables& t, int W, int H, int n_frames);
// A call of at most one_pass_max_frames frames of 720p and more runs the gather chain in one pass (plan_clod refuses the
// request for tree cascades and under a pass_split).
inline bool one_pass_for(const Tunables& t, int W, int H, int n_frames) {
    // (below 720p the queue pass costs nothing — 640 x 480 0.473 / 0.476 ms with / without it, 320 x 240 the same)
    return n_frames <= t.one_pass_max_frames && (uint64_t)W * (uint64_t)H >= 800000ull;
}

bool has_trees(const vj_cascade& c);       // some tree has more than one node
bool linear_stumps(const vj_cascade& c);   // a linear cascade of stumps (Tunables::gather_waves_for, split_for)
uint32_t frame_elems_for(int W, int H);    // elements of one frame of the integral images, slack rows included
// What every entry point that takes a vj_params checks before it plans anything: VJ_ERR_ARG for a flag combination no plan
// describes (VJ_FLAG_GRID_F64 alone would give the region pass a position table its launcher never binds).
int check_params(const vj_params& p);
// Scales per tile group: VJ_TILE_GROUP (a diagnostic), read when an environment is created and by the plan query.
constexpr int TILE_GROUP_SHIPPED = 4;
int tile_group_from_env();

// The plan of a call of n_frames frames (it decides the gather chain's wave count and with it the size of the first-pass
// units).  tile_group, sq32: the environment's two diagnostics (vj_env).  former_shapes: the shape search as it was before
// round 11, for the plan dump (tools/plan_dump.py).  VJ_OK, or an error code with vj_last_error set; *pl and *tab are then unusable.
int plan_clod(const Tunables& t, int tile_group, bool sq32, const vj_cascade& c, int W, int H, const vj_params& p, float tile_split,
              const TileThresholds& thresholds, int n_frames, bool one_pass, bool former_shapes, PlanHost* pl, PlanTables* tab);

}  // namespace vj
