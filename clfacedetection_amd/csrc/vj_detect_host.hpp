// Layouts and arithmetic of the clod profile's detect drivers (vj_detect.cpp, vj_detect_regions.cpp).  No device, no
// HIP header: tests/detect_host_asan_driver.cpp checks every piece against brute force under ASan + UBSan.
#pragma once
#include "../../include/vj.h"
#include "vj_device.hpp"
#include "vj_grid_parts.hpp"

#include <algorithm>
#include <vector>

namespace vj {

// Where the counters of one batch live, in u32 slots of the lane's block: [MAX_PASSES][MAX_SCALES][Q_PARTS] queue counts |
// det_count | pad | one stage_entered[VJ_MAX_STAGES] (u64) array per kernel launch (array 0 is spare) | the block of a
// region-of-interest pass (vj_detect_rois, vj_detect_chain) | the queue counts of the tiles' own queue set (stage trees: split_sets).
struct CountsLayout {
    static constexpr size_t q_counts = (size_t)MAX_SCALES * Q_PARTS;   // counters of one queue: [scale][part]
    static constexpr size_t det_count_u32 = MAX_PASSES * q_counts;
    static constexpr size_t stage_off_u32 = det_count_u32 + 2;
    static constexpr size_t roi_off_u32 = stage_off_u32 + (size_t)(1 + VJ_MAX_LAUNCHES) * VJ_MAX_STAGES * 2;   // (array 1 + i: launch i)
    // the region block, slot by slot from roi_off_u32 (INVALID: regions outside their frames; GROUP_OVERFLOW: host copy only, the
    // flag itself sits in d_group; slot 7 is a pad; STAGES: the pass's stage_entered array, u64)
    enum RoiSlot : size_t { ROI_REGIONS, ROI_UNITS, ROI_INVALID, ROI_TICKET, ROI_DETS, ROI_GROUP_OVERFLOW, ROI_TILES, ROI_STAGES = 8 };
    static constexpr size_t roi_head_u32 = ROI_DETS + 1;   // regions .. detections: what the chain copies first
    static constexpr size_t roi_block_u32 = ROI_STAGES + (size_t)VJ_MAX_STAGES * 2;
    static constexpr size_t roi(RoiSlot s) { return roi_off_u32 + s; }
    static constexpr size_t q2_off_u32 = roi_off_u32 + roi_block_u32;   // second set of queue counters (stage trees)
    static constexpr size_t bytes = (q2_off_u32 + MAX_PASSES * q_counts) * sizeof(uint32_t);
    // The spare stage array (array 0) holds the tree counters (u64): the first cascade's visited child nodes and rectangles, the region pass's.
    static constexpr size_t tree_first_u64 = 0, tree_region_u64 = 2, tree_pair_bytes = 2 * sizeof(uint64_t);
    static constexpr size_t tree_region_u32 = stage_off_u32 + tree_region_u64 * 2;
    // Queue 0 does not exist, so its q_counts counters serve as tickets, zeroed with the block once per enqueue_cascade.  From
    // the front: pass ps draws from [ps * Q_PARTS, (ps + 1) * Q_PARTS) — pass 0 is the grid pass, whose GRID_PARTS parts of the
    // (frame, unit) list take the first range (one grid launch per zeroing); from the back: tile class c at
    // q_counts - 8 (c + 1), the region pass's tiles at q_counts - 40.
    static constexpr size_t ticket_range = 8;
    static constexpr size_t pass_tickets_end = (size_t)MAX_PASSES * Q_PARTS;
    static constexpr size_t tile_tickets_begin = q_counts - ticket_range * TILE_CLASSES;
    static constexpr size_t tile_tickets(uint32_t cls) { return q_counts - ticket_range * (cls + 1u); }
    static constexpr size_t roi_tickets_begin = q_counts - 40u;
};
static_assert(GRID_PARTS == Q_PARTS, "the grid pass's tickets are pass 0's range of queue 0's counters");
static_assert(CountsLayout::pass_tickets_end <= CountsLayout::roi_tickets_begin, "pass tickets (the grid pass's among them) end before the region pass's");
static_assert(CountsLayout::roi_tickets_begin + 8u <= CountsLayout::tile_tickets_begin, "the region pass's tile tickets end before the tile classes'");

// The lane's pinned read-back: the counters block, then (256-byte aligned) the first detections.
constexpr size_t PINNED_DET_OFF = (CountsLayout::bytes + 255) & ~(size_t)255;
inline size_t pinned_det_room(size_t pinned_bytes) { return (pinned_bytes - PINNED_DET_OFF) / sizeof(DetEntry); }

// The grouped hand-off's scratch (vj_detect_chain, min_neighbors != 0), one buffer: keys (u64) | grouped regions | the zeroed
// counter block (per frame: count, cursor, grouped count; then the overflow flag) | frame_first | the groups' weights | the regions'.
struct GroupLayout { size_t keys, grouped, zeroed, frame_first, grouped_weight, roi_weight, total; };
inline GroupLayout group_layout(size_t det_cap, size_t n_frames) {
    GroupLayout g = {};
    g.grouped = g.keys + det_cap * 8u;
    g.zeroed = g.grouped + det_cap * sizeof(RoiDev);
    g.frame_first = g.zeroed + (3u * n_frames + 1u) * 4u;
    g.grouped_weight = g.frame_first + (n_frames + 1u) * 4u;
    g.roi_weight = g.grouped_weight + det_cap * 4u;
    g.total = g.roi_weight + det_cap * 4u;
    return g;
}

// A DetEntry's / RoiDet's `off` — the byte offset of a window's origin in the batch sum image — as frame and position.
struct WindowAt { uint32_t frame, x, y; };
inline WindowAt decode_window(uint32_t off, uint32_t frame_elems, uint32_t stride) {
    const uint64_t fbytes = (uint64_t)frame_elems * 4u;
    const uint32_t f = (uint32_t)(off / fbytes);
    const uint32_t el = (uint32_t)((off - (uint64_t)f * fbytes) / 4u);
    return WindowAt{f, el % stride, el / stride};
}

// Frames per sub-batch so that 32-bit byte offsets into the batch sum image never wrap and the worst-case survivor queues stay
// within a fixed budget; 0: not even one frame can be addressed.  The queue limits never go below one frame: a single frame whose
// queue exceeds them is layout_queues' to refuse (past 2^32 - 1 entries) or the allocation's.
constexpr uint64_t Q_BUDGET_BYTES = 6ull << 30;   // per queue
inline uint64_t max_frames_for(uint64_t frame_elems, uint64_t max_reach_elems, uint64_t windows_per_frame, int max_subbatch) {
    const uint64_t frame_bytes = frame_elems * 4u, tail = max_reach_elems * 4u + 16u;
    if (!frame_bytes || tail > 0xffffffffull) return 0;
    uint64_t max_frames = (0xffffffffull - tail) / frame_bytes;
    // a queue holds Q_PARTS parts of ceil(frames / Q_PARTS) frames' worth of windows each (layout_queues)
    auto fit_parts = [](uint64_t worth) { return worth >= Q_PARTS ? worth / Q_PARTS * Q_PARTS : std::max<uint64_t>(1, worth); };
    if (windows_per_frame) {
        max_frames = std::min<uint64_t>(max_frames, fit_parts(Q_BUDGET_BYTES / sizeof(QEntry) / windows_per_frame));
        max_frames = std::min<uint64_t>(max_frames, fit_parts(0xffffffffull / windows_per_frame));
    }
    if (max_subbatch > 0) max_frames = std::min<uint64_t>(max_frames, (uint64_t)max_subbatch);
    return max_frames;
}

// Which passes of a cascade run where (enqueue_cascade).  Two chains share the first part of the cascade and run CONCURRENTLY
// on two streams:
//   A (e->stream) : the LDS-tile launches (LDS-bound)
//   B (e->stream2): the global-gather first pass and the queue passes that only it feeds (texture-address-bound) — every pass
//                   that begins before the stage at which tiles hand over (tiles leave at one boundary when tile_min_lanes = 0)
// then B joins A and the remaining queue passes, from first_joint_pass on, run on A.
struct PassSchedule {
    uint32_t handover;         // the stage at which tiles hand their survivors to the queues
    size_t first_joint_pass;
    bool two_streams;
    // Stage tree in chains (seg_last): the chains' queue passes would have to wait for BOTH the grid pass and the
    // tiles, because a crowded tile hands its windows to the same queues — and the tiles take longer than the grid
    // pass (4096 x 4096: 7.8 vs 4.8 ms, then 7.8 ms of queue passes).  So the tiles get a queue set of their own:
    // the grid pass's survivors go down the tree on stream B while the tiles still run, and after the join the same
    // passes run once more on what the tiles left (usually little: thin passes).
    bool split_sets;
};
// (tile_end: the CONFIGURED one, not the plan's clamped one; general: a stage tree, whose tiles run the linear prefix only)
inline PassSchedule pass_schedule(const std::vector<uint32_t>& pass_bounds, uint32_t tile_end, bool general, uint32_t general_prefix, int tile_min_lanes,
                                  uint32_t n_units, uint32_t n_tile_units, bool concurrent, bool tree_split_queues, bool seg_last_empty) {
    const size_t n_pass = pass_bounds.size() - 1;
    PassSchedule s;
    s.handover = general ? general_prefix : std::max<uint32_t>(tile_end, pass_bounds[1]);
    s.first_joint_pass = 1;
    if (tile_min_lanes == 0)
        while (s.first_joint_pass < n_pass && pass_bounds[s.first_joint_pass] < s.handover) ++s.first_joint_pass;
    s.two_streams = concurrent && n_tile_units > 0 && n_units > 0;
    s.split_sets = s.two_streams && general && !seg_last_empty && tree_split_queues;
    if (s.split_sets) s.first_joint_pass = n_pass;
    if (n_units == 0) s.first_joint_pass = 1;   // no gather chain: every queue pass is a joint one
    return s;
}

}  // namespace vj
