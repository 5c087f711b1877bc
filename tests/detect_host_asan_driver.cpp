// Sanitizer driver of the clod detect drivers' layouts and arithmetic (csrc/vj_detect_host.hpp), built by
// tests/test_sanitizers_detect_host.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/detect_host_asan_driver.cpp
// from that header alone (no HIP involved).  Against brute force:
//   counters block   every named range of CountsLayout lies inside `bytes` and no two overlap (a byte map);
//   grouped buffer   the parts do not overlap, the u64 part is 8-byte aligned and the rest 4-byte aligned, `total` is the formula restated
//                    here;
//   offset decode    inverts the encoding for every window of a 5-frame batch of 13 x 9 frames, and at the last element of a frame
//                    whose frame_elems * 4 * nf is just under 2^32;
//   max_frames       the count keeps every byte offset + reach + 16 below 2^32, the queue within its budget and windows x frames
//                    below 2^32, and the next count breaks one of these or max_subbatch;
//   pass schedule    equals a literal restatement of enqueue_cascade's decisions written as one function.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_detect_host.hpp"

using namespace vj;
typedef CountsLayout CL;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

// ------------------------------------------------------------------ counters block
static std::vector<uint8_t> g_map;
static size_t g_ranges = 0;
static void mark_u32(size_t first_u32, size_t n_u32) {
    CHECK(n_u32 > 0 && (first_u32 + n_u32) * 4 <= CL::bytes);
    for (size_t b = first_u32 * 4; b < (first_u32 + n_u32) * 4; ++b) {
        CHECK(g_map[b] == 0);
        g_map[b] = 1;
    }
    ++g_ranges;
}

static void check_counts_layout() {
    g_map.assign(CL::bytes, 0);
    for (int set = 0; set < 2; ++set) {
        const size_t base = set ? CL::q2_off_u32 : 0;
        for (size_t ps = 1; ps < (size_t)MAX_PASSES; ++ps) mark_u32(base + ps * CL::q_counts, CL::q_counts);   // queue counters [scale][part]
        for (size_t ps = 0; ps < (size_t)MAX_PASSES; ++ps) mark_u32(base + ps * Q_PARTS, Q_PARTS);              // pass tickets in queue 0's counters
    }
    CHECK(CL::pass_tickets_end == (size_t)MAX_PASSES * Q_PARTS);
    mark_u32(CL::roi_tickets_begin, CL::ticket_range);
    for (uint32_t c = 0; c < (uint32_t)TILE_CLASSES; ++c) mark_u32(CL::tile_tickets(c), CL::ticket_range);
    CHECK(CL::tile_tickets(TILE_CLASSES - 1) == CL::tile_tickets_begin && CL::tile_tickets(0) + CL::ticket_range == CL::q_counts);
    mark_u32(CL::det_count_u32, 1);
    // the spare stage array's tree counters (u64 pairs), then one stage array per launch
    mark_u32(CL::stage_off_u32 + CL::tree_first_u64 * 2, CL::tree_pair_bytes / 4);
    mark_u32(CL::tree_region_u32, CL::tree_pair_bytes / 4);
    CHECK(CL::tree_region_u32 == CL::stage_off_u32 + CL::tree_region_u64 * 2 && CL::stage_off_u32 % 2 == 0);
    CHECK((CL::tree_region_u64 + 2) <= (size_t)VJ_MAX_STAGES);
    for (size_t l = 0; l < (size_t)VJ_MAX_LAUNCHES; ++l) mark_u32(CL::stage_off_u32 + (1 + l) * VJ_MAX_STAGES * 2, (size_t)VJ_MAX_STAGES * 2);
    // the region block
    for (CL::RoiSlot s : {CL::ROI_REGIONS, CL::ROI_UNITS, CL::ROI_INVALID, CL::ROI_TICKET, CL::ROI_DETS, CL::ROI_GROUP_OVERFLOW, CL::ROI_TILES})
        mark_u32(CL::roi(s), 1);
    mark_u32(CL::roi(CL::ROI_STAGES), (size_t)VJ_MAX_STAGES * 2);
    CHECK(CL::roi(CL::ROI_STAGES) % 2 == 0);                                    // (u64 counters)
    CHECK(CL::roi_head_u32 == 5 && CL::roi_off_u32 + CL::roi_block_u32 == CL::q2_off_u32);
    CHECK(CL::roi(CL::ROI_STAGES) + (size_t)VJ_MAX_STAGES * 2 == CL::q2_off_u32);
    CHECK(g_ranges == 2 * (2 * (size_t)MAX_PASSES - 1) + 1 + TILE_CLASSES + 1 + 2 + VJ_MAX_LAUNCHES + 7 + 1);
    // the pinned read-back: detections after the block, 256-byte aligned, room counted in whole entries
    CHECK(PINNED_DET_OFF >= CL::bytes && PINNED_DET_OFF % 256 == 0 && PINNED_DET_OFF - CL::bytes < 256);
    for (size_t pinned : {PINNED_DET_OFF, PINNED_DET_OFF + 7, PINNED_DET_OFF + 8, (size_t)1 << 20}) {
        const size_t room = pinned_det_room(pinned);
        CHECK(PINNED_DET_OFF + room * sizeof(DetEntry) <= pinned && PINNED_DET_OFF + (room + 1) * sizeof(DetEntry) > pinned);
    }
}

// ------------------------------------------------------------------ grouped buffer
static void check_group_layout() {
    for (size_t cap : {1u, 2u, 63u, 64u, 65u, 4096u})
        for (size_t nf : {1u, 2u, 7u, 64u}) {
            const GroupLayout g = group_layout(cap, nf);
            // the formula restated: keys (u64) | grouped | the zeroed counter block | frame_first | weights | weights
            const size_t o_keys = 0, o_grouped = o_keys + cap * 8u, o_zero = o_grouped + cap * sizeof(RoiDev), o_first = o_zero + (3u * nf + 1u) * 4u,
                         o_gw = o_first + (nf + 1u) * 4u, o_rw = o_gw + cap * 4u, total = o_rw + cap * 4u;
            CHECK(g.keys == o_keys && g.grouped == o_grouped && g.zeroed == o_zero && g.frame_first == o_first && g.grouped_weight == o_gw &&
                  g.roi_weight == o_rw && g.total == total);
            const size_t first[] = {g.keys, g.grouped, g.zeroed, g.frame_first, g.grouped_weight, g.roi_weight};
            const size_t bytes[] = {cap * 8u, cap * sizeof(RoiDev), (3u * nf + 1u) * 4u, (nf + 1u) * 4u, cap * 4u, cap * 4u};
            std::vector<uint8_t> map(g.total, 0);
            for (int k = 0; k < 6; ++k) {
                CHECK(first[k] % (k == 0 ? 8u : 4u) == 0 && first[k] + bytes[k] <= g.total);
                for (size_t b = first[k]; b < first[k] + bytes[k]; ++b) {
                    CHECK(map[b] == 0);
                    map[b] = 1;
                }
            }
        }
}

// ------------------------------------------------------------------ offset decode
static void check_decode() {
    {
        const uint32_t W = 13, H = 9, stride = W + 1, nf = 5;
        const uint32_t frame_elems = ((stride * (H + 1) + 63u) / 64u) * 64u + 64u;   // (rows past H and an alignment tail, as frame_elems_for leaves)
        size_t n = 0;
        for (uint32_t f = 0; f < nf; ++f)
            for (uint32_t y = 0; y <= H; ++y)
                for (uint32_t x = 0; x <= W; ++x, ++n) {
                    const uint32_t off = (uint32_t)(((uint64_t)f * frame_elems + (uint64_t)y * stride + x) * 4u);
                    const WindowAt at = decode_window(off, frame_elems, stride);
                    CHECK(at.frame == f && at.x == x && at.y == y);
                }
        CHECK(n == (size_t)nf * 14 * 10);
    }
    {   // the last element of the last frame of a batch whose sum image is just under 2^32 bytes
        const uint32_t stride = 32767, nf = 3;
        const uint32_t frame_elems = (uint32_t)(0xffffffffull / 4u / nf);
        CHECK((uint64_t)frame_elems * 4u * nf < (1ull << 32) && (uint64_t)(frame_elems + 1) * 4u * nf >= (1ull << 32));
        for (uint32_t f = 0; f < nf; ++f) {
            const uint32_t el = frame_elems - 1;
            const uint32_t off = (uint32_t)(((uint64_t)f * frame_elems + el) * 4u);
            const WindowAt at = decode_window(off, frame_elems, stride);
            CHECK(at.frame == f && at.x == el % stride && at.y == el / stride);
        }
    }
}

// ------------------------------------------------------------------ max_frames
// What n frames in flight need (layout_queues: Q_PARTS parts of ceil(n / Q_PARTS) frames' worth of windows each, one part per
// frame below Q_PARTS frames).
static bool offsets_fit(uint64_t n, uint64_t fe, uint64_t reach) { return (__uint128_t)n * fe * 4u + (__uint128_t)reach * 4u + 16u <= 0xffffffffull; }
static bool queue_fits(uint64_t n, uint64_t wpf) {
    const __uint128_t per_part = n >= Q_PARTS ? (n + Q_PARTS - 1) / Q_PARTS : 1, parts = n >= Q_PARTS ? Q_PARTS : n;
    const __uint128_t entries = (__uint128_t)wpf * per_part * parts;
    return entries * sizeof(QEntry) <= Q_BUDGET_BYTES && entries <= 0xffffffffull;
}
static void check_max_frames() {
    const uint64_t edge[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 1000, 65535, 65536, 1u << 20, (1u << 24) + 3, (1u << 28) - 1, 1u << 28, (1u << 30) - 1, 1u << 30,
                             0x7fffffffull, 0x80000000ull, 0xfffffffbull, 0xfffffffeull, 0xffffffffull};
    const int subs[] = {0, -1, 1, 2, 7, 8, 9, 100, 0x7fffffff};
    size_t n_zero = 0, n_floor = 0, n_by_offsets = 0, n_by_queue = 0, n_by_sub = 0;
    for (uint64_t fe : edge)
        for (uint64_t reach : edge)
            for (uint64_t wpf : edge)
                for (int sub : subs) {
                    const uint64_t n = max_frames_for(fe, reach, wpf, sub);
                    if (n == 0) {   // not even one frame can be addressed (or there is no frame at all)
                        CHECK(fe == 0 || !offsets_fit(1, fe, reach));
                        ++n_zero;
                        continue;
                    }
                    CHECK(fe != 0 && offsets_fit(n, fe, reach));
                    CHECK(sub <= 0 || n <= (uint64_t)sub);
                    // the floor of the queue limits: a single frame is never split, so its queue is checked
                    // where it is laid out (csrc/vj_env.cpp, layout_queues: VJ_ERR_LIMIT "survivor queue needs N entries" past 2^32 - 1)
                    if (n == 1 && wpf && !queue_fits(1, wpf)) {
                        ++n_floor;
                        continue;
                    }
                    CHECK(!wpf || queue_fits(n, wpf));
                    const bool sub_breaks = sub > 0 && n + 1 > (uint64_t)sub, off_breaks = !offsets_fit(n + 1, fe, reach), q_breaks = wpf && !queue_fits(n + 1, wpf);
                    CHECK(sub_breaks || off_breaks || q_breaks);
                    n_by_sub += sub_breaks, n_by_offsets += off_breaks, n_by_queue += q_breaks;
                }
    CHECK(n_zero > 100 && n_floor > 10 && n_by_offsets > 100 && n_by_queue > 100 && n_by_sub > 100);
}

// ------------------------------------------------------------------ pass schedule
// enqueue_cascade's decisions restated as one function (handover / first_joint_pass / two_streams / split_sets, and chain B's
// "no gather units: the first joint pass is 1").
static PassSchedule schedule_restated(const std::vector<uint32_t>& pass_bounds, uint32_t e_tile_end, bool general, uint32_t general_prefix, int tile_min_lanes,
                                      uint32_t n_units, uint32_t n_tile_units, bool concurrent, bool tree_split_queues, bool seg_last_empty) {
    const size_t n_pass = pass_bounds.size() - 1;
    const uint32_t ca_tile_end = general ? general_prefix : e_tile_end;
    const uint32_t handover = general ? general_prefix : std::max<uint32_t>(ca_tile_end, pass_bounds[1]);
    size_t first_joint_pass = 1;
    if (tile_min_lanes == 0)
        while (first_joint_pass < n_pass && pass_bounds[first_joint_pass] < handover) ++first_joint_pass;
    const bool two_streams = concurrent && n_tile_units > 0 && n_units > 0;
    const bool split_sets = two_streams && general && !seg_last_empty && tree_split_queues;
    if (split_sets) first_joint_pass = n_pass;
    if (!(n_units > 0)) first_joint_pass = 1;
    return PassSchedule{handover, first_joint_pass, two_streams, split_sets};
}

static void check_schedule() {
    const uint32_t N = 22;
    const std::vector<std::vector<uint32_t>> bounds = {{0, N}, {0, 3, N}, {0, 3, 8, N}, {0, 2, 5, 9, N}};
    size_t n = 0, n_split = 0, n_two = 0, n_joint_late = 0;
    for (const std::vector<uint32_t>& pb : bounds) {
        std::vector<uint32_t> ends = {0};
        for (uint32_t b : pb)
            for (int d = -1; d <= 1; ++d)
                if ((int)b + d >= 0) ends.push_back(b + d);   // on, below and above every boundary
        for (uint32_t tile_end : ends)
            for (uint32_t prefix : ends)
                for (int flags = 0; flags < 32; ++flags)
                    for (uint32_t n_units = 0; n_units < 2; ++n_units)
                        for (uint32_t n_tile_units = 0; n_tile_units < 2; ++n_tile_units) {
                            const bool general = flags & 1, concurrent = flags & 2, split = flags & 4, seg_empty = flags & 8;
                            const int min_lanes = flags & 16 ? 8 : 0;
                            const PassSchedule a = pass_schedule(pb, tile_end, general, prefix, min_lanes, n_units, n_tile_units, concurrent, split, seg_empty);
                            const PassSchedule b = schedule_restated(pb, tile_end, general, prefix, min_lanes, n_units, n_tile_units, concurrent, split, seg_empty);
                            CHECK(a.handover == b.handover && a.first_joint_pass == b.first_joint_pass && a.two_streams == b.two_streams && a.split_sets == b.split_sets);
                            CHECK(a.first_joint_pass >= 1 && a.first_joint_pass <= std::max<size_t>(1, pb.size() - 1));
                            ++n, n_split += a.split_sets, n_two += a.two_streams, n_joint_late += a.first_joint_pass > 1;
                        }
    }
    CHECK(n > 10000 && n_split > 100 && n_two > 1000 && n_joint_late > 1000);
}

int main() {
    check_counts_layout();
    check_group_layout();
    check_decode();
    check_max_frames();
    check_schedule();
    printf("detect_host_asan_driver: OK\n");
    return 0;
}
