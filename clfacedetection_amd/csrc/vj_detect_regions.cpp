// A second cascade inside regions of the frames, on the frames' own integral images: vj_detect_rois (the caller's regions) and
// vj_detect_chain (the first cascade's detections, handed over on the device), ONE region pass per sub-batch.
#include "vj_env_internal.hpp"

using namespace vj;
typedef CountsLayout CL;

namespace {

// One sub-batch's region pass: the second cascade, where it runs and what the pass that fitted left.
struct RegionPass {
    vj_env* e;
    Lane* L;
    Plan* pl2;
    const vj_cascade* second;
    const vj_params* p_second;
    int W, H, nf;
    uint32_t n_reg;        // vj_detect_rois: the caller's regions, uploaded to e->d_rois
    uint32_t n_det2 = 0;   // what the pass that fitted left: its detections ...
    float ms = 0;          // ... and its time on the device
    const uint32_t* host_counts() const { return (const uint32_t*)L->h_pinned; }
    uint32_t* dev_counts() const { return (uint32_t*)L->d_counts.p; }
    int copy_counts(size_t first_u32, size_t n_bytes) const {   // a range of the counters block to its place in the pinned copy
        HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + first_u32, dev_counts() + first_u32, n_bytes, hipMemcpyDeviceToHost, e->stream));
        return VJ_OK;
    }
};

// vj_detect_chain's part of a region pass: the first cascade, whose detections (grouped on the device when `grouped`) are the regions.
struct ChainHandoff {
    Plan* pl1;
    const vj_params* p_first;
    bool grouped;
    GroupArgs ga;
};

// Arguments of the region pass (roi_plan_units + cascade_roi_pass): `second` inside regions of the nf frames whose integral images sit in e->d_sum / e->d_sqsum.  The region list is
// e->d_rois (max_rois entries), its length on the device at the region block's first slot; the counters live in the lane's counts block.  pl1: the plan whose detections are the regions.
void fill_region_args(const RegionPass& rp, uint32_t max_rois, const Plan* pl1, RoiArgs& ra, CascadeArgs& ca) {
    const vj_env* e = rp.e;
    const Plan* pl2 = rp.pl2;
    uint32_t* counts = rp.dev_counts();
    memset(&ra, 0, sizeof(ra));
    ra.frame_bytes = pl2->frame_elems * 4u;
    ra.stride = (uint32_t)rp.W + 1u;
    ra.rois = (RoiDev*)e->d_rois.p;
    ra.n_rois = counts + CL::roi(CL::ROI_REGIONS);
    ra.max_rois = max_rois;
    ra.n_frames = (uint32_t)rp.nf;
    ra.frame_w = rp.W;
    ra.frame_h = rp.H;
    ra.win_w0 = rp.second->win_w;
    ra.win_h0 = rp.second->win_h;
    ra.units = (RoiUnit*)e->d_roi_units.p;
    ra.n_units = counts + CL::roi(CL::ROI_UNITS);   // (the slot after it: invalid regions)
    ra.max_units = e->roi_unit_cap;
    ra.ticket = counts + CL::roi(CL::ROI_TICKET);
    ra.det = (RoiDet*)e->d_roi_det.p;
    ra.det_count = counts + CL::roi(CL::ROI_DETS);
    ra.det_cap = e->roi_det_cap;
    if (pl1) {
        ra.det_in = (const DetEntry*)rp.L->d_det.p;
        ra.det_in_count = counts + CL::det_count_u32;
        ra.det_in_cap = rp.L->det_cap;
        ra.scales_in = (const ScaleDev*)pl1->d_scales.p;
    }
    fill_plan_args(e, rp.L, pl2, rp.nf, rp.W, *rp.p_second, ca);   // (pos_mode is 0 on this path: check_params sends the f64 grids through the per-size plans; bound all the same)
    ca.sq_u32 = 0u;   // the region pass reads the u64 squared integral, whatever the lane's batch was integrated as
    ca.gather_waves = (uint32_t)std::min(e->gather_waves_for(rp.nf, pl2->general, pl2->trees), (int)GATHER_WAVES_FULL);   // the region pass keeps full queues
    ca.q_cap = (uint32_t)UNIT_WINDOWS;
    ca.stage_end = pl2->general ? pl2->pass_bounds.back() : (uint32_t)pl2->stages.size();   // stage trees: positions in the sweep order
    ca.gather_pairs = 2u;   // regions are small: thin waves, latency-bound
    ca.sp_tail_max = (uint32_t)std::max(0, std::min(e->sp_tail_max, (int)gather_tail_max(ca.q_cap)));
    ca.stage_entered = (unsigned long long*)(counts + CL::roi(CL::ROI_STAGES));
    ca.tree_ctr = (unsigned long long*)(counts + CL::stage_off_u32) + CL::tree_region_u64;   // the spare array's [2], [3]: the region pass's
    // Regions with large grids at the small scales (many raw candidates, big faces) run those grids on the tile kernel
    // (cascade_tile_roi_pass: tiles of the second cascade's two-per-CU tile scales, laid inside the region): stump cascades
    // whose plan has such tiles.  The caller sizes e->d_roi_tiles and zeroes the eight ticket counters.
    if (e->roi_tile_min_windows > 0 && !pl2->general && !pl2->trees && pl2->wave_tail && pl2->class_first[1] > pl2->class_first[0] &&
        e->roi_tile_cap != 0u) {
        ra.tiles = (RoiTile*)e->d_roi_tiles.p;
        ra.n_tiles = counts + CL::roi(CL::ROI_TILES);
        ra.max_tiles = e->roi_tile_cap;
        ra.tile_min_windows = (uint32_t)e->roi_tile_min_windows;
        ca.tile_lds_bytes = pl2->class_lds[0];
        const int per_cu = std::max(1, std::min(32 / TILE_WAVES, (int)(160u * 1024u / ca.tile_lds_bytes)));
        ra.tile_blocks = (uint32_t)std::max(1, e->n_cu * per_cu);
        ca.tile_ticket = counts + CL::roi_tickets_begin;
        ca.n_pass = 1;                       // the whole cascade inside the tile: survivors are detections
        ca.pass_begin[1] = (uint32_t)pl2->stages.size();
        ca.tile_end = (uint32_t)pl2->stages.size();
        ca.tile_repack_mask = e->tile_repack_mask;
        ca.tile_sp_begin = (uint32_t)e->tile_sp_begin;
        ca.sp_blocks = (const SpBlock*)pl2->d_sp_blocks.p;
        ca.n_sp_blocks = pl2->n_sp_blocks;
        ca.tile_ws_min = (uint32_t)e->tile_ws_min;
        ca.tile_ws_max = (uint32_t)std::min(e->tile_ws_max, (int)TILE_WS_MAX_WINDOWS);
    }
}

// Before the pass, vj_detect_chain: the first cascade (it zeroes the region block and the tile tickets with the counters block), a region's room per detection, the grouping's arguments.
int enqueue_first_cascade(const RegionPass& rp, ChainHandoff& ch) {
    vj_env* e = rp.e;
    Lane* L = rp.L;
    int rc;
    if ((rc = enqueue_cascade(e, L, ch.pl1, rp.W, *ch.p_first))) return rc;
    if ((rc = e->d_rois.ensure((size_t)L->det_cap * sizeof(RoiDev)))) return rc;
    GroupArgs& ga = ch.ga;
    memset(&ga, 0, sizeof(ga));
    if (!ch.grouped) return VJ_OK;
    const size_t nfz = (size_t)rp.nf;
    const GroupLayout g = group_layout(L->det_cap, nfz);
    if ((rc = e->d_group.ensure(g.total))) return rc;
    char* gb = (char*)e->d_group.p;
    ga.det = (const DetEntry*)L->d_det.p;
    ga.det_count = rp.dev_counts() + CL::det_count_u32;
    ga.det_cap = L->det_cap;
    ga.scales = (const ScaleDev*)ch.pl1->d_scales.p;
    ga.frame_bytes = ch.pl1->frame_elems * 4u;
    ga.stride = (uint32_t)rp.W + 1u;
    ga.n_frames = (uint32_t)rp.nf;
    ga.threshold = (int32_t)std::max<uint32_t>(ch.p_first->min_neighbors, 1u);   // clod.cpp:1326
    ga.eps = 0.2;                                                                 // clod.cpp:11
    ga.keys = (uint64_t*)(gb + g.keys);
    ga.grouped = (RoiDev*)(gb + g.grouped);
    ga.frame_count = (uint32_t*)(gb + g.zeroed);
    ga.frame_cursor = ga.frame_count + nfz;
    ga.grouped_count = ga.frame_cursor + nfz;
    ga.overflow = ga.grouped_count + nfz;
    ga.frame_first = (uint32_t*)(gb + g.frame_first);
    ga.grouped_weight = (uint32_t*)(gb + g.grouped_weight);
    ga.roi_weight = (uint32_t*)(gb + g.roi_weight);
    ga.rois = (RoiDev*)e->d_rois.p;
    ga.max_rois = L->det_cap;
    ga.group_max = (uint32_t)e->group_max;
    return VJ_OK;
}

// Run the region pass until the units, detections and region tiles fit their buffers.  chain == null: the caller's regions; else the first cascade runs before every
// attempt and the loop has two more exits: its detections overflowed (both run again), or a frame overflowed the device grouping (REGION_PASS_LEFT: the host route).
enum { REGION_PASS_LEFT = -1 };   // (no VJ_ERR_* code)
int run_region_pass_until_fit(RegionPass& rp, ChainHandoff* chain) {
    vj_env* e = rp.e;
    Lane* L = rp.L;
    int rc;
    if (e->roi_unit_cap == 0) e->roi_unit_cap = 1u << 18;
    if (e->roi_det_cap == 0) e->roi_det_cap = 1u << 16;
    hipEvent_t* ev = &L->launch_ev[2 * VJ_MAX_LAUNCHES - 2];   // the lane's last pair of launch events lies around the pass
    for (int attempt = 0; attempt < 6; ++attempt) {
        if (chain) {
            if ((rc = enqueue_first_cascade(rp, *chain))) return rc;
        } else {   // the caller's regions: the region block, its tile tickets and its tree counters start at zero; the region count goes up
            uint32_t* counts = rp.dev_counts();
            HIP_TRY(hipMemsetAsync(counts + CL::roi_tickets_begin, 0, CL::ticket_range * 4, e->stream));   // tile tickets of the region pass
            HIP_TRY(hipMemsetAsync(counts + CL::roi_off_u32, 0, CL::roi_block_u32 * 4, e->stream));
            HIP_TRY(hipMemsetAsync(counts + CL::tree_region_u32, 0, CL::tree_pair_bytes, e->stream));   // the region pass's tree counters
            HIP_TRY(hipMemcpyAsync(counts + CL::roi(CL::ROI_REGIONS), &rp.n_reg, 4, hipMemcpyHostToDevice, e->stream));
        }
        if ((rc = e->d_roi_units.ensure((size_t)e->roi_unit_cap * sizeof(RoiUnit)))) return rc;
        if ((rc = e->d_roi_det.ensure((size_t)e->roi_det_cap * sizeof(RoiDet)))) return rc;
        if (e->roi_tile_cap == 0) e->roi_tile_cap = 1u << 16;
        if ((rc = e->d_roi_tiles.ensure((size_t)e->roi_tile_cap * sizeof(RoiTile)))) return rc;
        RoiArgs ra;
        CascadeArgs ca;
        fill_region_args(rp, chain ? L->det_cap : rp.n_reg, chain ? chain->pl1 : nullptr, ra, ca);
        HIP_TRY(hipEventRecord(ev[0], e->stream));
        if (chain && chain->grouped) {
            chain->ga.n_rois = ra.n_rois;
            const int grc = launch_group_rois(chain->ga, e->stream);
            if (grc) {
                set_error("grouping launch failed: %s", hipGetErrorString((hipError_t)grc));
                return VJ_ERR_HIP;
            }
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CL::roi(CL::ROI_GROUP_OVERFLOW), chain->ga.overflow, 4, hipMemcpyDeviceToHost, e->stream));
        }
        const int hrc = launch_roi_chain(ra, ca, chain && !chain->grouped, rp.pl2->trees, (rp.p_second->flags & VJ_FLAG_COUNTERS) != 0, rp.pl2->general,
                                         std::max(1, e->n_cu * e->blocks_per_cu), e->stream, e->concurrent ? e->stream2 : nullptr, e->fork_ev, e->join_ev);
        if (hrc) {
            set_error("region pass launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
        HIP_TRY(hipEventRecord(ev[1], e->stream));
        if (chain) {   // the region counters join the block enqueue_cascade already copies; copy them again now that they are final
            if ((rc = rp.copy_counts(CL::roi_off_u32, CL::roi_head_u32 * 4))) return rc;
            if ((rc = rp.copy_counts(CL::roi(CL::ROI_TILES), 4))) return rc;   // region tiles
            if ((rc = rp.copy_counts(CL::roi(CL::ROI_STAGES), (size_t)VJ_MAX_STAGES * 2 * 4))) return rc;
        } else if ((rc = rp.copy_counts(CL::roi_off_u32, CL::roi_block_u32 * 4))) {
            return rc;
        }
        if ((rc = rp.copy_counts(CL::tree_region_u32, CL::tree_pair_bytes))) return rc;
        HIP_TRY(hipEventRecord(L->done, e->stream));
        HIP_TRY(hipEventSynchronize(L->done));
        const uint32_t* hc = rp.host_counts();
        const uint32_t n_units = hc[CL::roi(CL::ROI_UNITS)], n_tiles2 = hc[CL::roi(CL::ROI_TILES)], n_det1 = hc[CL::det_count_u32];
        rp.n_det2 = hc[CL::roi(CL::ROI_DETS)];
        if (hc[CL::roi(CL::ROI_INVALID)] != 0) {
            set_error("internal error: %u regions outside their frames", hc[CL::roi(CL::ROI_INVALID)]);
            return VJ_ERR_HIP;
        }
        if (chain && n_det1 > L->det_cap) {   // as finish_batch would: grow, and run both cascades again
            const uint32_t want = grown_cap(L->det_cap, n_det1);
            if ((rc = L->d_det.ensure((size_t)want * sizeof(DetEntry)))) return rc;
            L->det_cap = want;
            continue;
        }
        if (chain && chain->grouped && hc[CL::roi(CL::ROI_GROUP_OVERFLOW)] != 0) return REGION_PASS_LEFT;   // a frame with more raw candidates than the device kernel groups
        if (n_units > e->roi_unit_cap || rp.n_det2 > e->roi_det_cap || n_tiles2 > e->roi_tile_cap) {
            e->roi_unit_cap = grown_cap(e->roi_unit_cap, n_units);
            e->roi_det_cap = grown_cap(e->roi_det_cap, rp.n_det2);
            e->roi_tile_cap = grown_cap(e->roi_tile_cap, n_tiles2);
            continue;
        }
        HIP_TRY(hipEventElapsedTime(&rp.ms, ev[0], ev[1]));
        return VJ_OK;
    }
    set_error("region buffers kept overflowing");
    return VJ_ERR_LIMIT;
}

// The pass's detections as the device left them, and appended to dets2 (`frame`: the region): origin_of(region) -> RawDet{its number in the result, 0, its x, its y}.
int read_region_dets(const RegionPass& rp, std::vector<RoiDet>* raw2) {
    raw2->resize(rp.n_det2);
    if (rp.n_det2) HIP_TRY(hipMemcpy(raw2->data(), rp.e->d_roi_det.p, (size_t)rp.n_det2 * sizeof(RoiDet), hipMemcpyDeviceToHost));
    return VJ_OK;
}
template <class OriginOf>
void decode_region_dets(const RegionPass& rp, const std::vector<RoiDet>& raw2, OriginOf origin_of, std::vector<RawDet>* dets2) {
    for (const RoiDet& d : raw2) {
        const WindowAt at = decode_window(d.off, rp.pl2->frame_elems, (uint32_t)rp.W + 1u);
        const RawDet o = origin_of(d.roi);
        dets2->push_back(RawDet{o.frame, d.slot, at.x - o.x, at.y - o.y});
    }
}

// Counted calls: the pass's stage_entered array, and its visited child nodes / rectangles parked as finish_batch parks them.
void add_region_counters(const RegionPass& rp, vj_counters* k) {
    if (!(rp.p_second->flags & VJ_FLAG_COUNTERS)) return;
    const unsigned long long* se = (const unsigned long long*)(rp.host_counts() + CL::roi(CL::ROI_STAGES));
    const unsigned long long* tc = (const unsigned long long*)(rp.host_counts() + CL::stage_off_u32) + CL::tree_region_u64;
    k->stump_evals += tc[0];
    k->gather_bytes += tc[1];
    for (size_t s2 = 0; s2 < rp.pl2->stages.size(); ++s2) k->stage_entered[s2] += se[s2];
}

// The region pass's plan: its scale records go to the device with a queue layout (none is used by the region pass).
int upload_scale_records(Plan* pl2) {
    uint64_t dummy = 0;
    return pl2->frames_q == 0 ? layout_queues(pl2, 1, &dummy) : VJ_OK;
}

// vj_detect_rois on frames of one size with a linear cascade: one integral per frame and ONE region pass for regions of
// any sizes (the machinery of vj_detect_chain's second half, the region list uploaded instead of built on the device) —
// not one plan and one vj_detect call per distinct region size.
int detect_rois_on_device(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                          const vj_params* p, int W, int H, vj_result* out) {
    int rc;
    Plan* pl2;
    if ((rc = get_plan(e, c, W, H, *p, &pl2))) return rc;
    uint64_t max_frames;
    if ((rc = subbatch_frames(e, pl2, nullptr, &max_frames))) return rc;
    if ((rc = upload_scale_records(pl2))) return rc;
    Lane* L = &e->lane0;
    std::vector<RawDet> dets2;
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        std::vector<RoiDev> regions;
        std::vector<int> index;   // position in `regions` -> the caller's region
        for (int i = 0; i < n_rois; ++i)
            if (rois[i].frame >= f0 && rois[i].frame < f0 + nf) {
                regions.push_back(RoiDev{rois[i].frame - f0, rois[i].x, rois[i].y, rois[i].w, rois[i].h});
                index.push_back(i);
            }
        if (regions.empty()) continue;
        if ((rc = enqueue_prepare(e, L, pl2, frames + f0, nf, W, H, false, nullptr))) return rc;
        RegionPass rp{e, L, pl2, c, p, W, H, nf, (uint32_t)regions.size()};
        if ((rc = e->d_rois.ensure((size_t)rp.n_reg * sizeof(RoiDev)))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_rois.p, regions.data(), (size_t)rp.n_reg * sizeof(RoiDev), hipMemcpyHostToDevice, e->stream));
        if ((rc = run_region_pass_until_fit(rp, nullptr))) return rc;
        float ms_i = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, L->ev[0], L->ev[1]));
        out->timing.integral_ms += ms_i;
        out->timing.cascade_ms += rp.ms;
        out->timing.total_ms += ms_i + rp.ms;
        out->timing.n_cascade_launches = 1;
        std::vector<RoiDet> raw2;
        if ((rc = read_region_dets(rp, &raw2))) return rc;
        decode_region_dets(rp, raw2, [&](uint32_t r) { return RawDet{index[r], 0, (uint32_t)regions[r].x, (uint32_t)regions[r].y}; }, &dets2);
        add_region_counters(rp, &out->counters);
    }
    return build_result(pl2, dets2, out->counters.stage_entered[0], *p, out);   // (the windows of a region pass: the ones that entered stage 0)
}

std::vector<vj_roi> detections_as_rois(const vj_result& r) {
    std::vector<vj_roi> rois(r.count);
    for (uint32_t i = 0; i < r.count; ++i) rois[i] = vj_roi{(int32_t)r.rects[i].frame, r.rects[i].x, r.rects[i].y, r.rects[i].w, r.rects[i].h};
    return rois;
}

// The chain the long way round: the first cascade as vj_detect runs (and groups) it, its result handed back as a region list.
// Whatever earlier sub-batches left in the two results is dropped first: no regions is an empty, zeroed second result.
int chain_through_host(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames, int n_frames,
                       const vj_params* p_first, const vj_params* p_second, vj_result* out_first, vj_result* out_second) {
    vj_result_free(out_first);
    vj_result_free(out_second);
    memset(out_second, 0, sizeof(*out_second));
    if (const int rc = vj_detect(e, first, frames, n_frames, p_first, out_first)) return rc;
    const std::vector<vj_roi> regions = detections_as_rois(*out_first);
    if (regions.empty()) return VJ_OK;
    return vj_detect_rois(e, second, frames, n_frames, regions.data(), (int)regions.size(), p_second, out_second);
}

}  // namespace

extern "C" {

// Second cascade on regions of interest (config 5: eyes inside faces).  A ROI is a view —
// pointer + stride — into its frame, as the reference's callers would pass a sub-image header; detection windows
// come in few distinct sizes, so the ROIs are grouped by size and every group is ONE batched vj_detect pass.
int vj_detect_rois(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                   const vj_params* p, vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || n_rois < 0 || (n_rois > 0 && (!frames || !rois))) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (refuse_equalize(p->flags, "vj_detect_rois")) return VJ_ERR_UNSUPPORTED;
    if (const int prc = check_params(*p)) return prc;
    std::map<std::pair<int, int>, std::vector<int>> by_size;   // (w, h) -> ROI indices
    for (int i = 0; i < n_rois; ++i) {
        const vj_roi& r = rois[i];
        if (r.frame < 0 || r.frame >= n_frames || !frames[r.frame].data || r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 ||
            r.x + r.w > frames[r.frame].width || r.y + r.h > frames[r.frame].height) {
            set_error("roi %d lies outside its frame", i);
            return VJ_ERR_ARG;
        }
        by_size[{r.w, r.h}].push_back(i);
    }
    // frames of one size, a linear cascade, the exhaustive grid: every region in one pass on the frames' own integral images
    // (a scale mask selects among the plan's scales; every region still enumerates its own prefix of them)
    if (n_rois > 0 && n_frames > 0 && !(p->flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW)) && p->scale_factor > 1.0f && e->rois_on_device) {
        bool same = true;
        for (int i = 0; i < n_frames && same; ++i)
            same = frames[i].data && frames[i].width == frames[0].width && frames[i].height == frames[0].height &&
                   image_channels(frames[i]) == image_channels(frames[0]) && frames[i].stride >= frames[i].width * image_channels(frames[i]);
        int W = 0, H = 0, CH = 0;
        if (same && check_frames(frames, n_frames, &W, &H, &CH) == VJ_OK) {
            HIP_TRY(hipSetDevice(e->device));
            return detect_rois_on_device(e, c, frames, n_frames, rois, n_rois, p, W, H, out);
        }
    }
    std::vector<vj_rect> all;
    for (const auto& kv : by_size) {
        std::vector<vj_image> views;
        int ch0 = -1;
        for (int i : kv.second) {
            const vj_roi& r = rois[i];
            const vj_image& f = frames[r.frame];
            const int ch = image_channels(f);
            if (ch0 < 0) ch0 = ch;
            if (ch != ch0) {
                set_error("ROIs of one size must come from frames with the same channel count");
                return VJ_ERR_ARG;
            }
            views.push_back(vj_image{f.data + (size_t)r.y * (size_t)f.stride + (size_t)r.x * (size_t)ch, r.w, r.h, f.stride,
                                     f.on_device, f.channels});
        }
        vj_result part;
        int rc = vj_detect(e, c, views.data(), (int)views.size(), p, &part);
        if (rc) {
            vj_result_free(&part);
            return rc;
        }
        for (uint32_t k = 0; k < part.count; ++k) {
            vj_rect rr = part.rects[k];
            rr.frame = kv.second[(size_t)rr.frame];   // index in the batch -> ROI index
            all.push_back(rr);
        }
        // counters and times add up over the groups
        out->counters.windows += part.counters.windows;
        out->counters.stump_evals += part.counters.stump_evals;
        out->counters.gather_bytes += part.counters.gather_bytes;
        for (int s2 = 0; s2 < VJ_MAX_STAGES; ++s2) out->counters.stage_entered[s2] += part.counters.stage_entered[s2];
        out->timing.integral_ms += part.timing.integral_ms;
        out->timing.cascade_ms += part.timing.cascade_ms;
        out->timing.total_ms += part.timing.total_ms;
        vj_result_free(&part);
    }
    std::stable_sort(all.begin(), all.end(), [](const vj_rect& a, const vj_rect& b) { return a.frame < b.frame; });
    return rects_to_result(all, out);
}

// ------------------------------------------------------------------ two cascades, hand-off on the device
int vj_detect_chain(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames, int n_frames,
                    const vj_params* p_first, const vj_params* p_second, vj_result* out_first, vj_result* out_second) {
    if (!e || !first || !second || !p_first || !p_second || !out_first || !out_second || n_frames < 0 || (n_frames > 0 && !frames))
        return VJ_ERR_ARG;
    memset(out_first, 0, sizeof(*out_first));
    memset(out_second, 0, sizeof(*out_second));
    if (refuse_equalize(p_first->flags | p_second->flags, "vj_detect_chain")) return VJ_ERR_UNSUPPORTED;
    if (n_frames == 0) return VJ_OK;
    for (const vj_params* pp : {p_first, p_second})
        if (const int prc = check_params(*pp)) return prc;
    // the CPU variants' skip rules make a window's fate depend on its row's history inside ITS image: the first cascade runs
    // as vj_detect does, the second one per region size on the sub-images (vj_detect_rois' path for these modes) — the
    // hand-off goes through the host, the results are the ones the definition above gives
    if ((p_first->flags | p_second->flags) & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW))
        return chain_through_host(e, first, second, frames, n_frames, p_first, p_second, out_first, out_second);
    const bool grouped = p_first->min_neighbors != 0;   // the regions are the GROUPED candidates (grouped on the device)
    int W, H, CH;
    int rc = check_frames(frames, n_frames, &W, &H, &CH);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    Plan *pl1, *pl2;
    // (the first cascade's chain balance is found by feedback as in vj_detect: its kernels run before the region pass starts)
    vj_env::Balance* bal = balance_of(e, first, W, H, *p_first, n_frames, true);
    if (bal) balance_touch(bal, n_frames);
    if ((rc = get_plan(e, first, W, H, *p_first, &pl1, n_frames))) return rc;
    // the second cascade is planned for the frame's stride and every scale a region as large as the frame could use;
    // each region picks its own scales and grid on the device
    if ((rc = get_plan(e, second, W, H, *p_second, &pl2))) return rc;
    if ((rc = get_plan(e, first, W, H, *p_first, &pl1, n_frames))) return rc;   // (the cache may have evicted it for pl2: look it up again)
    uint64_t max_frames;
    if ((rc = subbatch_frames(e, pl1, pl2, &max_frames))) return rc;
    if ((rc = upload_scale_records(pl2))) return rc;
    Lane* L = &e->lane0;
    std::vector<RawDet> dets1;
    std::vector<vj_rect> grouped1;       // grouped mode: the first result, as the device grouped it
    std::vector<RawDet> dets2;             // (frame: the region's position in dets1 / grouped1 until the result step ranks it)
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        if ((rc = enqueue_prepare(e, L, pl1, frames + f0, nf, W, H, false, nullptr))) return rc;
        ChainHandoff chain{pl1, p_first, grouped};
        RegionPass rp{e, L, pl2, second, p_second, W, H, nf, 0u};
        rc = run_region_pass_until_fit(rp, &chain);
        // a frame overflowed the device grouping: the same result the long way round (group on the host, hand the regions back as a list)
        if (rc == REGION_PASS_LEFT) return chain_through_host(e, first, second, frames, n_frames, p_first, p_second, out_first, out_second);
        if (rc) return rc;
        // first cascade: decode (finish_batch appends in the device's order: a region's number is its detection's place in it)
        const size_t base1 = dets1.size(), base_g = grouped1.size();
        if ((rc = finish_batch(e, L, pl1, f0, W, H, *p_first, &dets1, &out_first->counters, &out_first->timing))) return rc;
        std::vector<RoiDet> raw2;
        if ((rc = read_region_dets(rp, &raw2))) return rc;
        if (grouped) {   // the first result is the region list itself
            const uint32_t n_rois = rp.host_counts()[CL::roi(CL::ROI_REGIONS)];
            std::vector<RoiDev> regions(n_rois);
            std::vector<uint32_t> weights(n_rois);
            if (n_rois) {
                HIP_TRY(hipMemcpy(regions.data(), e->d_rois.p, (size_t)n_rois * sizeof(RoiDev), hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(weights.data(), (const char*)e->d_group.p + group_layout(L->det_cap, (size_t)nf).roi_weight, (size_t)n_rois * 4u, hipMemcpyDeviceToHost));
            }
            for (uint32_t i = 0; i < n_rois; ++i)
                grouped1.push_back(vj_rect{regions[i].x, regions[i].y, regions[i].w, regions[i].h, (float)weights[i], regions[i].frame + f0, -1});
            decode_region_dets(rp, raw2, [&](uint32_t r) { return RawDet{(int)(base_g + r), 0, (uint32_t)regions[r].x, (uint32_t)regions[r].y}; }, &dets2);
        } else {
            decode_region_dets(rp, raw2, [&](uint32_t r) { return RawDet{(int)(base1 + r), 0, dets1[base1 + r].x, dets1[base1 + r].y}; }, &dets2);
        }
        out_second->timing.cascade_ms += rp.ms;
        out_second->timing.total_ms += rp.ms;
        out_second->timing.n_cascade_launches = 1;
        add_region_counters(rp, &out_second->counters);
    }
    balance_feedback(bal, e, pl1, *p_first, n_frames, max_frames, &out_first->timing);
    // the first result in its sorted order; regions are numbered by their position in it
    if (grouped) {   // frames in order, groups in cv::partition's class order: already the result's order
        if ((rc = rects_to_result(grouped1, out_first))) return rc;
        fill_counters(pl1, pl1->windows_per_frame * (uint64_t)n_frames, *p_first, &out_first->counters);
    } else {
        std::vector<uint32_t> order(dets1.size()), rank(dets1.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return std::tie(dets1[a].frame, dets1[a].slot, dets1[a].y, dets1[a].x) < std::tie(dets1[b].frame, dets1[b].slot, dets1[b].y, dets1[b].x);
        });
        for (size_t i = 0; i < order.size(); ++i) rank[order[i]] = (uint32_t)i;
        for (RawDet& d : dets2) d.frame = (int)rank[(size_t)d.frame];
        if ((rc = build_result(pl1, dets1, pl1->windows_per_frame * (uint64_t)n_frames, *p_first, out_first))) return rc;
    }
    return build_result(pl2, dets2, out_second->counters.stage_entered[0], *p_second, out_second);
}

}  // extern "C"
