// The launch sequence of one vj_detect call, blocking or through a vj_stream.  It replaces clodDetectObjectsOpenCL (clod.cpp:1176-1336): where the reference does, per frame, one blocking launch
// + count read-back per (scale, stage) — up to 924 round trips at 1080p — this driver enqueues 3 integral launches and a handful of cascade passes for the WHOLE batch and synchronises once.
#include "vj_env_internal.hpp"

#include <cstdio>
#include <cstdlib>

using namespace vj;

namespace vj {

int ensure_queues(vj_env* e, Plan* pl, int frames) {
    uint64_t q_entries = 0;
    if (const int rc = layout_queues(pl, frames, &q_entries)) return rc;
    const size_t n_pass = pl->pass_bounds.size() - 1;
    for (size_t ps = 1; ps < n_pass; ++ps)
        if (const int rc = e->d_q[ps].ensure(std::max<uint64_t>(q_entries, 1) * sizeof(QEntry))) return rc;
    return VJ_OK;
}

int enqueue_prepare(vj_env* e, Lane* L, Plan* pl, const vj_image* frames, int nf, int W, int H, bool fixed_queue_layout,
                    hipStream_t copy_stream, bool equalize, bool sq_u32) {
    int rc;
    int channels = image_channels(frames[0]);
    if ((rc = ensure_image_buffers(e, W, H, nf, true, channels, L))) return rc;
    if (!fixed_queue_layout && (rc = ensure_queues(e, pl, nf))) return rc;
    if ((rc = L->d_counts.ensure(CountsLayout::bytes))) return rc;
    if (L->det_cap == 0) {
        L->det_cap = e->det_cap_init;
        if ((rc = L->d_det.ensure((size_t)L->det_cap * sizeof(DetEntry)))) return rc;
    }
    const uint8_t* d_gray;
    size_t gray_frame_bytes;
    int gray_stride;
    if ((rc = stage_frames(e, frames, nf, W, H, &d_gray, &gray_frame_bytes, &gray_stride, L, copy_stream))) return rc;
    if (copy_stream) {
        HIP_TRY(hipEventRecord(L->upload_done, copy_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, L->upload_done, 0));
    }
    HIP_TRY(hipEventRecord(L->ev[0], e->stream));
    // VJ_FLAG_EQUALIZE_HIST: from here on the batch is the lane's equalized gray frames (a redo integrates those again)
    if (equalize && (rc = enqueue_equalize(e, L, &d_gray, &gray_frame_bytes, &gray_stride, &channels, W, H, nf))) return rc;
    L->src_gray = d_gray;
    L->src_frame_bytes = gray_frame_bytes;
    L->src_stride = gray_stride;
    L->src_channels = channels;
    // (a variance rectangle wider than SQ32_MAX_AREA pixels has no strip height: such frames keep the u64 layout)
    L->sq_u32 = sq_u32 && e->sq32 && e->sq_u32 && (uint32_t)W <= SQ32_MAX_AREA;
    if ((rc = enqueue_integral(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, channels, L->sq_u32))) return rc;
    HIP_TRY(hipEventRecord(L->ev[1], e->stream));
    HIP_TRY(hipEventRecord(L->integral_done, e->stream));   // the lane's frame buffer may be overwritten from here on
    L->nf = nf;
    return VJ_OK;
}

void fill_plan_args(const vj_env* e, const Lane* L, const Plan* pl, int nf, int W, const vj_params& p, CascadeArgs& ca) {
    memset(&ca, 0, sizeof(ca));
    ca.sum = (const uint32_t*)e->d_sum.p;
    ca.sqsum = (const uint64_t*)e->d_sqsum.p;
    ca.sq_u32 = L->sq_u32 ? 1u : 0u;
    ca.table = (const uint32_t*)pl->d_table.p;
    ca.scales = (const ScaleDev*)pl->d_scales.p;
    ca.stages = (const StageDev*)pl->d_stages.p;
    ca.n_frames = (uint32_t)nf;
    ca.n_scales = (uint32_t)pl->scales.size();
    ca.frame_elems = pl->frame_elems;
    ca.sum_bytes = (uint32_t)((uint64_t)pl->frame_elems * 4u * (uint64_t)nf);
    ca.stride = (uint32_t)W + 1u;
    ca.signed_mean = (p.flags & VJ_FLAG_SIGNED_MEAN) ? 1u : 0u;
    ca.identity_order = pl->general ? 0u : 1u;
    ca.pos_mode = pl->pos_mode;
    ca.pos_tab = (const uint32_t*)pl->d_pos_tab.p;
    ca.max_stage_nodes = pl->max_stage_nodes;
}

namespace {

// The launch bookkeeping of one enqueue_cascade: every launch lies between its own pair of events on its stream, is described in the lane's list and counts into its own stage array.
struct LaunchLog {
    Lane* L;
    const Plan* pl;
    unsigned long long* stage_arrays;   // the block's stage arrays on the device (array 0 is spare)

    int begin(int kind, int cls, uint32_t sb, uint32_t se, uint32_t lds, hipStream_t st) {
        std::vector<vj_launch>& linfo = L->linfo;
        if (linfo.size() < VJ_MAX_LAUNCHES) HIP_TRY(hipEventRecord(L->launch_ev[2 * linfo.size()], st));
        vj_launch li = {};
        li.kind = kind, li.lds_class = cls, li.stage_begin = (int32_t)sb, li.stage_end = (int32_t)se, li.lds_bytes = lds;
        for (uint32_t slot = 0; slot < pl->scales.size(); ++slot) {
            const ScaleDev& sd = pl->scales[slot];
            const bool in = kind == VJ_LAUNCH_QUEUE ||
                            (kind == VJ_LAUNCH_TILE && sd.tile_rw && sd.tile_row_end > 0 && (int)pl->scales[pl->tile_lead[slot]].tile_class == cls) ||
                            (kind == VJ_LAUNCH_GRID && sd.tile_row_end < sd.ny);
            if (in && sd.scale_idx < 128) li.scale_mask[sd.scale_idx >> 6] |= 1ull << (sd.scale_idx & 63);
        }
        linfo.push_back(li);
        return VJ_OK;
    }
    // the launch just begun counts into its own array
    unsigned long long* counters() const { return stage_arrays + std::min<size_t>(L->linfo.size(), VJ_MAX_LAUNCHES) * VJ_MAX_STAGES; }
    int end(hipStream_t st) {
        if (L->linfo.size() <= VJ_MAX_LAUNCHES) HIP_TRY(hipEventRecord(L->launch_ev[2 * L->linfo.size() - 1], st));
        return VJ_OK;
    }
};

// One enqueue_cascade in progress: what its steps share, and the steps in the order they run.
struct CascadeRun {
    vj_env* const e;
    Lane* const L;
    Plan* const pl;
    const int W;
    const vj_params& p;
    const int nf = L->nf;
    const size_t n_pass = pl->pass_bounds.size() - 1;
    const bool count = (p.flags & VJ_FLAG_COUNTERS) != 0;
    const int n_blocks = std::max(1, e->n_cu * e->blocks_per_cu);   // workgroups of a gather launch that has the device to itself
    LaunchLog log{L, pl, (unsigned long long*)((uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32)};
    CascadeArgs ca = {};   // the base arguments every launch starts from (the steps below run in this order only: each fills what the next reads)
    bool banded = false, general_kernel = false;
    PassSchedule sch = {};
    hipStream_t sB = nullptr;   // chain B's stream ...
    int b_blocks = 0;           // ... and its workgroups

    uint32_t* qcount(int set, size_t ps) const { return (uint32_t*)L->d_counts.p + (set ? CountsLayout::q2_off_u32 : 0) + ps * CountsLayout::q_counts; }   // (set 1: the tiles' own)
    bool pass_is_last(size_t ps) const { return pl->seg_last.empty() ? ps + 1 == n_pass : pl->seg_last[ps] != 0; }

    // 1. the counters block starts at zero (the tickets and the region block with it)
    int zero_counters() {
        HIP_TRY(hipMemsetAsync(L->d_counts.p, 0, CountsLayout::bytes, e->stream));
        HIP_TRY(hipEventRecord(L->ev[2], e->stream));
        return VJ_OK;
    }
    // 2. the arguments every launch of the batch shares
    void fill_base_args() {
        fill_plan_args(e, L, pl, nf, W, p, ca);
        ca.units = (const UnitDev*)pl->d_units.p;
        ca.n_units = (uint32_t)pl->units.size();
        ca.tile_units = (const UnitDev*)pl->d_tile_units.p;
        ca.n_tile_units = (uint32_t)pl->tile_units.size();
        // waves per workgroup of the gather chain: four for batches, three for single frames and for stage trees (their
        // workgroups carry a second LDS array); the launchers clamp, the kernels read blockDim.  The waves of a linear launch
        // divide one 16 KiB array (vj_gather_queue.hpp), and the plan's units must fit a wave's share: a plan cut for fewer
        // waves than this call would run (a stream's plan, a sub-batch) keeps the call at the waves it was cut for
        ca.gather_waves = gather_waves_fitting((uint32_t)e->gather_waves_for(nf, pl->general, pl->trees), pl->unit_cap);
        ca.q_cap = pl->general ? (uint32_t)UNIT_WINDOWS : gather_queue_cap(ca.gather_waves);
        ca.total_waves = (uint32_t)n_blocks * ca.gather_waves;
        ca.det = (DetEntry*)L->d_det.p;
        ca.det_count = (uint32_t*)L->d_counts.p + CountsLayout::det_count_u32;
        ca.det_cap = L->det_cap;
        ca.stage_entered = log.stage_arrays;
        ca.tree_ctr = log.stage_arrays + CountsLayout::tree_first_u64;   // array 0 is spare: the first cascade's visited child nodes / their rectangles
        ca.n_pass = (uint32_t)n_pass;
        for (size_t ps = 0; ps <= n_pass; ++ps) ca.pass_begin[ps] = pl->pass_bounds[ps];
        for (size_t ps = 1; ps < n_pass; ++ps) {
            ca.q_pass[ps] = (QEntry*)e->d_q[ps].p;
            ca.q_pass_count[ps] = qcount(0, ps);
        }
        // linear cascades: the kernel sees the configured tile_end, not the plan's clamped pl->tile_end; a tile leaves at the first pass boundary
        // at or beyond it, and `banded` / `handover` (compute_schedule) compare it with pass_bounds[1]
        ca.tile_end = pl->general ? pl->general_prefix : (uint32_t)e->tile_end;   // stage trees: tiles run the linear prefix only
        ca.tile_min_lanes = (uint32_t)e->tile_min_lanes;
        ca.tile_repack_mask = e->tile_repack_mask;
        ca.tile_sp_begin = (!pl->general && (pl->wave_tail || pl->tree2)) ? (uint32_t)e->tile_sp_begin : 0xffffffffu;   // the finishes walk positions linearly: never on a stage tree
        ca.tree2 = pl->tree2 ? 1u : 0u;
        ca.n_seg = e->tile_segments ? pl->tile_n_seg : 0u;
        for (int k = 0; k < 4; ++k) ca.seg_end[k] = pl->tile_seg_end[k];
        ca.seg_chain = pl->tile_seg_chain;
        ca.sp_blocks = (const SpBlock*)pl->d_sp_blocks.p;
        ca.n_sp_blocks = pl->n_sp_blocks;
        ca.tile_ws_min = pl->wave_tail ? (uint32_t)e->tile_ws_min : 0u;   // no wave-independent tail: wave-split to the end
        ca.tile_ws_max = (uint32_t)std::min(e->tile_ws_max, (int)TILE_WS_MAX_WINDOWS);
        ca.gather_pairs = e->pairs_for(nf);
        ca.sp_tail_max = (uint32_t)std::max(0, std::min(e->sp_tail_max, (int)gather_tail_max(ca.q_cap)));
    }
    // 3. P2 skip modes: the windows the reference's sequential CPU loop visits, as a bitmap: stage-0 verdict of every grid window,
    // then the parity recurrence; the passes drop the unvisited windows while they enumerate the grid
    int skip_bitmap() {
        if (!pl->skip_mode || !pl->n_skip_units) return VJ_OK;
        if (const int rc = e->d_skip_bits.ensure((size_t)pl->skip_frame_words * 8u * (size_t)nf)) return rc;
        ca.skip_bits = (unsigned long long*)e->d_skip_bits.p;
        ca.skip_frame_words = pl->skip_frame_words;
        ca.skip_units = (const UnitDev*)pl->d_skip_units.p;
        ca.n_skip_units = pl->n_skip_units;
        ca.skip_segs = (const UnitDev*)pl->d_skip_segs.p;
        ca.n_skip_segs = pl->n_skip_segs;
        const int hrc = launch_skip_bitmap(ca, pl->trees, std::max(1, e->n_cu * 4), e->stream);
        if (hrc) {
            set_error("skip bitmap launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
        return VJ_OK;
    }
    // 4. which passes run on which chain (pass_schedule, vj_detect_host.hpp), and the buffers the choice needs
    int compute_schedule() {
        general_kernel = pl->general && pl->seg_last.empty();   // run_stages_general finishes the tree
        // Band-major queue pass: a batch of a linear cascade whose gather chain is grid pass + ONE queue pass that only the grid
        // pass feeds.  It reads nothing but the runs the grid pass records in run_table, so the tiles must not feed that queue:
        // they run the whole cascade themselves only when tile_end lies BEYOND the boundary (at tile_end == pass_bounds[1] they
        // hand their survivors to q_pass[1], and the chunked pass, which sweeps the whole sub-queue, takes the batch)
        banded = e->q_band_px > 0 && !pl->unit_groups.empty() && !pl->general && n_pass == 2 && nf >= e->q_band_min_frames &&
                 e->tile_min_lanes == 0 && (uint32_t)e->tile_end > pl->pass_bounds[1];
        if (banded) {
            if (const int rc = e->d_run_table.ensure((size_t)nf * pl->units.size() * 8u)) return rc;
            ca.run_table = (uint32_t*)e->d_run_table.p;
        }
        sch = pass_schedule(pl->pass_bounds, (uint32_t)e->tile_end, pl->general, pl->general_prefix, e->tile_min_lanes, ca.n_units, ca.n_tile_units,
                            e->concurrent != 0, e->tree_split_queues, pl->seg_last.empty());
        for (size_t ps = 1; ps < n_pass && sch.split_sets; ++ps) {
            if (const int rc = e->d_q2[ps].ensure(e->d_q[ps].cap)) return rc;
            ca.q_pass[ps] = (QEntry*)e->d_q2[ps].p;        // (the grid and queue passes take theirs from queue_args)
            ca.q_pass_count[ps] = qcount(1, ps);
        }
        sB = sch.two_streams ? e->stream2 : e->stream;
        // chain B next to the tiles: one small workgroup per CU (the texture-address unit it is bound by saturates at
        // one wave per SIMD), so that the tile workgroups find their LDS share next to it
        b_blocks = sch.two_streams ? std::max(1, e->n_cu * e->concurrent_blocks_per_cu) : n_blocks;
        return VJ_OK;
    }
    // The arguments of gather pass ps on queue set `set`: pass ps reads queue ps (filled by pass ps-1 and by tiles that left at
    // this boundary) and appends its survivors to queue ps+1
    CascadeArgs queue_args(size_t ps, int set = 0) const {
        CascadeArgs qa = ca;
        const DevBuf* dq = set ? e->d_q2 : e->d_q;
        qa.stage_begin = pl->pass_bounds[ps];
        qa.stage_end = pl->pass_bounds[ps + 1];
        const bool last = pass_is_last(ps);
        qa.q_in = (const QEntry*)dq[ps].p;
        qa.q_in_count = qcount(set, ps);
        qa.q_ticket = qcount(set, 0) + ps * Q_PARTS;   // queue 0 does not exist: its counters serve as tickets
        // frame-major order inside a part: one slice per frame of the part's frame group (-1), or as configured
        qa.q_slices = e->q_slices >= 0 ? (uint32_t)std::max(1, e->q_slices)
                                       : (uint32_t)std::max(1, std::min(16, (nf + (int)Q_PARTS - 1) / (int)Q_PARTS));
        qa.min_chunk = (uint32_t)e->min_chunk;
        qa.wide_tail = (e->wide_tail < 0 ? nf <= 4 : e->wide_tail != 0) ? 1u : 0u;
        qa.q_out = last ? nullptr : (QEntry*)dq[ps + 1].p;
        qa.q_out_count = last ? nullptr : qcount(set, ps + 1);
        if (banded && ps == 1) {
            qa.q_groups = (const UnitDev*)pl->d_unit_groups.p;
            qa.n_q_groups = (uint32_t)pl->unit_groups.size();
        }
        if (!pl->seg_fail.empty() && pl->seg_fail[ps] != 0) {   // stage tree: this segment's rejects continue
            qa.q_fail = (QEntry*)dq[pl->seg_fail[ps]].p;
            qa.q_fail_count = qcount(set, pl->seg_fail[ps]);
        }
        return qa;
    }
    // A failed launch is the call's error at once.  After the fork that leaves stream2 un-joined: it waits for the fork event and
    // nothing waits for it, and the next call's fork orders it behind the environment's stream again.
    static int launched(int hrc) {
        if (hrc) set_error("cascade launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return hrc ? VJ_ERR_HIP : VJ_OK;
    }
    // One gather launch (the grid pass or a queue pass) with its bookkeeping.
    int launch_gather(CascadeArgs& a, int kind, bool last, bool general, int blocks, hipStream_t st) {
        if (const int rc = log.begin(kind, 0, a.stage_begin, a.stage_end, 0, st)) return rc;
        a.stage_entered = log.counters();
        const int hrc = launch_cascade_pass(a, kind == VJ_LAUNCH_GRID, pl->trees, last, count, general, blocks, st);
        if (const int rc = log.end(st)) return rc;
        return launched(hrc);
    }
    // 5. chain B starts where chain A stands
    int fork_chains() {
        if (sch.two_streams) {
            HIP_TRY(hipEventRecord(e->fork_ev, e->stream));
            HIP_TRY(hipStreamWaitEvent(e->stream2, e->fork_ev, 0));
        }
        HIP_TRY(hipEventRecord(L->pass_ev[0], e->stream));
        return VJ_OK;
    }
    // 6. chain A: the tile launches, one per LDS class
    int tile_chain() {
        for (uint32_t ci = 0; ci < TILE_CLASSES && ca.n_tile_units > 0; ++ci) {
            // largest LDS first: the one-workgroup-per-CU class suffers most from the gather chain, whose first pass is
            // the heavier one (measured: 48.3 -> 47.2 ms)
            const uint32_t cls = TILE_CLASSES - 1u - ci;
            const uint32_t n_cls = pl->class_first[cls + 1] - pl->class_first[cls];
            if (!n_cls) continue;
            CascadeArgs ta = ca;
            ta.tile_units = (const UnitDev*)pl->d_tile_units.p + pl->class_first[cls];
            ta.n_tile_units = n_cls;
            ta.tile_lds_bytes = pl->class_lds[cls];
            ta.tile_ticket = qcount(0, 0) + CountsLayout::tile_tickets(cls);   // queue 0 does not exist: its counters are free
            // workgroups per CU: what the LDS allows (160 KiB per CU), at most 4 x 8 waves
            const int per_cu = std::max(1, std::min(32 / TILE_WAVES, (int)(160u * 1024u / ta.tile_lds_bytes)));
            const int tb = (int)std::min<uint64_t>((uint64_t)n_cls * (uint64_t)nf, (uint64_t)e->n_cu * (uint64_t)per_cu);
            const uint32_t deepest = std::min<uint32_t>((uint32_t)pl->stages.size(), sch.handover);
            if (const int rc = log.begin(VJ_LAUNCH_TILE, (int)cls, 0, deepest, ta.tile_lds_bytes, e->stream)) return rc;
            ta.stage_entered = log.counters();
            const int hrc = launch_cascade_tile_pass(ta, pl->trees, count, std::max(1, tb), e->stream);
            if (const int rc = log.end(e->stream)) return rc;
            if (hrc) return launched(hrc);
        }
        return VJ_OK;
    }
    // 7. chain B: grid pass, then the queue passes fed by it alone
    int gather_chain() {
        if (ca.n_units == 0) return VJ_OK;
        CascadeArgs ga = queue_args(0);   // (q_ticket: pass 0's range — the tickets of the unit list's parts)
        if (const int rc = launch_gather(ga, VJ_LAUNCH_GRID, n_pass == 1, general_kernel && n_pass == 1, b_blocks, sB)) return rc;
        for (size_t ps = 1; ps < sch.first_joint_pass; ++ps) {
            CascadeArgs qa = queue_args(ps);
            // (next to the tiles one workgroup per CU; a stage tree's chains are latency-bound: all of them)
            const int qb = sch.split_sets ? n_blocks : b_blocks;
            qa.total_waves = (uint32_t)qb * qa.gather_waves;
            if (const int rc = launch_gather(qa, VJ_LAUNCH_QUEUE, pass_is_last(ps), false, qb, sB)) return rc;
        }
        return VJ_OK;
    }
    // 8. B joins A; the passes up to the first joint one are timed from here
    int join_chains() {
        if (sch.two_streams) {
            HIP_TRY(hipEventRecord(e->join_ev, e->stream2));
            HIP_TRY(hipStreamWaitEvent(e->stream, e->join_ev, 0));
        }
        for (size_t ps = 1; ps < n_pass && ps < VJ_MAX_PASSES && ps <= sch.first_joint_pass; ++ps)
            HIP_TRY(hipEventRecord(L->pass_ev[ps], e->stream));
        return VJ_OK;
    }
    // 9. the joint passes (split_sets: all of them once more, on the tiles' queue set)
    int joint_passes() {
        for (size_t ps = sch.split_sets ? 1 : sch.first_joint_pass; ps < n_pass; ++ps) {
            if (ps > sch.first_joint_pass && ps < VJ_MAX_PASSES) HIP_TRY(hipEventRecord(L->pass_ev[ps], e->stream));
            CascadeArgs qa = queue_args(ps, sch.split_sets ? 1 : 0);
            if (const int rc = launch_gather(qa, VJ_LAUNCH_QUEUE, pass_is_last(ps), general_kernel, n_blocks, e->stream)) return rc;
        }
        return VJ_OK;
    }
    // 10. read back the counters block and the first detections (nearly always all of them)
    int readback(int launches) {
        if (n_pass <= VJ_MAX_PASSES && launches) HIP_TRY(hipEventRecord(L->pass_ev[n_pass], e->stream));
        HIP_TRY(hipEventRecord(L->ev[3], e->stream));
        L->launches = launches;
        L->n_pass = n_pass;
        L->count = count;
        HIP_TRY(hipMemcpyAsync(L->h_pinned, L->d_counts.p, CountsLayout::bytes, hipMemcpyDeviceToHost, e->stream));
        L->det_copied = (uint32_t)std::min<size_t>(pinned_det_room(L->h_pinned_bytes), L->det_cap);
        HIP_TRY(hipMemcpyAsync((char*)L->h_pinned + PINNED_DET_OFF, L->d_det.p, (size_t)L->det_copied * sizeof(DetEntry), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipEventRecord(L->done, e->stream));
        L->pending = true;
        return VJ_OK;
    }
};

}  // namespace

int enqueue_cascade(vj_env* e, Lane* L, Plan* pl, int W, const vj_params& p) {
    int rc;
    CascadeRun r{e, L, pl, W, p};
    L->linfo.clear();
    if ((rc = r.zero_counters())) return rc;
    r.fill_base_args();
    if ((rc = r.skip_bitmap())) return rc;
    if ((rc = r.compute_schedule())) return rc;
    if (r.ca.n_units + r.ca.n_tile_units == 0) return r.readback(0);
    if ((rc = r.fork_chains())) return rc;
    // When the chains overlap, B goes first, so that the tile workgroups find their LDS share next to its small workgroups.
    if ((rc = r.sch.two_streams ? r.gather_chain() : r.tile_chain())) return rc;
    if ((rc = r.sch.two_streams ? r.tile_chain() : r.gather_chain())) return rc;
    if ((rc = r.join_chains())) return rc;
    if ((rc = r.joint_passes())) return rc;
    return r.readback((int)r.n_pass);
}

// Wait for the batch on lane L and decode it: detections appended to `dets` with frame numbers offset by f0.  When the
// detection buffer overflowed it is grown and the cascade passes run again — on the integral images still in place for a
// blocking call, after recomputing them from the lane's frames for a stream lane (the two lanes of a vj_stream share
// the environment's integral images, and the next batch's have replaced this one's by now).  The redo is ordered on the
// environment's stream behind everything already queued, and finished synchronously here.
int finish_batch(vj_env* e, Lane* L, Plan* pl, int f0, int W, int H, const vj_params& p, std::vector<RawDet>* dets,
                 vj_counters* ctr, vj_timing* tm) {
    int rc;
    for (int attempt = 0; attempt < 3; ++attempt) {
        HIP_TRY(hipEventSynchronize(L->done));
        L->pending = false;
        const size_t n_pass = L->n_pass;
        const int launches = L->launches;
        const bool count = L->count;
        const std::vector<vj_launch>& linfo = L->linfo;
        const uint32_t n_det = ((const uint32_t*)L->h_pinned)[CountsLayout::det_count_u32];
        float ms_i = 0, ms_c = 0, ms_t = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, L->ev[0], L->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_c, L->ev[2], L->ev[3]));
        HIP_TRY(hipEventElapsedTime(&ms_t, L->ev[0], L->ev[3]));
        if (n_det > L->det_cap) {  // detections overflowed: grow and redo the cascade passes
            const uint32_t want = grown_cap(L->det_cap, n_det);
            if ((rc = L->d_det.ensure((size_t)want * sizeof(DetEntry)))) return rc;
            L->det_cap = want;
            if (L->shared_integrals) {
                HIP_TRY(hipEventRecord(L->ev[0], e->stream));
                if ((rc = enqueue_integral(e, L->src_gray, L->src_frame_bytes, L->src_stride, W, H, L->nf, L->src_channels, L->sq_u32))) return rc;
                HIP_TRY(hipEventRecord(L->ev[1], e->stream));
            }
            if ((rc = enqueue_cascade(e, L, pl, W, p))) return rc;
            continue;
        }
        if (attempt == 0) tm->integral_ms += ms_i;
        tm->cascade_ms += ms_c;
        tm->total_ms += ms_t;
        if (launches && n_pass <= VJ_MAX_PASSES)
            for (size_t ps = 0; ps < n_pass; ++ps) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, L->pass_ev[ps], L->pass_ev[ps + 1]));
                tm->pass_ms[ps] += ms;
                tm->pass_stage_begin[ps] = (int32_t)pl->pass_bounds[ps];
                tm->pass_stage_end[ps] = (int32_t)pl->pass_bounds[ps + 1];
            }
        tm->n_cascade_launches = std::max(tm->n_cascade_launches, launches);
        const unsigned long long* se_all = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::stage_off_u32);
        if (linfo.size() <= VJ_MAX_LAUNCHES) {
            for (size_t i = 0; i < linfo.size(); ++i) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, L->launch_ev[2 * i], L->launch_ev[2 * i + 1]));
                vj_launch acc = tm->launch[i];   // sums over sub-batches: time and counters
                tm->launch[i] = linfo[i];
                tm->launch[i].ms = acc.ms + ms;
                const unsigned long long* se = se_all + (1 + i) * VJ_MAX_STAGES;
                for (size_t s = 0; s < (size_t)VJ_MAX_STAGES; ++s)
                    tm->launch[i].stage_entered[s] = acc.stage_entered[s] + (count ? se[s] : 0ull);
            }
            tm->n_launches = (int32_t)linfo.size();
        }
#ifdef VJ_STAMPS
        if (getenv("VJ_DEBUG_STAMPS")) {  // diagnostic build (-DVJ_STAMPS=1): phase cycle sums of the tile kernel
            const unsigned long long* se = se_all;
            for (size_t l = 0; l < linfo.size(); ++l)
                fprintf(stderr, "vj launch %zu kind %d class %d: max resident workgroups %llu\n", l, linfo[l].kind, linfo[l].lds_class,
                        se[(1 + l) * VJ_MAX_STAGES + 39]);
            for (size_t l = 0; l < linfo.size(); ++l)   // queue passes: chunk time sum / max / chunks; stump-parallel tail: A, B, pairs, stages
                if (linfo[l].kind == 1)
                    fprintf(stderr, "vj queue launch %zu [%d,%d): chunks %llu sum %llu max %llu | tail A %llu B %llu pairs %llu stages %llu\n", l,
                            linfo[l].stage_begin, linfo[l].stage_end, se[(1 + l) * VJ_MAX_STAGES + 50], se[(1 + l) * VJ_MAX_STAGES + 48],
                            se[(1 + l) * VJ_MAX_STAGES + 49], se[(1 + l) * VJ_MAX_STAGES + 51], se[(1 + l) * VJ_MAX_STAGES + 52],
                            se[(1 + l) * VJ_MAX_STAGES + 53], se[(1 + l) * VJ_MAX_STAGES + 54]);
            for (size_t l = 0; l < linfo.size(); ++l)   // grid pass: when the waves leave the unit loop (vj_kernels.hip, slots 40..45)
                if (linfo[l].kind == VJ_LAUNCH_GRID) {
                    const unsigned long long* g = se + (1 + l) * VJ_MAX_STAGES + 40;
                    const double wgs = (double)std::max(1ull, g[5]), span = (double)(g[3] - ~g[4]);
                    fprintf(stderr, "vj grid launch %zu: workgroups %llu span %.0f ticks | per workgroup last - mean wave end: mean %.0f (%.2f %%) max %llu (%.2f %%) | "
                            "launch end - mean last wave end %.0f (%.2f %%)\n", l, g[5], span, (double)g[0] / wgs, 100.0 * (double)g[0] / wgs / span, g[1],
                            100.0 * (double)g[1] / span, (double)g[3] - (double)g[2] / wgs, 100.0 * ((double)g[3] - (double)g[2] / wgs) / span);
                }
            fprintf(stderr, "vj stamps:");
            for (int i = 40; i < 63; ++i) {   // (60 .. 62: the dense sweep's groups, its lone chunks, how many lone chunks)
                unsigned long long v = 0;
                for (int l = 1; l <= VJ_MAX_LAUNCHES; ++l) v += se[l * VJ_MAX_STAGES + i];
                fprintf(stderr, " %llu", v);
            }
            fprintf(stderr, "\n");
        }
#endif
        if (count) {
            for (size_t s = 0; s < pl->stages.size(); ++s)
                for (int l = 1; l <= VJ_MAX_LAUNCHES; ++l) ctr->stage_entered[s] += se_all[(size_t)l * VJ_MAX_STAGES + s];
            // multi-node trees: nodes below the roots that the walks visited, and their rectangles — parked in the two derived
            // fields until fill_counters prices the roots (every entering window evaluates those) and adds these
            ctr->stump_evals += se_all[CountsLayout::tree_first_u64];
            ctr->gather_bytes += se_all[CountsLayout::tree_first_u64 + 1];
        }
        std::vector<DetEntry> raw(n_det);
        const uint32_t have = std::min(n_det, L->det_copied);
        if (have) memcpy(raw.data(), (const char*)L->h_pinned + PINNED_DET_OFF, (size_t)have * sizeof(DetEntry));
        if (n_det > have)
            HIP_TRY(hipMemcpy(raw.data() + have, (const DetEntry*)L->d_det.p + have, (size_t)(n_det - have) * sizeof(DetEntry), hipMemcpyDeviceToHost));
        for (const DetEntry& d : raw) {
            const WindowAt at = decode_window(d.off, pl->frame_elems, (uint32_t)W + 1u);
            dets->push_back(RawDet{f0 + (int)at.frame, d.scale, at.x, at.y});
        }
        return VJ_OK;
    }
    set_error("detection buffer overflow persisted");
    return VJ_ERR_LIMIT;
}

// Node evaluations as the oracle counts them: every node a window's walk visits.  Stumps: every node of an
// entered stage.  Multi-node trees: the root of every tree of an entered stage + the nodes below the roots that the
// counted kernels saw visited (parked in the two derived fields by whoever read the device's counters back).
void fill_counters(const Plan* pl, uint64_t windows, const vj_params& p, vj_counters* k) {
    if (!(p.flags & VJ_FLAG_COUNTERS)) return;
    k->windows = windows;
    uint64_t rect_evals = pl->trees ? k->gather_bytes : 0;
    k->stump_evals = pl->trees ? k->stump_evals : 0;
    for (size_t s = 0; s < pl->stages.size(); ++s) {
        k->stump_evals += k->stage_entered[s] * (pl->trees ? pl->prog.n_roots[s] : pl->prog.n_nodes[s]);
        rect_evals += k->stage_entered[s] * (pl->trees ? pl->prog.n_root_rects[s] : pl->prog.n_rects[s]);
    }
    k->gather_bytes = 48ull * k->windows + 16ull * rect_evals;
}

int rects_to_result(const std::vector<vj_rect>& rects, vj_result* out) {
    out->count = (uint32_t)rects.size();
    if (rects.empty()) return VJ_OK;
    out->rects = (vj_rect*)malloc(rects.size() * sizeof(vj_rect));
    if (!out->rects) return VJ_ERR_NOMEM;
    memcpy(out->rects, rects.data(), rects.size() * sizeof(vj_rect));
    return VJ_OK;
}

int build_result(const Plan* pl, std::vector<RawDet>& dets, uint64_t windows, const vj_params& p, vj_result* out) {
    // deterministic order: (frame, scale_idx, y, x)
    std::sort(dets.begin(), dets.end(), [](const RawDet& a, const RawDet& b) {
        return std::tie(a.frame, a.slot, a.y, a.x) < std::tie(b.frame, b.slot, b.y, b.x);
    });
    std::vector<vj_rect> rects(dets.size());
    for (size_t i = 0; i < dets.size(); ++i) {
        const vj_scale_info& si = pl->scales_info[dets[i].slot];
        rects[i] = vj_rect{(int32_t)dets[i].x, (int32_t)dets[i].y, si.win_w, si.win_h, 0.0f, dets[i].frame, si.scale_idx};
    }
    if (const int rc = rects_to_result(rects, out)) return rc;
    if (p.min_neighbors != 0 && out->count) {  // clod.cpp:1325-1326: filterResult(matches, n, MAX(min_neighbors, 1), EPS)
        const int rc = vj_group_rectangles(out->rects, &out->count, (int)std::max<uint32_t>(p.min_neighbors, 1u), 0.2);
        if (rc) return rc;
    }
    fill_counters(pl, windows, p, &out->counters);
    return VJ_OK;
}

uint64_t max_frames_per_subbatch(const vj_env* e, const Plan* pl) {
    return max_frames_for(pl->frame_elems, pl->max_reach_elems, pl->windows_per_frame, e->max_subbatch);
}

int subbatch_frames(const vj_env* e, const Plan* pl, const Plan* pl2, uint64_t* max_frames) {
    *max_frames = max_frames_per_subbatch(e, pl);
    if (pl2) *max_frames = std::min(*max_frames, max_frames_per_subbatch(e, pl2));
    if (*max_frames) return VJ_OK;
    set_error("a single frame exceeds the 32-bit offset range");
    return VJ_ERR_LIMIT;
}

// Feedback for the chain balance: only the timed (uncounted) kernel variants of a call that was one sub-batch.  A plan none of
// whose scales can run on tiles has nothing to balance; a CANDIDATE split that leaves one chain only (every tile moved to the
// gathers, or a share of the scales without large ones) is measured like any other — the search must be able to step back from it
void balance_feedback(vj_env::Balance* bal, const vj_env* e, const Plan* pl, const vj_params& p, int n_frames, uint64_t max_frames, vj_timing* timing) {
    if (bal && bal->phase != 3) {
        bool any_tile_scale = false;
        for (const ScaleDev& sd : pl->scales) any_tile_scale |= sd.tile_rw != 0;
        if (!any_tile_scale) {
            bal->cur = bal->best;
            bal->phase = 3;
        } else if (!(p.flags & VJ_FLAG_COUNTERS) && (uint64_t)n_frames <= max_frames && n_frames == bal->n_ref) {
            balance_report(bal, timing->cascade_ms / (float)n_frames, !e->tile_thresholds_set);
        }
    }
    timing->tile_split = pl->tile_split;
    timing->balance_state = !bal ? 0 : bal->phase == 3 ? 2 : 1;
    timing->balance_calls = bal ? bal->calls : 0;
}

}  // namespace vj

struct vj_stream {
    vj_env* e = nullptr;
    vj_params p;
    int W = 0, H = 0, CH = 1, max_batch = 0;
    std::unique_ptr<Plan> plan;     // private: its queue layout must not change while a batch is in flight
    Lane lanes[2];
    hipStream_t copy = nullptr;
    int fifo[2] = {0, 0};           // lanes holding submitted batches, oldest first
    int n_pending = 0;
    int n_frames_of[2] = {0, 0};
};

extern "C" {

int vj_detect(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_params* p,
              vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (n_frames == 0) return VJ_OK;
    // VJ_FLAG_EQUALIZE_HIST is read here and nowhere else: plans, balance entries and kernels see the parameters without it
    const bool equalize = (p->flags & VJ_FLAG_EQUALIZE_HIST) != 0u;
    vj_params q = *p;
    q.flags &= ~(uint32_t)VJ_FLAG_EQUALIZE_HIST;
    p = &q;
    int rc, W, H, CH;
    if ((rc = check_params(*p)) || (rc = check_frames(frames, n_frames, &W, &H, &CH))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    Plan* pl;
    vj_env::Balance* bal = balance_of(e, c, W, H, *p, n_frames, true);   // (created before the plan is looked up: it names the split)
    if (bal) balance_touch(bal, n_frames);
    if ((rc = get_plan(e, c, W, H, *p, &pl, n_frames))) return rc;
    uint64_t max_frames;
    if ((rc = subbatch_frames(e, pl, nullptr, &max_frames))) return rc;
    std::vector<RawDet> dets;
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        if ((rc = enqueue_prepare(e, &e->lane0, pl, frames + f0, nf, W, H, false, nullptr, equalize, true))) return rc;
        if ((rc = enqueue_cascade(e, &e->lane0, pl, W, *p))) return rc;
        if ((rc = finish_batch(e, &e->lane0, pl, f0, W, H, *p, &dets, &out->counters, &out->timing))) return rc;
    }
    balance_feedback(bal, e, pl, *p, n_frames, max_frames, &out->timing);
    return build_result(pl, dets, pl->windows_per_frame * (uint64_t)n_frames, *p, out);
}

void vj_result_free(vj_result* r) {
    if (!r) return;
    free(r->rects);
    r->rects = nullptr;
    r->count = 0;
}

// ------------------------------------------------------------------ frame streams: two lanes, so that batch k+1 uploads while the kernels of batch k run
int vj_stream_create(vj_env* e, const vj_cascade* c, int width, int height, int channels, int max_batch, const vj_params* p,
                     vj_stream** out) {
    if (!out) return VJ_ERR_ARG;
    *out = nullptr;
    if (!e || !c || !p || width <= 0 || height <= 0 || max_batch <= 0) return VJ_ERR_ARG;
    const int CH = channels <= 1 ? 1 : channels;
    if (CH != 1 && CH != 3 && CH != 4) return VJ_ERR_ARG;
    if (refuse_equalize(p->flags, "vj_stream_create")) return VJ_ERR_UNSUPPORTED;
    if (check_params(*p)) return VJ_ERR_ARG;
    if ((uint64_t)(width + 1) * (uint64_t)(height + 3) >= (1ull << 30)) {
        set_error("image too large");
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    auto s = std::make_unique<vj_stream>();
    s->e = e;
    s->p = *p;
    s->W = width;
    s->H = height;
    s->CH = CH;
    s->max_batch = max_batch;
    s->plan = std::make_unique<Plan>();
    struct Guard {   // releases what was created when a later step fails
        vj_stream* s;
        ~Guard() { if (s) vj_stream_destroy(s); }
    } guard{nullptr};
    // (a chain balance already found for this workload by vj_detect's feedback is taken over; a stream does not search itself)
    const vj_env::Balance* bal = balance_of(e, c, width, height, *p, max_batch, false);
    const bool lower_thresholds = bal && balance_choice(bal, -1).thr == 1 && !e->tile_thresholds_set;
    int rc = plan_and_upload(e, *c, width, height, *p, s->plan.get(), bal ? bal->best : e->split_for(max_batch, *p, linear_stumps(*c)),
                             thresholds_for(*e, lower_thresholds ? 3 : 0), max_batch, false);
    if (rc) {
        s->plan->release_device();
        return rc;
    }
    vj_stream* raw = s.release();
    guard.s = raw;
    if ((uint64_t)max_batch > max_frames_per_subbatch(e, raw->plan.get())) {
        set_error("max_batch %d exceeds what one launch sequence can address at this frame size (%llu frames)", max_batch,
                  (unsigned long long)max_frames_per_subbatch(e, raw->plan.get()));
        return VJ_ERR_LIMIT;
    }
    for (Lane& L : raw->lanes) {
        if ((rc = L.create())) return rc;
        L.shared_integrals = true;
    }
    HIP_TRY(hipStreamCreateWithFlags(&raw->copy, hipStreamNonBlocking));
    // every buffer at its final size now: nothing is (re)allocated while batches are in flight
    for (Lane& L : raw->lanes)
        if ((rc = ensure_image_buffers(e, width, height, max_batch, true, CH, &L))) return rc;
    if ((rc = ensure_queues(e, raw->plan.get(), max_batch))) return rc;
    guard.s = nullptr;
    *out = raw;
    return VJ_OK;
}

int vj_stream_submit(vj_stream* s, const vj_image* frames, int n_frames) {
    if (!s || !frames || n_frames <= 0 || n_frames > s->max_batch) return VJ_ERR_ARG;
    if (s->n_pending >= 2) {
        set_error("two batches are pending: collect one before submitting the next");
        return VJ_ERR_LIMIT;
    }
    int W, H, CH;
    int rc = check_frames(frames, n_frames, &W, &H, &CH);
    if (rc) return rc;
    if (W != s->W || H != s->H || CH != s->CH) {
        set_error("frames do not have the stream's size / channel count");
        return VJ_ERR_ARG;
    }
    vj_env* e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    const int lane = s->n_pending == 0 ? 0 : 1 - s->fifo[0];
    Lane* L = &s->lanes[lane];
    // the lane's frame buffer is free once the integral kernels of its previous batch have read it
    HIP_TRY(hipEventSynchronize(L->integral_done));
    if ((rc = enqueue_prepare(e, L, s->plan.get(), frames, n_frames, W, H, true, s->copy, false, true))) return rc;
    if ((rc = enqueue_cascade(e, L, s->plan.get(), W, s->p))) return rc;
    s->fifo[s->n_pending] = lane;
    s->n_frames_of[lane] = n_frames;
    s->n_pending++;
    return VJ_OK;
}

int vj_stream_collect(vj_stream* s, vj_result* out) {
    if (!s || !out) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (s->n_pending == 0) {
        set_error("no batch is pending");
        return VJ_ERR_ARG;
    }
    vj_env* e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    const int lane = s->fifo[0];
    s->fifo[0] = s->fifo[1];
    s->n_pending--;
    Lane* L = &s->lanes[lane];
    std::vector<RawDet> dets;
    if (const int rc = finish_batch(e, L, s->plan.get(), 0, s->W, s->H, s->p, &dets, &out->counters, &out->timing)) return rc;
    return build_result(s->plan.get(), dets, s->plan->windows_per_frame * (uint64_t)s->n_frames_of[lane], s->p, out);
}

void vj_stream_destroy(vj_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->e->device);
    if (s->e->stream) (void)hipStreamSynchronize(s->e->stream);
    if (s->e->stream2) (void)hipStreamSynchronize(s->e->stream2);
    if (s->copy) {
        (void)hipStreamSynchronize(s->copy);
        (void)hipStreamDestroy(s->copy);
    }
    for (Lane& L : s->lanes) L.destroy();
    if (s->plan) s->plan->release_device();
    delete s;
}

}  // extern "C"
