// Host driver of vj_run_windows: the clod profile's cascade on a caller's list of windows.  What needs no device
// — argument checks, per-scale geometry, the scatter of results — is vj_points_host.cpp; ordering and units are the OpenCV
// profile's (vj_cv_points_host.cpp); the node tables are build_node_table's (vj_plan.cpp), as every other clod path builds them.
#include "vj_env_internal.hpp"

#include <cmath>

using namespace vj;

namespace {

// The stage records of `c` (what the clod plans hold, once per cascade)
int get_clod_point_cascade(vj_env* e, const vj_cascade* c, uint64_t call_tick, ClodPointCascade** out) {
    auto it = e->clod_point_cascades.find(c->uid);
    if (it != e->clod_point_cascades.end()) {
        it->second->last_used = call_tick;
        *out = it->second.get();
        return VJ_OK;
    }
    cv_point_make_room(e, e->clod_point_cascades, call_tick);
    auto pc = std::make_unique<ClodPointCascade>();
    const StageProgram prog = build_stage_program(*c);
    std::vector<uint32_t> order;
    if (!stage_sweep_order(prog, &order)) {
        set_error("stage links form a cycle");
        return VJ_ERR_UNSUPPORTED;
    }
    const size_t n = c->stages.size();
    for (const auto& t : c->trees)
        if (t.n_nodes != 1) pc->trees = true;
    std::vector<StageDev> stages(n);
    for (size_t s = 0; s < n; ++s) {
        const bool linear = prog.on_fail[s] == STAGE_REJECT && (prog.on_pass[s] == (int)s + 1 || (prog.on_pass[s] == STAGE_ACCEPT && s + 1 == n));
        if (!linear) pc->is_tree = true;
        StageDev& sd = stages[s];
        memset(&sd, 0, sizeof(sd));
        sd.first_node = prog.first_node[s];
        sd.n_nodes = prog.n_nodes[s];
        sd.threshold = c->stages[s].threshold;
        sd.on_pass = prog.on_pass[s];
        sd.on_fail = prog.on_fail[s];
        sd.n_trees = (uint32_t)c->stages[s].n_trees;
        sd.order = s < order.size() ? order[s] : 0u;
    }
    pc->n_order = (uint32_t)order.size();
    pc->n_stages = (uint32_t)n;
    int rc = pc->d_stages.ensure(stages.size() * sizeof(StageDev));
    if (!rc && hipMemcpy(pc->d_stages.p, stages.data(), stages.size() * sizeof(StageDev), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("uploading the stage records failed");
        rc = VJ_ERR_HIP;
    }
    if (rc) {
        pc->release_device();
        return rc;
    }
    pc->last_used = call_tick;
    *out = pc.get();
    e->clod_point_cascades[c->uid] = std::move(pc);
    return VJ_OK;
}

// The record and node table of ONE scale on frames of width W (precomputeKernelCascade, clod.cpp:529-578, reads the image only
// through its width).  The table is built when the window fits the W x H frame: no window of a larger one is evaluated.
int get_clod_point_plan(vj_env* e, const vj_cascade* c, int W, int H, float scale, bool tilted_as_upright, uint64_t call_tick,
                        ClodPointPlan** out) {
    uint32_t bits;
    memcpy(&bits, &scale, 4);
    const vj_env::ClodPointPlanKey key(c->uid, W, bits, tilted_as_upright ? 1 : 0);
    auto it = e->clod_point_plans.find(key);
    ClodPointPlan* pl = it != e->clod_point_plans.end() ? it->second.get() : nullptr;
    const uint32_t stride = (uint32_t)W + 1u;
    ClodPointScale sc;
    int rc = clod_point_scale(c->win_w, c->win_h, scale, W, H, &sc);
    if (rc) return rc;
    if (!pl) {
        cv_point_make_room(e, e->clod_point_plans, call_tick);
        auto fresh = std::make_unique<ClodPointPlan>();
        pl = fresh.get();
        pl->rec.win_w = (uint32_t)sc.win_w;
        pl->rec.win_h = (uint32_t)sc.win_h;
        e->clod_point_plans[key] = std::move(fresh);
    }
    pl->last_used = call_tick;
    if (sc.fits && !pl->d_table.p) {
        pl->rec.area = (float)sc.area;
        pl->rec.e_lt = (uint32_t)sc.ex * stride + (uint32_t)sc.ex;
        pl->rec.e_dw = (uint32_t)sc.ew;
        pl->rec.e_dh = (uint32_t)sc.eh * stride;
        vj_scale_info si;
        memset(&si, 0, sizeof(si));
        si.scale = scale;
        si.area = sc.area;
        si.accepted = 1;
        std::vector<NodeRec> table(c->nodes.size());
        rc = build_node_table(*c, W, si, table.data());
        // furthest element a gather of this scale touches, from the window origin: the variance rectangle and every feature corner
        uint64_t reach = (uint64_t)pl->rec.e_lt + pl->rec.e_dh + pl->rec.e_dw;
        for (const NodeRec& r : table) {
            const uint32_t dw[3] = {r.dw01 & 0xffffu, r.dw01 >> 16, r.dw2_flags & 0xffffu};
            for (int q = 0; q < 3; ++q)
                if (q < 2 || r.w[2] != 0.0f) reach = std::max<uint64_t>(reach, ((uint64_t)r.lt[q] + r.dh[q] + dw[q]) / 4u);
        }
        pl->max_reach = reach;
        if (!rc) rc = pl->d_table.ensure(std::max<size_t>(table.size(), 1) * sizeof(NodeRec));
        if (!rc && !table.empty() && hipMemcpy(pl->d_table.p, table.data(), table.size() * sizeof(NodeRec), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("uploading a node table failed");
            rc = VJ_ERR_HIP;
        }
        if (rc) {
            pl->release_device();
            e->clod_point_plans.erase(key);
            return rc;
        }
        pl->rec.table = (const NodeRec*)pl->d_table.p;
    }
    *out = pl;
    return VJ_OK;
}

}  // namespace

extern "C" {

// runCascade + computeVariance on a caller's windows (clod.cpp:736-787, :418-446)
int vj_run_windows(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const float* scales, int n_scales,
                   const vj_window* windows, uint32_t n_windows, int start_stage, uint32_t flags, vj_clod_window_result* out) {
    int W = 0, H = 0, CH = 1;
    int rc = clod_points_check(c, frames, n_frames, scales, n_scales, windows, n_windows, start_stage, flags, out, &W, &H, &CH);
    if (rc) return rc;
    if (n_windows == 0) return VJ_OK;
    if (!e) {
        set_error("vj_run_windows: no environment");
        return VJ_ERR_ARG;
    }
    if ((int)c->stages.size() > VJ_MAX_STAGES || c->stages.empty()) {
        set_error("cascade has %zu stages; 1..%d are supported", c->stages.size(), VJ_MAX_STAGES);
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (plans may be released below)
    const uint64_t call_tick = ++e->plan_tick;
    ClodPointCascade* pc;
    if ((rc = get_clod_point_cascade(e, c, call_tick, &pc))) return rc;
    if (pc->is_tree && start_stage != 0) {
        set_error("vj_run_windows: a stage tree starts at stage 0 only (start_stage %d)", start_stage);
        return VJ_ERR_ARG;
    }
    const uint32_t stride = (uint32_t)W + 1u;
    const uint32_t frame_elems = frame_elems_for(W, H);
    // the slots some window names: their records; the others keep a window no frame holds (they are never read)
    std::vector<uint8_t> used((size_t)n_scales, 0);
    for (uint32_t i = 0; i < n_windows; ++i) used[(size_t)windows[i].scale] = 1;
    std::vector<ClodPointScaleDev> recs((size_t)n_scales);
    for (int k = 0; k < n_scales; ++k) {
        memset(&recs[(size_t)k], 0, sizeof(ClodPointScaleDev));
        recs[(size_t)k].win_w = recs[(size_t)k].win_h = CV_POINT_WIN_MAX;
        if (!used[(size_t)k]) continue;
        ClodPointPlan* pl;
        if ((rc = get_clod_point_plan(e, c, W, H, scales[k], (flags & VJ_FLAG_TILTED_AS_UPRIGHT) != 0u, call_tick, &pl))) return rc;
        recs[(size_t)k] = pl->rec;
        if ((int)pl->rec.win_w > W || (int)pl->rec.win_h > H) {   // outside everywhere
            recs[(size_t)k].table = nullptr;
            continue;
        }
        // the feature-reach check of the other clod paths, per slot: evaluated windows lie inside the frame; a feature may overshoot
        // its window by one column / row (separate rounding) into the frame allocation's zeroed slack rows
        const uint64_t origin_max = (uint64_t)(H - (int)pl->rec.win_h) * stride + (uint64_t)(W - (int)pl->rec.win_w);
        if (origin_max + pl->max_reach >= (uint64_t)frame_elems) {
            set_error("scale %d (%.9g): feature reach exceeds the frame allocation", k, (double)scales[k]);
            return VJ_ERR_LIMIT;
        }
    }
    if ((rc = e->d_cv_point_scales.ensure(recs.size() * sizeof(ClodPointScaleDev)))) return rc;
    HIP_TRY(hipMemcpy(e->d_cv_point_scales.p, recs.data(), recs.size() * sizeof(ClodPointScaleDev), hipMemcpyHostToDevice));
    // a sub-batch: its sum images within 32-bit byte offsets, and its sqsum images too (one buffer descriptor for all of its frames)
    const uint64_t frame_bytes = (uint64_t)frame_elems * 4u;
    if (frame_bytes * 2u > 0xfffffff0ull) {   // (the kernel's 32-bit sqsum offsets would wrap)
        set_error("vj_run_windows: a %d x %d frame's sqsum image exceeds one 4 GiB buffer descriptor", W, H);
        return VJ_ERR_LIMIT;
    }
    int max_frames = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_frames, 0xfffffff0ull / (frame_bytes * 2u)));
    if (e->max_subbatch > 0) max_frames = std::min(max_frames, e->max_subbatch);
    std::vector<uint32_t> order;
    std::vector<size_t> sub_first;
    cv_points_order(windows, n_windows, n_frames, max_frames, &order, &sub_first);
    e->cv_points_integral_ms = e->cv_points_pass_ms = 0.0f;
    std::vector<CvPointDev> points;
    std::vector<CvPointUnit> units;
    std::vector<ClodPointResult> res;
    for (size_t b = 0; b + 1 < sub_first.size(); ++b) {
        const size_t m = sub_first[b + 1] - sub_first[b];
        if (m == 0) continue;   // (a sub-batch no window looks at is not uploaded; within one, every frame is)
        const int f0 = (int)b * max_frames, nf = std::min(max_frames, n_frames - f0);
        const uint32_t* ord = order.data() + sub_first[b];
        cv_points_build(windows, ord, m, f0, &points, &units);
        if ((rc = ensure_image_buffers(e, W, H, nf, true, CH))) return rc;
        const uint8_t* d_gray;
        size_t gray_frame_bytes;
        int gray_stride;
        if ((rc = stage_frames(e, frames + f0, nf, W, H, &d_gray, &gray_frame_bytes, &gray_stride))) return rc;
        HIP_TRY(hipEventRecord(e->lane0.ev[0], e->stream));
        if ((rc = enqueue_integral(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, CH))) return rc;
        HIP_TRY(hipEventRecord(e->lane0.ev[1], e->stream));
        if ((rc = e->d_cv_points.ensure(points.size() * sizeof(CvPointDev)))) return rc;
        if ((rc = e->d_cv_point_units.ensure(units.size() * sizeof(CvPointUnit)))) return rc;
        if ((rc = e->d_cv_point_out.ensure(m * sizeof(ClodPointResult)))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_cv_points.p, points.data(), points.size() * sizeof(CvPointDev), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->d_cv_point_units.p, units.data(), units.size() * sizeof(CvPointUnit), hipMemcpyHostToDevice, e->stream));
        ClodPointArgs a;
        memset(&a, 0, sizeof(a));
        a.sum = (const uint32_t*)e->d_sum.p;
        a.sqsum = (const uint64_t*)e->d_sqsum.p;
        a.scales = (const ClodPointScaleDev*)e->d_cv_point_scales.p;
        a.stages = (const StageDev*)pc->d_stages.p;
        a.points = (const CvPointDev*)e->d_cv_points.p;
        a.units = (const CvPointUnit*)e->d_cv_point_units.p;
        a.out = (ClodPointResult*)e->d_cv_point_out.p;
        a.n_units = (uint32_t)units.size();
        a.n_points = (uint32_t)m;
        a.n_frames = (uint32_t)nf;
        a.frame_elems = frame_elems;
        a.stride = stride;
        a.width = (uint32_t)W;
        a.height = (uint32_t)H;
        a.n_stages = pc->n_stages;
        a.n_order = pc->n_order;
        a.start_stage = (uint32_t)std::min<int>(start_stage, (int)pc->n_stages);
        a.signed_mean = (flags & VJ_FLAG_SIGNED_MEAN) ? 1u : 0u;
        // one wave per unit, at most four workgroups (16 waves) per CU; the rest by stride
        const int n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((units.size() + CLOD_POINT_WAVES - 1) / CLOD_POINT_WAVES, (uint64_t)std::max(1, e->n_cu * 4)));
        a.total_waves = (uint32_t)n_blocks * CLOD_POINT_WAVES;
        HIP_TRY(hipEventRecord(e->lane0.ev[2], e->stream));
        const int hrc = launch_clod_points_pass(a, pc->trees, pc->is_tree, n_blocks, e->stream);
        if (hrc) {
            set_error("window-list launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
        HIP_TRY(hipEventRecord(e->lane0.ev[3], e->stream));
        res.resize(m);
        HIP_TRY(hipMemcpyAsync(res.data(), e->d_cv_point_out.p, m * sizeof(ClodPointResult), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        float ms_i = 0, ms_p = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_p, e->lane0.ev[2], e->lane0.ev[3]));
        e->cv_points_integral_ms += ms_i;
        e->cv_points_pass_ms += ms_p;
        clod_points_scatter(res.data(), ord, m, out);
    }
    return VJ_OK;
}

}  // extern "C"
