// Host driver of the window-list calls: a cascade on a caller's list of windows, written once for both arithmetic
// profiles.  run_points<P> is instantiated where P's builders live: vj_cv.cpp (vj_run_windows_opencv) and vj_points_driver.cpp
// (vj_run_windows); what needs no device is vj_cv_points_host.cpp and vj_points_host.cpp.  A profile P is a struct of types,
// constants and static functions, no object (the caller's scale and result types come with the entry point's arguments):
//   name; waves             the entry point, for messages; waves per workgroup of the pass
//   Geom                    what a scale gives whatever the image (win_w, win_h, fits)
//   ScaleDev, Result, Args  the kernel's scale record, verdict and arguments
//   check, scatter          the device-free refusals and the verdicts' way back (vj_*points_host.hpp)
//   cascades(e), plans(e), plan_key(c, W, scale, flags)            its two caches
//   build_stages(c, prog, order, pc, &stages)                      a cascade's stage records and PointCascade's flags
//   geometry(c, scale, W, H, &g), build_scale(c, scale, W, g, &rec, table, &max_reach)   one scale's Geom (or its refusal); its record, table, reach
//   extra_images(e, pc, d_gray, ...), fill_args(e, pc, flags, &a)  images beyond sum and sqsum, timed with them; the Args fields only P has
//   launch(a, pc, n_blocks, stream)
#pragma once
#include "vj_env_internal.hpp"

namespace vj {

// The entry of `m` for `uid`, touched; a new one is built by build(c, prog, order, pc, &stages) and its stage records uploaded.
template <class Build>
int get_point_cascade(vj_env* e, vj_env::PointCascades& m, const vj_cascade* c, uint64_t call_tick, PointCascade** out, Build build) {
    auto it = m.find(c->uid);
    if (it != m.end()) {
        it->second->last_used = call_tick;
        *out = it->second.get();
        return VJ_OK;
    }
    cache_make_room(e, m, call_tick);
    auto pc = std::make_unique<PointCascade>();
    const StageProgram prog = build_stage_program(*c);
    std::vector<uint32_t> order;
    if (!stage_sweep_order(prog, &order)) {
        set_error("stage links form a cycle");
        return VJ_ERR_UNSUPPORTED;
    }
    pc->n_order = (uint32_t)order.size();
    pc->n_stages = (uint32_t)c->stages.size();
    std::vector<StageDev> stages;
    build(c, prog, order, pc.get(), &stages);
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
    m[c->uid] = std::move(pc);
    return VJ_OK;
}

// The entry of `m` for `key`, touched; a new one starts with the scale's window size.  build(&rec, table, &max_reach) and the upload
// run when the window fits the frame and no table exists yet (no window of a larger one is evaluated); on failure the entry is erased.
template <class Map, class Plan, class Build>
int get_point_plan(vj_env* e, Map& m, const typename Map::key_type& key, uint32_t win_w, uint32_t win_h, bool fits, size_t n_nodes,
                   uint64_t call_tick, Plan** out, Build build) {
    auto it = m.find(key);
    Plan* pl = it != m.end() ? it->second.get() : nullptr;
    if (!pl) {
        cache_make_room(e, m, call_tick);
        auto fresh = std::make_unique<Plan>();
        pl = fresh.get();
        pl->rec.win_w = win_w;
        pl->rec.win_h = win_h;
        m[key] = std::move(fresh);
    }
    pl->last_used = call_tick;
    if (fits && !pl->d_table.p) {
        std::vector<typename Plan::Node> table(n_nodes);
        int rc = build(&pl->rec, table.data(), &pl->max_reach);
        if (!rc) rc = pl->d_table.ensure(std::max<size_t>(n_nodes, 1) * sizeof(typename Plan::Node));
        if (!rc && n_nodes && hipMemcpy(pl->d_table.p, table.data(), n_nodes * sizeof(typename Plan::Node), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("uploading a node table failed");
            rc = VJ_ERR_HIP;
        }
        if (rc) {
            pl->release_device();
            m.erase(key);
            return rc;
        }
        pl->rec.table = (const typename Plan::Node*)pl->d_table.p;
    }
    *out = pl;
    return VJ_OK;
}

template <class P, class Scale, class Out>
int run_points(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const Scale* scales, int n_scales,
               const vj_window* windows, uint32_t n_windows, int start_stage, uint32_t flags, Out* out) {
    typedef typename P::ScaleDev ScaleDev;
    typedef typename P::Result Result;
    int W = 0, H = 0, CH = 1;
    int rc = P::check(c, frames, n_frames, scales, n_scales, windows, n_windows, start_stage, flags, out, &W, &H, &CH);
    if (rc) return rc;
    if (n_windows == 0) return VJ_OK;
    if (!e) {
        set_error("%s: no environment", P::name);
        return VJ_ERR_ARG;
    }
    if ((int)c->stages.size() > VJ_MAX_STAGES || c->stages.empty()) {
        set_error("cascade has %zu stages; 1..%d are supported", c->stages.size(), VJ_MAX_STAGES);
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (plans may be released below)
    const uint64_t call_tick = ++e->plan_tick;
    PointCascade* pc;
    if ((rc = get_point_cascade(e, P::cascades(e), c, call_tick, &pc, P::build_stages))) return rc;
    const uint32_t stride = (uint32_t)W + 1u;
    const uint32_t frame_elems = frame_elems_for(W, H);
    // the slots some window names: their records; the others keep a window no frame holds (they are never read)
    std::vector<uint8_t> used((size_t)n_scales, 0);
    for (uint32_t i = 0; i < n_windows; ++i) used[(size_t)windows[i].scale] = 1;
    std::vector<ScaleDev> recs((size_t)n_scales);
    for (int k = 0; k < n_scales; ++k) {
        memset(&recs[(size_t)k], 0, sizeof(ScaleDev));
        recs[(size_t)k].win_w = recs[(size_t)k].win_h = CV_POINT_WIN_MAX;
        if (!used[(size_t)k]) continue;
        typename P::Geom g;
        if ((rc = P::geometry(c, scales[k], W, H, &g))) return rc;
        PointPlan<ScaleDev>* pl;
        rc = get_point_plan(e, P::plans(e), P::plan_key(c, W, scales[k], flags), (uint32_t)g.win_w, (uint32_t)g.win_h, g.fits, c->nodes.size(),
                            call_tick, &pl, [&](ScaleDev* rec, typename PointPlan<ScaleDev>::Node* table, uint64_t* max_reach) {
                                return P::build_scale(c, scales[k], W, g, rec, table, max_reach);
                            });
        if (rc) return rc;
        recs[(size_t)k] = pl->rec;
        if ((int)pl->rec.win_w > W || (int)pl->rec.win_h > H) {   // outside everywhere
            recs[(size_t)k].table = nullptr;
            continue;
        }
        // evaluated windows lie inside the frame; a feature may overshoot its window by one column / row (separate rounding) into
        // the frame allocation's zeroed slack rows, as for whole frames
        const uint64_t origin_max = (uint64_t)(H - (int)pl->rec.win_h) * stride + (uint64_t)(W - (int)pl->rec.win_w);
        if (origin_max + pl->max_reach >= (uint64_t)frame_elems) {
            set_error("scale %d (%.*g): feature reach exceeds the frame allocation", k, std::numeric_limits<Scale>::max_digits10,
                      (double)scales[k]);
            return VJ_ERR_LIMIT;
        }
    }
    if ((rc = e->d_point_scales.ensure(recs.size() * sizeof(ScaleDev)))) return rc;
    HIP_TRY(hipMemcpy(e->d_point_scales.p, recs.data(), recs.size() * sizeof(ScaleDev), hipMemcpyHostToDevice));
    // a sub-batch: its sum images within 32-bit byte offsets, and its sqsum images too (one buffer descriptor for all of its frames)
    const uint64_t frame_bytes = (uint64_t)frame_elems * 4u;
    if (frame_bytes * 2u > 0xfffffff0ull) {   // (the kernel's 32-bit sqsum offsets would wrap)
        set_error("%s: a %d x %d frame's sqsum image exceeds one 4 GiB buffer descriptor", P::name, W, H);
        return VJ_ERR_LIMIT;
    }
    int max_frames = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_frames, 0xfffffff0ull / (frame_bytes * 2u)));
    if (e->max_subbatch > 0) max_frames = std::min(max_frames, e->max_subbatch);
    std::vector<uint32_t> order;
    std::vector<size_t> sub_first;
    cv_points_order(windows, n_windows, n_frames, max_frames, &order, &sub_first);
    e->points_integral_ms = e->points_pass_ms = 0.0f;
    std::vector<CvPointDev> points;
    std::vector<CvPointUnit> units;
    std::vector<Result> res;
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
        if ((rc = P::extra_images(e, *pc, d_gray, gray_frame_bytes, gray_stride, W, H, nf, CH))) return rc;
        HIP_TRY(hipEventRecord(e->lane0.ev[1], e->stream));
        if ((rc = e->d_points.ensure(points.size() * sizeof(CvPointDev)))) return rc;
        if ((rc = e->d_point_units.ensure(units.size() * sizeof(CvPointUnit)))) return rc;
        if ((rc = e->d_point_out.ensure(m * sizeof(Result)))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_points.p, points.data(), points.size() * sizeof(CvPointDev), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->d_point_units.p, units.data(), units.size() * sizeof(CvPointUnit), hipMemcpyHostToDevice, e->stream));
        typename P::Args a;
        memset(&a, 0, sizeof(a));
        a.sum = (const uint32_t*)e->d_sum.p;
        a.sqsum = (const uint64_t*)e->d_sqsum.p;
        a.scales = (const ScaleDev*)e->d_point_scales.p;
        a.stages = (const StageDev*)pc->d_stages.p;
        a.points = (const CvPointDev*)e->d_points.p;
        a.units = (const CvPointUnit*)e->d_point_units.p;
        a.out = (Result*)e->d_point_out.p;
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
        P::fill_args(e, *pc, flags, &a);
        // one wave per unit, at most four workgroups (16 waves) per CU; the rest by stride
        const int n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((units.size() + P::waves - 1) / P::waves, (uint64_t)std::max(1, e->n_cu * 4)));
        a.total_waves = (uint32_t)n_blocks * P::waves;
        HIP_TRY(hipEventRecord(e->lane0.ev[2], e->stream));
        const int hrc = P::launch(a, *pc, n_blocks, e->stream);
        if (hrc) {
            set_error("window-list launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
        HIP_TRY(hipEventRecord(e->lane0.ev[3], e->stream));
        res.resize(m);
        HIP_TRY(hipMemcpyAsync(res.data(), e->d_point_out.p, m * sizeof(Result), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        float ms_i = 0, ms_p = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_p, e->lane0.ev[2], e->lane0.ev[3]));
        e->points_integral_ms += ms_i;
        e->points_pass_ms += ms_p;
        P::scatter(res.data(), ord, m, out);
    }
    return VJ_OK;
}

}  // namespace vj
