// gfx950 kernel of the OpenCV arithmetic profile's window-list pass (vj_run_windows_opencv):
// cvRunHaarClassifierCascadeSum (tempcv.cpp:795-972) on windows the CALLER names — (frame, x, y, scale slot) — with the cascade set to
// the slot's scale as cvSetImagesForHaarClassifierCascade sets it (:549-768: one node table per slot, built on the host with the
// frame's stride).  Every window gets the function's two results: its return value and the f64 it leaves in stage_sum.
//
// One work unit is up to 64 windows of one scale slot (the host groups the list by slot): one wave, lane = window, wave-uniform
// control flow.  The border rule (:817-820) comes first, in 64 bits — the coordinates are the caller's, any int32 — and a lane it
// catches reads no image: it writes -1 and is done.  The others take their variance norm factor (cv_window_vnf) and then
//   linear cascades  the stages from start_stage on over the wave's LDS queue, compacted after every stage (the sweep of cv_flush_to,
//                    its stump-parallel form for a thin population included); who fails a stage writes (-stage, its sum) before the
//                    compaction drops it, who passes the last stage writes (1, the last sum);
//   stage trees      the whole tree in lock-step (the form of cv_roi_pass: stages swept once in a topological order, every lane
//                    carrying the stage it visits next), every lane keeping the sum of the stage it evaluated last.
// Per-window arithmetic: vj_cv_window.hpp, unchanged.  The verdicts are written with ordinary vector stores, each lane its own entry.
// MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_cv_window.hpp"
#include "vj_cv_points_units.hpp"

namespace vj {

template <bool TREES, bool STAGE_TREE>
__global__ __launch_bounds__(CV_WAVES_PER_BLOCK * 64) void cv_points_pass(CvPointArgs a) {
    // per wave: 64 queue entries, then the stump-parallel form's verdict masks (CV_TAIL_MAX x CV_TAIL_BLOCKS words) — CV_QCAP entries hold both
    static_assert(CV_QCAP * sizeof(CvQEntry) >= CV_TAIL_MAX * sizeof(CvQEntry) + CV_TAIL_MAX * CV_TAIL_BLOCKS * 8u, "queue + masks fit");
    __shared__ CvQEntry lds_q[CV_WAVES_PER_BLOCK * CV_QCAP];
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CvQEntry* q = lds_q + wib * CV_QCAP;
    const uint32_t rank = blockIdx.x * CV_WAVES_PER_BLOCK + wib;
    kptr<CvPointScaleDev> scales = as_k(a.scales);
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvPointUnit> units = as_k(a.units);
    // (the host keeps a sub-batch's sqsum images below 4 GiB, so one descriptor each covers the batch)
    const uint32_t batch_elems = a.n_frames * a.frame_elems;
    const rsrc_t img = make_rsrc(a.sum, batch_elems * 4u);
    const rsrc_t timg = make_rsrc(a.tilted != nullptr ? a.tilted : a.sum, batch_elems * 4u);
    const rsrc_t sq = make_rsrc(a.sqsum, batch_elems * 8u);

    // the waves of an XCD walk one contiguous eighth of the unit list (as cv_roi_pass deals its units): one slot's table at a time
    uint32_t u_first = rank, u_end = a.n_units, u_step = a.total_waves;
    if (gridDim.x >= 8u) {
        const uint32_t xcd = blockIdx.x & 7u;
        const uint32_t u_begin = (uint32_t)((unsigned long long)a.n_units * xcd / 8u);
        u_end = (uint32_t)((unsigned long long)a.n_units * (xcd + 1u) / 8u);
        u_step = ((gridDim.x - xcd + 7u) >> 3) * CV_WAVES_PER_BLOCK;
        u_first = u_begin + (blockIdx.x >> 3) * CV_WAVES_PER_BLOCK + wib;
    }
    for (uint32_t u = u_first; u < u_end; u += u_step) {
        const uint32_t first = units[u].first, count = min(units[u].count, CV_POINT_UNIT), slot = units[u].slot;
        const double inv_area = scales[slot].inv_area;
        const uint32_t win_w = scales[slot].win_w, win_h = scales[slot].win_h;
        const uint32_t q0 = scales[slot].q0, q1 = scales[slot].q1, q2 = scales[slot].q2, q3 = scales[slot].q3;
        kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(scales[slot].table));
        const bool valid = lane < count && first + lane < a.n_points;
        CvPointDev p = CvPointDev{-1, -1, 0u, 0u};
        if (valid) p = a.points[first + lane];
        const bool writes = valid && p.index < a.n_points;
        // pt.x < 0 || pt.y < 0 || pt.x + real_window_size.width >= sum.width || pt.y + real_window_size.height >= sum.height (:817-820)
        const bool border = p.x < 0 || p.y < 0 || (long long)p.x + (long long)win_w >= (long long)a.width + 1ll ||
                            (long long)p.y + (long long)win_h >= (long long)a.height + 1ll || p.frame >= a.n_frames;
        const bool eval = writes && !border;
        if (writes && border) a.out[p.index] = CvPointResult{-1, 0, 0.0};
        // (an evaluated window lies inside the frame: the offsets below are those of an in-frame origin)
        const uint32_t po = eval ? p.frame * a.frame_elems + (uint32_t)p.y * a.stride + (uint32_t)p.x : 0u;
        const uint32_t off = po * 4u;
        double vnf = 1.0;
        if (eval) cv_window_vnf(img, sq, off, po, q0, q1, q2, q3, inv_area, vnf);
        if (STAGE_TREE) {
            // tempcv.cpp:834-861: stage_sum is that of the stage evaluated last; any reject returns 0
            int32_t ptr = eval ? (int32_t)stages[0].order : -3;   // -1 accepted, -2 rejected, -3 not evaluated
            double last_sum = 0.0;
            for (uint32_t oi = 0; oi < a.n_order; ++oi) {
                const uint32_t s = stages[oi].order;
                const bool here = ptr == (int32_t)s;
                if (__ballot(here) == 0ull) continue;
                if (here) {
                    last_sum = cv_stage_sum<TREES, false>(img, timg, table + stages[s].first_node, stages[s].n_nodes, off, vnf);
                    ptr = last_sum >= (double)stages[s].threshold ? stages[s].on_pass : stages[s].on_fail;
                }
            }
            if (eval) a.out[p.index] = CvPointResult{ptr == -1 ? 1 : 0, 0, last_sum};
            continue;
        }
        if (a.start_stage >= a.n_stages) {   // the stage loop does not run (:864, :952): 1, stage_sum never written
            if (eval) a.out[p.index] = CvPointResult{1, 0, 0.0};
            continue;
        }
        const unsigned long long em = __ballot(eval);
        uint32_t n = (uint32_t)__popcll(em);
        if (eval) q[mbcnt(em)] = CvQEntry{off, p.index, vnf};   // (xy carries the window's entry of `out`)
        __builtin_amdgcn_wave_barrier();
        const bool upright = !TREES && a.tilted == nullptr;   // (the stump-parallel form reads the upright sum image only)
        for (uint32_t s = a.start_stage; s < a.n_stages && n != 0u; ++s) {
            kptr<NodeRecDev> tab = table + stages[s].first_node;
            const uint32_t n_nodes = stages[s].n_nodes, f64 = stages[s].cv_f64;
            const double thr = (double)stages[s].threshold;
            const bool have = lane < n, last = s + 1u == a.n_stages;
            const CvQEntry e = q[have ? lane : 0u];
            double ssum = 0.0;
            if (upright && n <= a.tail_max && n_nodes >= 16u && n_nodes <= CV_TAIL_BLOCKS * 64u) {
                // a thin population: the stage stump-parallel (lane = stump), verdict bits replayed in stump order
                const uint32_t* recs_g = reinterpret_cast<const uint32_t*>((uintptr_t)tab);
                unsigned long long* masks = reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX);
                ssum = f64 != 0u ? cv_tail_stage_sum<true>(img, recs_g, tab, n_nodes, q, n, masks, lane)
                                 : cv_tail_stage_sum<false>(img, recs_g, tab, n_nodes, q, n, masks, lane);
            } else if (have) {
                ssum = cv_stage_sum_mode<TREES>(img, timg, tab, n_nodes, e.off, e.vnf, f64, a.tree2);
            }
            const bool pass = have && ssum >= thr;
            // `return -i` with stage_sum = this stage's (:947-949, :963-965); after the last stage `return 1`
            if (have && (!pass || last) && e.xy < a.n_points) a.out[e.xy] = CvPointResult{pass ? 1 : -(int32_t)s, 0, ssum};
            const unsigned long long pm = __ballot(pass);
            __builtin_amdgcn_wave_barrier();
            if (pass) q[mbcnt(pm)] = e;
            n = (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_wave_barrier();
    }
}

int launch_cv_points_pass(const CvPointArgs& a, bool trees, bool stage_tree, int n_blocks, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    dim3 g(n_blocks), b(CV_WAVES_PER_BLOCK * 64);
    if (stage_tree) {
        if (trees) hipLaunchKernelGGL((cv_points_pass<true, true>), g, b, 0, stream, a);
        else       hipLaunchKernelGGL((cv_points_pass<false, true>), g, b, 0, stream, a);
    } else {
        if (trees) hipLaunchKernelGGL((cv_points_pass<true, false>), g, b, 0, stream, a);
        else       hipLaunchKernelGGL((cv_points_pass<false, false>), g, b, 0, stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace vj
