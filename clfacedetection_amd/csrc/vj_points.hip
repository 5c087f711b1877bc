// gfx950 kernel of the clod arithmetic profile's window-list pass (vj_run_windows): runCascade (clod.cpp:736-787)
// on windows the CALLER names — (frame, x, y, scale slot) — with what setupScale (:371-415) and precomputeKernelCascade (:529-578)
// give for the slot's scale (one node table per slot, built on the host with the frame's stride).  Every window gets the
// function's return value, computeVariance's value (:418-446) and the f32 sum of the stage that decided.
//
// One work unit is up to 64 windows of one scale slot (the host groups the list by slot): one wave, lane = window, wave-uniform
// control flow.  The inside test comes first, in 64 bits — the coordinates are the caller's, any int32 — and a lane it catches
// reads no image: it stores (VJ_WINDOW_OUTSIDE, 0, 0) and is done.  The others take their variance and then
//   linear cascades  the stages from start_stage on over the wave's LDS queue, compacted with a ballot after every stage; who
//                    fails a stage stores (-stage, variance, its sum) before the compaction drops it, who passes the last stage
//                    stores (1, variance, the last sum);
//   stage trees      the whole tree in lock-step (stages swept once in a topological order, every lane carrying the stage it
//                    visits next, tempcv.cpp:834-861), every lane keeping the sum of the stage it evaluated last; a reject is 0.
// Per-window arithmetic: vj_clod_window.hpp.  The only stores are one 16-byte record per window, ordinary vector stores, each to an
// index checked against the list's length.  MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_clod_window.hpp"
#include "vj_points_units.hpp"

namespace vj {

struct ClodQEntry {
    uint32_t off;     // byte offset of the window origin in the batch sum image
    uint32_t index;   // the window's entry of ClodPointArgs::out
    float    var;
};

template <bool TREES, bool STAGE_TREE>
__global__ __launch_bounds__(CLOD_POINT_WAVES * 64) void clod_points_pass(ClodPointArgs a) {
    __shared__ ClodQEntry lds_q[CLOD_POINT_WAVES * 64];
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    ClodQEntry* q = lds_q + wib * 64u;
    const uint32_t rank = blockIdx.x * CLOD_POINT_WAVES + wib;
    kptr<ClodPointScaleDev> scales = as_k(a.scales);
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvPointUnit> units = as_k(a.units);
    // (the host keeps a sub-batch's sqsum images below 4 GiB, so one descriptor each covers the batch; a read beyond it returns 0)
    const uint32_t batch_elems = a.n_frames * a.frame_elems;
    const rsrc_t img = make_rsrc(a.sum, batch_elems * 4u);
    const rsrc_t sq = make_rsrc(a.sqsum, batch_elems * 8u);

    // the waves of an XCD walk one contiguous eighth of the unit list (workgroups go round the 8 XCDs): one slot's table at a time in its L2
    uint32_t u_first = rank, u_end = a.n_units, u_step = a.total_waves;
    if (gridDim.x >= 8u) {
        const uint32_t xcd = blockIdx.x & 7u;
        const uint32_t u_begin = (uint32_t)((unsigned long long)a.n_units * xcd / 8u);
        u_end = (uint32_t)((unsigned long long)a.n_units * (xcd + 1u) / 8u);
        u_step = ((gridDim.x - xcd + 7u) >> 3) * CLOD_POINT_WAVES;
        u_first = u_begin + (blockIdx.x >> 3) * CLOD_POINT_WAVES + wib;
    }
    for (uint32_t u = u_first; u < u_end; u += u_step) {
        const uint32_t first = units[u].first, count = min(units[u].count, CV_POINT_UNIT), slot = units[u].slot;
        const float area = scales[slot].area;
        const uint32_t win_w = scales[slot].win_w, win_h = scales[slot].win_h;
        const uint32_t e_lt = scales[slot].e_lt, e_dw = scales[slot].e_dw, e_dh = scales[slot].e_dh;
        kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(scales[slot].table));
        const bool valid = lane < count && first + lane < a.n_points;
        CvPointDev p = CvPointDev{-1, -1, 0u, 0u};
        if (valid) p = a.points[first + lane];
        const bool writes = valid && p.index < a.n_points;
        // evaluated iff x >= 0, y >= 0, x + sw <= W, y + sh <= H: beyond that the reference reads outside the image
        const bool outside = p.x < 0 || p.y < 0 || (long long)p.x + (long long)win_w > (long long)a.width ||
                             (long long)p.y + (long long)win_h > (long long)a.height || p.frame >= a.n_frames;
        const bool eval = writes && !outside;
        if (writes && outside) a.out[p.index] = ClodPointResult{CLOD_POINT_OUTSIDE, 0.0f, 0.0f, 0};
        // (an evaluated window lies inside the frame: the offsets below are those of an in-frame origin)
        const uint32_t e = eval ? p.frame * a.frame_elems + (uint32_t)p.y * a.stride + (uint32_t)p.x : 0u;
        const uint32_t off = e * 4u;
        float var = 1.0f;
        if (eval) var = clodw_variance(img, sq, e, e_lt, e_dw, e_dh, area, a.signed_mean != 0u);
        if (STAGE_TREE) {
            int32_t ptr = eval ? (int32_t)stages[0].order : -3;   // -1 accepted, -2 rejected, -3 not evaluated
            float last_sum = 0.0f;
            for (uint32_t oi = 0; oi < a.n_order; ++oi) {
                const uint32_t s = stages[oi].order;
                const bool here = ptr == (int32_t)s;
                if (__ballot(here) == 0ull) continue;
                if (here) {
                    last_sum = clodw_stage_sum<TREES>(img, table + stages[s].first_node, stages[s].n_nodes, off, var);
                    ptr = last_sum >= stages[s].threshold ? stages[s].on_pass : stages[s].on_fail;
                }
            }
            if (eval) a.out[p.index] = ClodPointResult{ptr == -1 ? 1 : 0, var, last_sum, 0};
            continue;
        }
        if (a.start_stage >= a.n_stages) {   // the stage loop does not run: exit_stage keeps its 1 (clod.cpp:752)
            if (eval) a.out[p.index] = ClodPointResult{1, var, 0.0f, 0};
            continue;
        }
        const unsigned long long em = __ballot(eval);
        uint32_t n = (uint32_t)__popcll(em);
        if (eval) q[mbcnt(em)] = ClodQEntry{off, p.index, var};
        __builtin_amdgcn_wave_barrier();
        for (uint32_t s = a.start_stage; s < a.n_stages && n != 0u; ++s) {
            kptr<NodeRecDev> tab = table + stages[s].first_node;
            const uint32_t n_nodes = stages[s].n_nodes;
            const float thr = stages[s].threshold;
            const bool have = lane < n, last = s + 1u == a.n_stages;
            const ClodQEntry en = q[have ? lane : 0u];
            float ssum = 0.0f;
            if (have) ssum = clodw_stage_sum<TREES>(img, tab, n_nodes, en.off, en.var);
            const bool pass = have && ssum >= thr;   // `if(stage_sum < stage.threshold) exit_stage = -stage_index` (clod.cpp:769-770)
            if (have && (!pass || last) && en.index < a.n_points) a.out[en.index] = ClodPointResult{pass ? 1 : -(int32_t)s, en.var, ssum, 0};
            const unsigned long long pm = __ballot(pass);
            __builtin_amdgcn_wave_barrier();
            if (pass) q[mbcnt(pm)] = en;
            n = (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
        }
        __builtin_amdgcn_wave_barrier();
    }
}

int launch_clod_points_pass(const ClodPointArgs& a, bool trees, bool stage_tree, int n_blocks, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    dim3 g(n_blocks), b(CLOD_POINT_WAVES * 64);
    if (stage_tree) {
        if (trees) hipLaunchKernelGGL((clod_points_pass<true, true>), g, b, 0, stream, a);
        else       hipLaunchKernelGGL((clod_points_pass<false, true>), g, b, 0, stream, a);
    } else {
        if (trees) hipLaunchKernelGGL((clod_points_pass<true, false>), g, b, 0, stream, a);
        else       hipLaunchKernelGGL((clod_points_pass<false, false>), g, b, 0, stream, a);
    }
    return (int)hipGetLastError();
}

}  // namespace vj
