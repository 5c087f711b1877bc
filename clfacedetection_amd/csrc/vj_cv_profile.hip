// gfx950 kernels of the OpenCV arithmetic profile: cvHaarDetectObjects' scale-cascade path as the
// reference keeps it in tempcv.cpp (a private copy of OpenCV 2.4.2 haar.cpp; CV_HAAR_USE_SSE is commented
// out at :28-36, so the scalar branches are the specification) —
//   cvRunHaarClassifierCascadeSum   tempcv.cpp:795-972   f64 variance and stage sums, border rule, three paths:
//       stage tree (:834-861), stump cascade (:863-945, per-stage two_rects), general trees (:947-964)
//   icvEvalHidHaarClassifier        tempcv.cpp:771-792   sum < t ? left : right, int * float products
//   HaarDetectObjects_ScaleCascade_Invoker  :1116-1185    x = cvRound(ix * ystep), ixstep = result != 0 ? 1 : 2
//   tilted rectangles               tempcv.cpp:743-750   four corners in the tilted integral image
// Second arithmetic profile of the library; the clod profile (vj_kernels.hip) is the
// contract of the headline path.  MUST be compiled with -ffp-contract=off.
//
// One wave walks one window row.  The sequential "skip the next window after a reject" rule is a
// recurrence over the row, e[i] = !(e[i-1] && f[i-1]); because a window that follows a non-reject is always
// visited, e[i] only depends on the PARITY of the run of rejects that ends at i-1 (f computed for
// every grid position), which a wave gets from one __ballot per 64 positions plus one carry bit.  For linear
// cascades only a stage-0 reject skips (the later stages return -i != 0), so f is the stage-0 verdict and the
// later stages run on the visited survivors; a stage tree returns 0 on ANY reject, so there f is the verdict of
// the whole tree, evaluated for every grid position.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_cv_window.hpp"

namespace vj {

constexpr uint32_t CV_TREE_SEG_GROUPS = 16;   // stage trees: a row is resolved in segments of 16 x 64 grid positions
// (node, tree and stage sums, cv_tail_stage, cv_flush_to, cv_visited: vj_cv_window.hpp, shared with vj_cv_biggest.hip)

// 16- / 24-byte entries to and from the per-wave fail list in global memory.  The list is written with plain stores and read
// back by the SAME wave: the reads go to the L2 (agent-scope relaxed loads: sc1), behind a drain of the wave's stores.
template <typename E>
__device__ __forceinline__ E cv_load_entry_l2(const E* p) {
    static_assert(sizeof(E) % 8 == 0, "entries are multiples of 8 bytes");
    E e;
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(&e);
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(p);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(E) / 8u; ++k) dst[k] = __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return e;
}

// Sweep the chains of `ch` over the windows q[0, n) (LDS; entries carry .off and .vnf), all of one scale.  `final_(e, mine,
// accepted)` is called in wave-uniform control flow for windows whose walk ends: lanes with `mine` set hold such a window.
// `fail_g`: room for the population in global memory (this wave's own).
// SUMS (ROC calls): final_ takes a fourth argument, the sum of the stage that ended the walk; who passes a chain's last stage is
// handed to it right there, where the lane still holds that sum, instead of after the compaction.
template <bool TREES, bool SUMS = false, typename E, typename Final>
__device__ __forceinline__ void cv_chain_sweep(const CvChainDev& ch, kptr<StageDev> stages, rsrc_t img, rsrc_t timg, bool tail_ok, const uint32_t* table_g,
                                               kptr<NodeRecDev> table, E* q, uint32_t n, E* fail_g, unsigned long long* masks, uint32_t lane,
                                               Final final_) {
    for (uint32_t k = 0; k < ch.n && n != 0u; ++k) {
        const bool chained = ((ch.chained >> k) & 1u) != 0u;
        uint32_t nf = 0;
        for (uint32_t pos = ch.begin[k]; pos < ch.end[k] && n != 0u; ++pos) {
            const uint32_t s = stages[pos].order;
            const uint32_t first_node = stages[s].first_node, n_nodes = stages[s].n_nodes;
            const double thr = (double)stages[s].threshold;
            kptr<NodeRecDev> tab = table + first_node;
            if (!TREES && tail_ok && n <= ch.tail_max && n_nodes >= 16u && n_nodes <= CV_TAIL_BLOCKS * 64u) {   // uniform
                unsigned long long pm;
                double ssum = 0.0;
                if constexpr (SUMS) {
                    ssum = cv_tail_stage_sum(img, table_g + (size_t)first_node * 16u, tab, n_nodes, q, n, masks, lane);
                    pm = __ballot(lane < n && ssum >= thr);
                } else {
                    pm = cv_tail_stage(img, table_g + (size_t)first_node * 16u, tab, n_nodes, thr, q, n, masks, lane);
                }
                const bool have = lane < n;
                const E e = q[have ? lane : 0u];
                bool pass = ((pm >> lane) & 1ull) != 0ull;
                const unsigned long long fm = __ballot(have && !pass);
                if (fm != 0ull) {
                    if (chained) {
                        if (have && !pass) fail_g[nf + mbcnt(fm)] = e;
                        nf += (uint32_t)__popcll(fm);
                    } else {
                        if constexpr (SUMS) final_(e, have && !pass, false, ssum);
                        else final_(e, have && !pass, false);
                    }
                }
                if constexpr (SUMS) {
                    if (pos + 1u == ch.end[k]) {   // the chain's last stage: its passers are accepted, with this sum
                        if (pm != 0ull) final_(e, pass, true, ssum);
                        pass = false;
                        pm = 0ull;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                if (pass) q[mbcnt(pm)] = e;
                n = (uint32_t)__popcll(pm);
                __builtin_amdgcn_wave_barrier();
                continue;
            }
            uint32_t m = 0;
            for (uint32_t base = 0; base < n; base += 64u) {
                const uint32_t i = base + lane;
                const bool act = i < n;
                const E e = q[act ? i : 0u];
                double ssum = 0.0;
                bool pass = false;
                if (act) {
                    if (TREES) pass = (ssum = cv_stage_sum<true, false>(img, timg, tab, n_nodes, e.off, e.vnf)) >= thr;
                    else if (tail_ok) pass = (ssum = cv_stage_sum_pairs(img, tab, n_nodes, e.off, e.vnf)) >= thr;
                    else pass = (ssum = cv_stage_sum<false, false>(img, timg, tab, n_nodes, e.off, e.vnf)) >= thr;   // (tilted features)
                }
                const unsigned long long fm = __ballot(act && !pass);
                if (fm != 0ull) {
                    if (chained) {
                        if (act && !pass) fail_g[nf + mbcnt(fm)] = e;
                        nf += (uint32_t)__popcll(fm);
                    } else {
                        if constexpr (SUMS) final_(e, act && !pass, false, ssum);
                        else final_(e, act && !pass, false);
                    }
                }
                if constexpr (SUMS) {
                    if (pos + 1u == ch.end[k]) {   // the chain's last stage: its passers are accepted, with this sum
                        if (__ballot(pass) != 0ull) final_(e, pass, true, ssum);
                        pass = false;
                    }
                }
                const unsigned long long mask = __ballot(pass);
                __builtin_amdgcn_wave_barrier();   // every lane has read its entry before any lane overwrites
                if (pass) q[m + mbcnt(mask)] = e;
                m += (uint32_t)__popcll(mask);
                __builtin_amdgcn_wave_barrier();
            }
            n = m;
        }
        if constexpr (!SUMS) {
            for (uint32_t base = 0; base < n; base += 64u) {   // passed the chain's last stage: accepted
                const bool act = base + lane < n;
                const E e = q[act ? base + lane : 0u];
                final_(e, act, true);
            }
        }
        if (!chained) break;
        // the chain's rejects are the next chain's population
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < nf; i += 64u) q[i] = cv_load_entry_l2(fail_g + i);
        __builtin_amdgcn_wave_barrier();
        n = nf;
    }
}

template <bool TREES, bool COUNT>
__device__ __forceinline__ void cv_flush(const CvArgs& a, rsrc_t img, rsrc_t timg, kptr<NodeRecDev> table, CvQEntry* q, uint32_t& n,
                                         uint32_t slot, uint32_t frame, uint32_t lane) {
    cv_flush_to<TREES, COUNT>(a, img, timg, table, q, n, lane, [&](const CvQEntry* qq, uint32_t m) {
        uint32_t g = 0;
        if (lane == 0) g = atomicAdd(a.det_count, m);
        g = __builtin_amdgcn_readfirstlane(g);
        for (uint32_t i = lane; i < m; i += 64u)
            if (g + i < a.det_cap) a.det[g + i] = CvDet{qq[i].xy & 0xffffu, qq[i].xy >> 16, slot, frame};
    });
}


// (cv_pruned: vj_devutil.hpp, shared with the prune-bitmap kernel of the tile scales, vj_canny.hip)
// PRUNE: CV_HAAR_DO_CANNY_PRUNING.  A pruned position is a "zero" of the walk like a reject (ixstep = 2) but is not evaluated;
// the test comes before the border rule.  PRUNE = false compiles to the kernels of flags = 0.
// EXH: CV_HAAR_SCALE_IMAGE's exhaustive grid (HaarDetectObjects_ScaleImage_Invoker, tempcv.cpp:1079-1102).  A "scale" is a level of
// the image pyramid inside the canvas (rows[r].count: element offset of its origin in the canvas's integral images), ystep is 1 or 2,
// EVERY grid position is visited — a reject skips nothing — and the border rule cannot fire (x < level width - window width).
// Positions and detections are in the level's own coordinates (the host scales them by the level's factor).  Per-window arithmetic:
// the same code.  EXH = false compiles to the kernels as they were.
// ROC (with EXH): cvHaarDetectObjectsForROC's outputRejectLevels (tempcv.cpp:1084-1095).  The records are CvRocDet:
// a linear cascade reports from its sweep of the later stages (cv_flush_roc); a stage tree reports an accepted window where the stage
// whose pass ended its walk was summed — every position is visited, so no walk has to be resolved first.  ROC = false compiles to
// the kernels as they were.
template <bool TREES, bool COUNT, bool STAGE_TREE, bool PRUNE = false, bool EXH = false, bool ROC = false>
__global__ __launch_bounds__(CV_WAVES_PER_BLOCK * 64) void cv_profile_pass(CvArgs a) {
    static_assert(!ROC || (EXH && !PRUNE), "reject levels exist on the exhaustive grid only");
    __shared__ CvQEntry lds_q[CV_WAVES_PER_BLOCK * CV_QCAP];
    __shared__ unsigned long long lds_words[CV_WAVES_PER_BLOCK][2][STAGE_TREE ? CV_TREE_SEG_GROUPS : 1];   // stage trees: verdict bits of a row segment
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CvQEntry* q = lds_q + wib * CV_QCAP;
    const uint32_t rank = blockIdx.x * CV_WAVES_PER_BLOCK + wib;
    (void)rank;
    kptr<CvScaleDev> scales = as_k(a.scales);
    kptr<UnitDev> rows = as_k(a.rows);
    kptr<StageDev> stages = as_k(a.stages);
    const uint32_t frame_bytes4 = a.frame_elems * 4u;
    const rsrc_t img = make_rsrc(a.sum, a.n_frames * frame_bytes4);
    const rsrc_t timg = make_rsrc(a.tilted != nullptr ? a.tilted : a.sum, a.n_frames * frame_bytes4);
    const rsrc_t eimg = make_rsrc(PRUNE ? a.edge_sum : a.sum, a.n_frames * frame_bytes4);
    const uint32_t total = a.n_rows * a.n_frames;

    // Blocks are dealt round-robin over the 8 XCDs (observed placement; speed only): the waves that share an XCD — and its
    // 4 MiB L2 — walk one contiguous eighth of the (frame, scale, row) list, i.e. neighbouring rows of the same frame's
    // integral images at the same time, instead of rows of every frame in flight (fabric traffic of this kernel: 1.6 TB
    // per launch on 64 x 1080p with the strided assignment).
    uint32_t u_first = rank, u_end = total, u_step = a.total_waves;
    if (gridDim.x >= 8u) {
        const uint32_t xcd = blockIdx.x & 7u;
        const uint32_t u_begin = (uint32_t)((unsigned long long)total * xcd / 8u);
        u_end = (uint32_t)((unsigned long long)total * (xcd + 1u) / 8u);
        u_step = ((gridDim.x - xcd + 7u) >> 3) * CV_WAVES_PER_BLOCK;
        u_first = u_begin + (blockIdx.x >> 3) * CV_WAVES_PER_BLOCK + wib;
    }
    for (uint32_t u = u_first; u < u_end; u += u_step) {
        const uint32_t frame = u / a.n_rows;
        const uint32_t r = u - frame * a.n_rows;
        const uint32_t slot = rows[r].scale, iy = rows[r].first;
        const uint32_t org = EXH ? rows[r].count : 0u;
        const double ystep = scales[slot].ystep, inv_area = scales[slot].inv_area;
        const uint32_t win_w = scales[slot].win_w, win_h = scales[slot].win_h, end_x = scales[slot].end_x;
        const uint32_t q0 = scales[slot].q0, q1 = scales[slot].q1, q2 = scales[slot].q2, q3 = scales[slot].q3;
        kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(a.table)) + scales[slot].table_first;
        const rsrc_t sq_f = make_rsrc(a.sqsum + (size_t)frame * a.frame_elems, frame_bytes4 * 2u);
        const uint32_t frame_bytes = frame * frame_bytes4;
        const uint32_t y = (uint32_t)cv_round((double)iy * ystep);
        const bool row_border = !EXH && y + win_h >= a.sum_h;  // pt.y + height >= sum.height -> -1 (tempcv.cpp:817-820)
        uint32_t e0 = 0, e1 = 0, e2 = 0, e3 = 0;
        if (PRUNE) {
            kptr<CvPruneDev> pr = as_k(a.prune);
            e0 = pr[slot].p0 * 4u;
            e1 = pr[slot].p1 * 4u;
            e2 = pr[slot].p2 * 4u;
            e3 = pr[slot].p3 * 4u;
        }
        const double thr0 = (double)stages[0].threshold;
        uint32_t carry = 0;   // parity of the run of rejects that ends at the last position seen
        uint32_t n_q = 0;
        if (STAGE_TREE && !COUNT) {
            // Stage tree, every grid position (the skip rule needs the whole tree's verdict everywhere), but not every
            // position in lockstep to the end: the linear prefix runs on the dense groups; who is still inside the tree
            // afterwards (a few percent) waits in the wave's queue with its target stage, and a FULL chunk of those
            // sweeps the rest of the tree at a time — 64 lanes of survivors pay for the chains instead of every group
            // of 64 positions paying for its deepest lane.  The verdict bits of a row segment (reject / accept words)
            // sit in LDS until every position of the segment has one; then the walk is resolved group by group.
            unsigned long long* Fw = lds_words[wib][0];
            unsigned long long* Aw = lds_words[wib][1];
            uint32_t prefix = 0;   // leading stages of the sweep order that reject outright and pass to the next one
            while (prefix + 1u < a.n_order && stages[stages[prefix].order].on_fail == -2 &&
                   stages[stages[prefix].order].on_pass == (int32_t)stages[prefix + 1u].order)
                ++prefix;
            CvQEntry* fail_g = reinterpret_cast<CvQEntry*>(a.fail_scratch) + (size_t)rank * CV_QCAP;
            auto drain = [&](uint32_t seg0) {
                if (a.chains.n != 0u) {
                    // the tree is made of chains: compacting sweeps (every queued window sits at the first stage of chain 0)
                    if constexpr (ROC)
                        cv_chain_sweep<TREES, true>(a.chains, stages, img, timg, a.tilted == nullptr, a.table + (size_t)scales[slot].table_first * 16u, table, q,
                                                    n_q, fail_g, reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX), lane,
                                                    [&](const CvQEntry& e, bool mine, bool accepted, double ssum) {
                                                        if (accepted)   // (uniform)
                                                            cv_roc_report(a, mine, (uint32_t)cv_round((double)(e.xy & 0xffffu) * ystep), y, slot, frame,
                                                                          a.n_stages, ssum, lane);
                                                    });
                    else
                    cv_chain_sweep<TREES>(a.chains, stages, img, timg, a.tilted == nullptr, a.table + (size_t)scales[slot].table_first * 16u, table, q, n_q,
                                          fail_g, reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX), lane,
                                          [&](const CvQEntry& e, bool mine, bool accepted) {
                                              if (mine) {
                                                  const uint32_t rel = (e.xy & 0xffffu) - seg0;
                                                  atomicOr((accepted ? Aw : Fw) + (rel >> 6), 1ull << (rel & 63u));
                                              }
                                          });
                    n_q = 0;
                    __builtin_amdgcn_wave_barrier();
                    return;
                }
                for (uint32_t base = 0; base < n_q; base += 64u) {
                    const bool act = base + lane < n_q;
                    const CvQEntry e = q[act ? base + lane : 0u];
                    int32_t ptr = act ? (int32_t)(e.xy >> 16) : -3;
                    double last_sum = 0.0;   // (ROC) of the last stage this window was in
                    for (uint32_t oi = prefix; oi < a.n_order; ++oi) {
                        const uint32_t s = stages[oi].order;
                        const bool here = ptr == (int32_t)s;
                        if (__ballot(here) == 0ull) continue;
                        if (here) {
                            const double ssum = cv_stage_sum<TREES, false>(img, timg, table + stages[s].first_node, stages[s].n_nodes, e.off, e.vnf);
                            const bool pass = ssum >= (double)stages[s].threshold;
                            ptr = pass ? stages[s].on_pass : stages[s].on_fail;
                            if (ROC) last_sum = ssum;
                        }
                    }
                    if constexpr (ROC) {
                        cv_roc_report(a, act && ptr == -1, (uint32_t)cv_round((double)(e.xy & 0xffffu) * ystep), y, slot, frame, a.n_stages, last_sum, lane);
                        continue;
                    }
                    if (act) {
                        const uint32_t rel = (e.xy & 0xffffu) - seg0;
                        if (ptr == -2) atomicOr(Fw + (rel >> 6), 1ull << (rel & 63u));
                        else if (ptr == -1) atomicOr(Aw + (rel >> 6), 1ull << (rel & 63u));
                    }
                }
                n_q = 0;
                __builtin_amdgcn_wave_barrier();
            };
            for (uint32_t seg0 = 0; seg0 < end_x; seg0 += CV_TREE_SEG_GROUPS * 64u) {
                const uint32_t seg_end = min(end_x, seg0 + CV_TREE_SEG_GROUPS * 64u);
                for (uint32_t ix0 = seg0; ix0 < seg_end; ix0 += 64u) {
                    const uint32_t ix = ix0 + lane;
                    const bool valid = ix < end_x;
                    const uint32_t x = (uint32_t)cv_round((double)(valid ? ix : 0u) * ystep);
                    const bool border = row_border || (!EXH && x + win_w >= a.stride);
                    const uint32_t po = org + y * a.stride + x;
                    const uint32_t off = frame_bytes + po * 4u;
                    double vnf = 1.0;
                    const bool pruned = PRUNE && valid && cv_pruned(eimg, img, off, e0, e1, e2, e3);
                    const bool eval = valid && !border && !pruned;
                    if (eval) {
                        const int32_t isum = (int32_t)(ld_u32(img, off, q0 * 4u) - ld_u32(img, off, q1 * 4u) - ld_u32(img, off, q2 * 4u) +
                                                       ld_u32(img, off, q3 * 4u));
                        const uint64_t qq = ld_u64(sq_f, po * 8u, q0 * 8u) - ld_u64(sq_f, po * 8u, q1 * 8u) - ld_u64(sq_f, po * 8u, q2 * 8u) +
                                            ld_u64(sq_f, po * 8u, q3 * 8u);
                        const double mean = (double)isum * inv_area;
                        vnf = (double)qq;
                        vnf = vnf * inv_area - mean * mean;
                        vnf = vnf >= 0.0 ? sqrt(vnf) : 1.0;
                    }
                    int32_t ptr = eval ? (int32_t)stages[0].order : -3;   // -1 accepted, -2 rejected, -3 not evaluated
                    double last_sum = 0.0;   // (ROC) of the last stage this window was in
                    for (uint32_t oi = 0; oi < prefix; ++oi) {
                        const uint32_t s = stages[oi].order;
                        const bool here = ptr == (int32_t)s;
                        if (__ballot(here) == 0ull) break;   // (nobody left in the prefix)
                        if (here) {
                            const double ssum = cv_stage_sum<TREES, false>(img, timg, table + stages[s].first_node, stages[s].n_nodes, off, vnf);
                            const bool pass = ssum >= (double)stages[s].threshold;
                            ptr = pass ? stages[s].on_pass : stages[s].on_fail;
                            if (ROC) last_sum = ssum;
                        }
                    }
                    if constexpr (ROC) cv_roc_report(a, ptr == -1, x, y, slot, frame, a.n_stages, last_sum, lane);   // (accepted inside the prefix)
                    const unsigned long long fm = __ballot(ptr == -2 || pruned), am = __ballot(ptr == -1), wm = __ballot(ptr >= 0);
                    if (lane == 0) {
                        Fw[(ix0 - seg0) >> 6] = fm;
                        Aw[(ix0 - seg0) >> 6] = am;
                    }
                    if (ptr >= 0) q[n_q + mbcnt(wm)] = CvQEntry{off, ix | ((uint32_t)ptr << 16), vnf};
                    n_q += (uint32_t)__popcll(wm);
                    __builtin_amdgcn_wave_barrier();
                    if (n_q > (uint32_t)CV_QCAP - 64u) drain(seg0);
                }
                drain(seg0);
                // every position of the segment has its verdict: the sequential walk, group by group (ROC: reported already)
                for (uint32_t ix0 = seg0; ix0 < seg_end && !ROC; ix0 += 64u) {
                    const uint32_t ix = ix0 + lane;
                    const unsigned long long F = Fw[(ix0 - seg0) >> 6], A = Aw[(ix0 - seg0) >> 6];
                    const bool visited = EXH ? ix < end_x : cv_visited(F, lane, min(64u, end_x - ix0), carry);
                    const bool hit = visited && ((A >> lane) & 1ull) != 0ull;
                    const unsigned long long hm = __ballot(hit);
                    if (hm != 0ull) {
                        uint32_t g = 0;
                        if (lane == 0) g = atomicAdd(a.det_count, (uint32_t)__popcll(hm));
                        g = __builtin_amdgcn_readfirstlane(g);
                        const uint32_t pos = g + mbcnt(hm);
                        if (hit && pos < a.det_cap) a.det[pos] = CvDet{(uint32_t)cv_round((double)ix * ystep), y, slot, frame};
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            continue;
        }
        for (uint32_t ix0 = 0; ix0 < end_x; ix0 += 64u) {
            const uint32_t ix = ix0 + lane;
            const bool valid = ix < end_x;
            const uint32_t x = (uint32_t)cv_round((double)(valid ? ix : 0u) * ystep);
            const bool border = row_border || (!EXH && x + win_w >= a.stride);
            const uint32_t po = org + y * a.stride + x;
            const uint32_t off = frame_bytes + po * 4u;
            double vnf = 1.0;
            const bool pruned = PRUNE && valid && cv_pruned(eimg, img, off, e0, e1, e2, e3);
            const bool eval = valid && !border && !pruned;
            if (eval) {
                const int32_t isum = (int32_t)(ld_u32(img, off, q0 * 4u) - ld_u32(img, off, q1 * 4u) - ld_u32(img, off, q2 * 4u) +
                                               ld_u32(img, off, q3 * 4u));
                const uint64_t qq = ld_u64(sq_f, po * 8u, q0 * 8u) - ld_u64(sq_f, po * 8u, q1 * 8u) - ld_u64(sq_f, po * 8u, q2 * 8u) +
                                    ld_u64(sq_f, po * 8u, q3 * 8u);
                const double mean = (double)isum * inv_area;
                vnf = (double)qq;
                vnf = vnf * inv_area - mean * mean;
                vnf = vnf >= 0.0 ? sqrt(vnf) : 1.0;
            }
            const uint32_t n_valid = min(64u, end_x - ix0);
            if (STAGE_TREE) {
                // the whole stage tree for every grid position (tempcv.cpp:834-861): every queued lane carries the
                // stage it visits next; stages are swept once in a topological order of the pass / fail graph
                int32_t ptr = eval ? (int32_t)stages[0].order : -3;   // -1 accepted, -2 rejected, -3 not evaluated
                unsigned long long entered = 0ull;
                double last_sum = 0.0;   // (ROC) of the last stage this window was in
                for (uint32_t oi = 0; oi < a.n_order; ++oi) {
                    const uint32_t s = stages[oi].order;
                    const bool here = ptr == (int32_t)s;
                    if (__ballot(here) == 0ull) continue;
                    if (here) {
                        const double ssum = cv_stage_sum<TREES, false>(img, timg, table + stages[s].first_node, stages[s].n_nodes, off, vnf);
                        const bool pass = ssum >= (double)stages[s].threshold;
                        ptr = pass ? stages[s].on_pass : stages[s].on_fail;
                        entered |= 1ull << s;
                        if (ROC) last_sum = ssum;
                    }
                }
                const unsigned long long F = __ballot(ptr == -2 || pruned);
                const bool visited = EXH ? valid : cv_visited(F, lane, n_valid, carry);
                if (COUNT) {
                    const unsigned long long vm = __ballot(visited);
                    if (lane == 0) atomicAdd(a.stage_entered + VJ_MAX_STAGES_DEV, (unsigned long long)__popcll(vm));
                    for (uint32_t s = 0; s < a.n_stages; ++s) {
                        const unsigned long long em = __ballot(visited && ((entered >> s) & 1ull) != 0ull);
                        if (lane == 0 && em != 0ull) atomicAdd(a.stage_entered + s, (unsigned long long)__popcll(em));
                    }
                }
                if constexpr (ROC) {
                    cv_roc_report(a, visited && ptr == -1, x, y, slot, frame, a.n_stages, last_sum, lane);
                    continue;
                }
                const unsigned long long am = __ballot(visited && ptr == -1);
                if (am != 0ull) {
                    uint32_t g = 0;
                    if (lane == 0) g = atomicAdd(a.det_count, (uint32_t)__popcll(am));
                    g = __builtin_amdgcn_readfirstlane(g);
                    const uint32_t pos = g + mbcnt(am);
                    if (visited && ptr == -1 && pos < a.det_cap) a.det[pos] = CvDet{x, y, slot, frame};
                }
                continue;
            }
            bool fail0 = false;
            if (eval)
                fail0 = !(cv_stage_sum_mode<TREES>(img, timg, table + stages[0].first_node, stages[0].n_nodes, off, vnf, stages[0].cv_f64, a.tree2) >= thr0);
            // which positions does the sequential walk visit?  parity of the reject run below each lane
            const unsigned long long F = __ballot(fail0 || pruned);
            const bool visited = EXH ? valid : cv_visited(F, lane, n_valid, carry);
            const bool pass0 = visited && !border && !fail0 && !pruned;
            if (COUNT) {
                const unsigned long long vm = __ballot(visited), em = __ballot(visited && !border && !pruned);
                if (lane == 0) {
                    atomicAdd(a.stage_entered + VJ_MAX_STAGES_DEV, (unsigned long long)__popcll(vm));
                    atomicAdd(a.stage_entered + 0, (unsigned long long)__popcll(em));
                }
            }
            const unsigned long long pm = __ballot(pass0);
            if (pass0) q[n_q + mbcnt(pm)] = CvQEntry{off, x | (y << 16), vnf};
            n_q += (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
            if (n_q > (uint32_t)CV_QCAP - 64u) {
                if constexpr (ROC) cv_flush_roc<TREES, COUNT>(a, img, timg, table, q, n_q, slot, frame, lane);
                else cv_flush<TREES, COUNT>(a, img, timg, table, q, n_q, slot, frame, lane);
            }
        }
        if (!STAGE_TREE && n_q != 0u) {
            if constexpr (ROC) cv_flush_roc<TREES, COUNT>(a, img, timg, table, q, n_q, slot, frame, lane);
            else cv_flush<TREES, COUNT>(a, img, timg, table, q, n_q, slot, frame, lane);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

template <bool TREES, bool STAGE_TREE, bool PRUNE = false, bool EXH = false, bool ROC = false>
static void cv_launch(const CvArgs& a, bool count, dim3 g, dim3 b, hipStream_t stream) {
    if (count) hipLaunchKernelGGL((cv_profile_pass<TREES, true, STAGE_TREE, PRUNE, EXH, ROC>), g, b, 0, stream, a);
    else       hipLaunchKernelGGL((cv_profile_pass<TREES, false, STAGE_TREE, PRUNE, EXH, ROC>), g, b, 0, stream, a);
}

int launch_cv_profile_pass(const CvArgs& a, bool trees, bool count, bool stage_tree, int n_blocks, void* stream_, bool prune, bool exhaustive,
                           bool roc) {
    hipStream_t stream = (hipStream_t)stream_;
    dim3 g(n_blocks), b(CV_WAVES_PER_BLOCK * 64);
    if (roc) {   // (the host asks for reject levels on the exhaustive grid only)
        if (!exhaustive || prune) return (int)hipErrorInvalidValue;
        if (stage_tree) {
            if (trees) cv_launch<true, true, false, true, true>(a, count, g, b, stream);
            else       cv_launch<false, true, false, true, true>(a, count, g, b, stream);
        } else {
            if (trees) cv_launch<true, false, false, true, true>(a, count, g, b, stream);
            else       cv_launch<false, false, false, true, true>(a, count, g, b, stream);
        }
        return (int)hipGetLastError();
    }
    if (exhaustive) {   // (never together with pruning: the scale-image branch does not read doCannyPruning)
        if (stage_tree) {
            if (trees) cv_launch<true, true, false, true>(a, count, g, b, stream);
            else       cv_launch<false, true, false, true>(a, count, g, b, stream);
        } else {
            if (trees) cv_launch<true, false, false, true>(a, count, g, b, stream);
            else       cv_launch<false, false, false, true>(a, count, g, b, stream);
        }
        return (int)hipGetLastError();
    }
    if (prune) {
        if (stage_tree) {
            if (trees) cv_launch<true, true, true>(a, count, g, b, stream);
            else       cv_launch<false, true, true>(a, count, g, b, stream);
        } else {
            if (trees) cv_launch<true, false, true>(a, count, g, b, stream);
            else       cv_launch<false, false, true>(a, count, g, b, stream);
        }
        return (int)hipGetLastError();
    }
    if (stage_tree) {
        if (trees) cv_launch<true, true>(a, count, g, b, stream);
        else       cv_launch<false, true>(a, count, g, b, stream);
    } else {
        if (trees) cv_launch<true, false>(a, count, g, b, stream);
        else       cv_launch<false, false>(a, count, g, b, stream);
    }
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------ stage trees whose prefix ran on LDS tiles
// cv_tile_pass<2> (vj_cv_tile.hip) evaluated the tree's linear prefix on every grid window of the small scales and queued
// the survivors.  cv_tree_walk takes them the rest of the way (tempcv.cpp:834-861: pass -> child, fail -> the next
// sibling up the tree, else reject; the stages are swept once in topological order, every lane carrying the stage it
// visits next) and sets each window's reject or accept bit; after skip_resolve has turned the reject bits of every
// window row into visited bits, cv_tree_emit reports the accepted windows the sequential walk visits.
__global__ __launch_bounds__(256) void cv_tree_walk(CvTreeArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvScaleDev> scales = as_k(a.scales);
    const rsrc_t img = make_rsrc(a.sum, a.sum_bytes);
    const uint32_t n = min(*a.tq_count, a.tq_cap);
    for (uint32_t base = wave * 64u; base < n; base += n_waves * 64u) {
        const bool act = base + lane < n;
        const CvTreeEntry e = a.tq[act ? base + lane : base];
        const uint32_t my_slot = e.bit_slot >> 8;
        int32_t ptr = act ? stages[stages[a.prefix - 1u].order].on_pass : -3;   // what passing the prefix's last stage leads to
        unsigned long long todo = __ballot(act);
        while (todo != 0ull) {   // the entries of one scale at a time: the feature table must be wave-uniform
            const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)my_slot, (int)__builtin_ctzll(todo));
            const bool mine = act && my_slot == slot;
            todo &= ~__ballot(mine);
            kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(a.table)) + scales[slot].table_first;
            for (uint32_t oi = a.prefix; oi < a.n_order; ++oi) {
                const uint32_t s = stages[oi].order;
                const bool here = mine && ptr == (int32_t)s;
                if (__ballot(here) == 0ull) continue;
                if (here) {
                    const bool pass = cv_stage_sum<false, false>(img, img, table + stages[s].first_node, stages[s].n_nodes, e.off, e.vnf) >=
                                      (double)stages[s].threshold;
                    ptr = pass ? stages[s].on_pass : stages[s].on_fail;
                }
            }
        }
        if (act) {
            const unsigned long long bit = 1ull << (e.bit_slot & 63u);
            if (ptr == -1) atomicOr(a.accept + e.word, bit);
            else atomicOr(a.reject + e.word, bit);   // -2, or a stage the sweep order never reaches: rejected
        }
    }
}

__global__ __launch_bounds__(256) void cv_tree_emit(CvTreeArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    kptr<UnitDev> segs = as_k(a.segs);
    kptr<CvScaleDev> scales = as_k(a.scales);
    const uint32_t total = a.n_segs * a.n_frames;
    for (uint32_t u = wave; u < total; u += n_waves) {
        const uint32_t frame = u / a.n_segs, r = u - frame * a.n_segs;
        const uint32_t slot = segs[r].scale, first = segs[r].first, wpr = segs[r].count;
        const uint32_t iy = (first - scales[slot].bits_base) / wpr;
        const double ystep = scales[slot].ystep;
        const uint32_t y = (uint32_t)cv_round((double)iy * ystep);
        const size_t w0 = (size_t)frame * a.bits_frame_words + first;
        for (uint32_t w = 0; w < wpr; ++w) {
            const unsigned long long hits = a.accept[w0 + w] & a.reject[w0 + w];   // (reject holds the VISITED bits by now)
            if (hits == 0ull) continue;   // uniform
            const bool hit = ((hits >> lane) & 1ull) != 0ull;
            uint32_t g = 0;
            if (lane == 0) g = atomicAdd(a.det_count, (uint32_t)__popcll(hits));
            g = __builtin_amdgcn_readfirstlane(g);
            const uint32_t pos = g + mbcnt(hits);
            if (hit && pos < a.det_cap) a.det[pos] = CvDet{(uint32_t)cv_round((double)(w * 64u + lane) * ystep), y, slot, frame};
        }
    }
}

// The same for a tree made of chains (CvTreeArgs::chains): one sub-queue per scale, so a wave draws chunks of CV_TQ_CHUNK windows
// of ONE scale and sweeps the chains over them like a linear cascade (cv_chain_sweep).
__global__ __launch_bounds__(256) void cv_tree_chain_pass(CvTreeArgs a) {
    __shared__ CvTreeEntry lds_q[4 * CV_TQ_CHUNK];
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CvTreeEntry* q = lds_q + wib * CV_TQ_CHUNK;
    CvTreeEntry* fail_g = reinterpret_cast<CvTreeEntry*>(a.fail_scratch) + (size_t)(blockIdx.x * 4u + wib) * CV_TQ_CHUNK;
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvScaleDev> scales = as_k(a.scales);
    kptr<uint32_t> counts = as_k(a.tq_count);
    const rsrc_t img = make_rsrc(a.sum, a.sum_bytes);
    while (true) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.ticket, 1u);
        t = __builtin_amdgcn_readfirstlane(t);
        // ticket -> (scale, chunk): the tile scales in order
        uint32_t slot = 0, n_here = 0;
        uint64_t first = 0;
        for (; slot < a.n_scales; ++slot) {
            if (scales[slot].tile_th == 0u) continue;
            const uint64_t cap = cv_tq_cap(scales[slot].end_x, scales[slot].end_y, a.n_frames, a.tq_shift);
            const uint32_t cnt = (uint32_t)min((uint64_t)counts[scales[slot].tq_slot], cap);
            const uint32_t n_chunks = (cnt + a.chunk - 1u) / a.chunk;
            if (t < n_chunks) {
                first = cv_tq_first(scales[slot].tq_win_first, scales[slot].tq_slot, a.n_frames, a.tq_shift) + (uint64_t)t * a.chunk;
                n_here = min(a.chunk, cnt - t * a.chunk);
                break;
            }
            t -= n_chunks;
        }
        if (slot == a.n_scales) return;   // every chunk is taken
        for (uint32_t i = lane; i < n_here; i += 64u) q[i] = a.tq[first + i];
        __builtin_amdgcn_wave_barrier();
        kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(a.table)) + scales[slot].table_first;
        cv_chain_sweep<false>(a.chains, stages, img, img, true, a.table + (size_t)scales[slot].table_first * 16u, table, q, n_here, fail_g,
                              reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX), lane, [&](const CvTreeEntry& e, bool mine, bool accepted) {
                                  if (mine) atomicOr((accepted ? a.accept : a.reject) + e.word, 1ull << (e.bit_slot & 63u));
                              });
        __builtin_amdgcn_wave_barrier();
    }
}

int launch_cv_tree_chain_pass(const CvTreeArgs& a, int n_blocks, void* stream_) {
    hipLaunchKernelGGL(cv_tree_chain_pass, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_cv_tree_walk(const CvTreeArgs& a, int n_blocks, void* stream_) {
    hipLaunchKernelGGL(cv_tree_walk, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}
int launch_cv_tree_emit(const CvTreeArgs& a, int n_blocks, void* stream_) {
    hipLaunchKernelGGL(cv_tree_emit, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------ tilted integral
// cvIntegral's tilted sum (OpenCV 2.4.2 imgproc; tilted(X, Y) = sum of gray(x, y) over y < Y, |x - X + 1| <= Y - y - 1),
// exact in 32 bits modulo 2^32 like CV_32S.  Only cascades with tilted features in the OpenCV profile ask for it; it is not on the
// headline path.
__device__ __forceinline__ uint32_t gray_at(const uint8_t* row, uint32_t x, uint32_t ch) {
    if (ch <= 1u) return row[x];
    const uint8_t* p = row + (size_t)x * ch;
    return (p[0] * 1868u + p[1] * 9617u + p[2] * 4899u + 8192u) >> 14;   // OpenCV's 8-bit BGR2GRAY, as the integral kernels
}

// Not by cvIntegral's row recurrence (each row depends on the two above: 1080 barriers deep, 1.25 ms whatever the batch).  With zero
// outside the frame,
//   A(x, y) = sum_k I(x - k, y - k)   (the "\" diagonal ending at (x, y)),    B(x, y) = sum_k I(x + k, y - k)   (the "/" diagonal),
// the triangle with its apex at pixel (x, y) is the one with its apex at (x, y - 1) plus both diagonals through (x, y):
//   Tri(x, y) = Tri(x, y - 1) + A(x, y) + B(x, y) - I(x, y),        tilted(X, Y) = Tri(X - 1, Y - 1)
// — a column prefix of C = A + B - I, and A and B are column prefixes of the image sheared one way and the other.  Three prefix sums
// over the rows, each in bands of 8 rows like the upright integral: per-band totals, an exclusive scan over the bands, the rows of a
// band from its prefix.  Integer adds mod 2^32 in another order: the same image, bit for bit (vj_integral_tilted's tests compare
// it with the oracle's direct sum).  diag: [frame][band][2][W + H] (A by x - y + H - 1, B by x + y), col: [frame][band][W + 1].
constexpr uint32_t TILT_ROWS = 8;
__device__ __forceinline__ uint32_t tilt_px(const TiltedArgs& a, const uint8_t* img, int32_t x, int32_t y) {
    if (x < 0 || y < 0 || x >= (int32_t)a.width || y >= (int32_t)a.height) return 0u;
    return gray_at(img + (size_t)y * a.gray_stride, (uint32_t)x, a.channels);
}

__global__ __launch_bounds__(256) void tilt_diag_sums(TiltedArgs a, uint32_t* diag) {
    const uint32_t D = a.width + a.height, i = blockIdx.x * 256u + threadIdx.x, band = blockIdx.y, frame = blockIdx.z;
    if (i >= D) return;
    const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
    const uint32_t n_bands = (a.height + TILT_ROWS - 1u) / TILT_ROWS;
    uint32_t sa = 0, sb = 0;
    for (uint32_t r = 0; r < TILT_ROWS; ++r) {
        const int32_t y = (int32_t)(band * TILT_ROWS + r);
        sa += tilt_px(a, img, (int32_t)i - (int32_t)(a.height - 1u) + y, y);
        sb += tilt_px(a, img, (int32_t)i - y, y);
    }
    uint32_t* d = diag + ((size_t)frame * n_bands + band) * 2u * D;
    d[i] = sa;
    d[D + i] = sb;
}

// exclusive prefix over the bands, in place: `n` values per band, `per_band` the distance between bands
__global__ __launch_bounds__(256) void tilt_band_scan(uint32_t* v, uint32_t n, uint32_t per_band, uint32_t n_bands) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, frame = blockIdx.y;
    if (i >= n) return;
    uint32_t* p = v + (size_t)frame * n_bands * per_band + i;
    uint32_t s = 0;
    for (uint32_t b0 = 0; b0 < n_bands; b0 += 8u) {   // eight bands' loads in flight per step
        uint32_t t[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) t[k] = b0 + k < n_bands ? p[(size_t)(b0 + k) * per_band] : 0u;
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            if (b0 + k < n_bands) p[(size_t)(b0 + k) * per_band] = s;
            s += t[k];
        }
    }
}

// C(xc, y) for the rows of one band: the diagonals' prefixes at the band's top edge plus their part inside the band
template <typename F>
__device__ __forceinline__ void tilt_band_rows(const TiltedArgs& a, const uint8_t* img, const uint32_t* d /* this band's diag block */, int32_t xc,
                                               uint32_t band, F row) {
    const uint32_t D = a.width + a.height;
    const int32_t y0 = (int32_t)(band * TILT_ROWS);
    for (uint32_t r = 0; r < TILT_ROWS && y0 + (int32_t)r < (int32_t)a.height; ++r) {
        const int32_t y = y0 + (int32_t)r;
        const int32_t ia = xc - y + (int32_t)(a.height - 1u), ib = xc + y;
        uint32_t A = ia >= 0 && ia < (int32_t)D ? d[ia] : 0u, B = ib >= 0 && ib < (int32_t)D ? d[D + ib] : 0u;
        for (int32_t k = 0; k <= (int32_t)r; ++k) {
            A += tilt_px(a, img, xc - k, y - k);
            B += tilt_px(a, img, xc + k, y - k);
        }
        row(y, A + B - tilt_px(a, img, xc, y));
    }
}

__global__ __launch_bounds__(256) void tilt_col_sums(TiltedArgs a, const uint32_t* diag, uint32_t* col) {
    const uint32_t ow = a.width + 1u, X = blockIdx.x * 256u + threadIdx.x, band = blockIdx.y, frame = blockIdx.z;
    if (X >= ow) return;
    const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
    const uint32_t n_bands = (a.height + TILT_ROWS - 1u) / TILT_ROWS, D = a.width + a.height;
    uint32_t s = 0;
    tilt_band_rows(a, img, diag + ((size_t)frame * n_bands + band) * 2u * D, (int32_t)X - 1, band, [&](int32_t, uint32_t c) { s += c; });
    col[((size_t)frame * n_bands + band) * ow + X] = s;
}

__global__ __launch_bounds__(256) void tilt_out_rows(TiltedArgs a, const uint32_t* diag, const uint32_t* col) {
    const uint32_t ow = a.width + 1u, X = blockIdx.x * 256u + threadIdx.x, band = blockIdx.y, frame = blockIdx.z;
    if (X >= ow) return;
    const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
    const uint32_t n_bands = (a.height + TILT_ROWS - 1u) / TILT_ROWS, D = a.width + a.height;
    uint32_t* out = a.tilted + (size_t)frame * a.frame_elems;
    if (band == 0u) out[X] = 0u;   // row 0
    uint32_t acc = col[((size_t)frame * n_bands + band) * ow + X];
    tilt_band_rows(a, img, diag + ((size_t)frame * n_bands + band) * 2u * D, (int32_t)X - 1, band, [&](int32_t y, uint32_t c) {
        acc += c;
        out[(size_t)(y + 1) * ow + X] = acc;   // tilted(X, Y = y + 1) = Tri(X - 1, y)
    });
}

int launch_tilted_bands(const TiltedArgs& a, uint32_t* diag, uint32_t* col, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t n_bands = (a.height + TILT_ROWS - 1u) / TILT_ROWS, D = a.width + a.height, ow = a.width + 1u;
    hipLaunchKernelGGL(tilt_diag_sums, dim3((D + 255u) / 256u, n_bands, a.n_frames), dim3(256), 0, stream, a, diag);
    hipLaunchKernelGGL(tilt_band_scan, dim3((2u * D + 255u) / 256u, a.n_frames), dim3(256), 0, stream, diag, 2u * D, 2u * D, n_bands);
    hipLaunchKernelGGL(tilt_col_sums, dim3((ow + 255u) / 256u, n_bands, a.n_frames), dim3(256), 0, stream, a, (const uint32_t*)diag, col);
    hipLaunchKernelGGL(tilt_band_scan, dim3((ow + 255u) / 256u, a.n_frames), dim3(256), 0, stream, col, ow, ow, n_bands);
    hipLaunchKernelGGL(tilt_out_rows, dim3((ow + 255u) / 256u, n_bands, a.n_frames), dim3(256), 0, stream, a, (const uint32_t*)diag, (const uint32_t*)col);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------ gray image
// clifGrayscale (clif.h:55-58 -> cvCvtColor BGR2GRAY): the gray image the integral kernels see, as its own output.
__global__ __launch_bounds__(256) void gray_rows(TiltedArgs a, uint8_t* dst, uint32_t dst_stride) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= a.width) return;
    dst[(size_t)y * dst_stride + x] = (uint8_t)gray_at(a.gray + (size_t)y * a.gray_stride, x, a.channels);
}

int launch_grayscale(const TiltedArgs& a, uint8_t* dst, uint32_t dst_stride, void* stream_) {
    hipLaunchKernelGGL(gray_rows, dim3((a.width + 255u) / 256u, a.height), dim3(256), 0, (hipStream_t)stream_, a, dst, dst_stride);
    return (int)hipGetLastError();
}

}  // namespace vj
