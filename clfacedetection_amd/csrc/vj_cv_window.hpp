// Per-window arithmetic of the OpenCV profile's row kernels, shared by vj_cv_profile.hip (the scale-cascade and scale-image
// paths) and vj_cv_biggest.hip (CV_HAAR_FIND_BIGGEST_OBJECT): node, tree and stage sums as cvRunHaarClassifierCascadeSum writes
// them (tempcv.cpp:771-972), the stump-parallel form of a stage for a thin population, the sweep of the later stages over a
// wave's queue of stage-0 survivors, and the skip recurrence of a window row.  MUST be compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"

namespace vj {

struct CvQEntry {
    uint32_t off;   // byte offset of the window origin in the batch sum image
    uint32_t xy;    // x | y << 16
    double vnf;     // variance_norm_factor
};

__device__ __forceinline__ int cv_round(double v) { return __double2int_rn(v); }   // cvRound: half to even

// calc_sum(rect, offset) = p0 - p1 - p2 + p3 in int (sumtype; tempcv.cpp:118-121): corner q of rectangle k sits
// at lt + {0, da, db, da + db}.  Upright: da = width, db = height * stride; tilted (:743-750): da = height *
// (stride - 1), db = width * (stride + 1).
__device__ __forceinline__ int32_t cv_calc_sum(rsrc_t img, uint32_t off, uint32_t lt, uint32_t da, uint32_t db) {
    return (int32_t)(ld_u32(img, off, lt) - ld_u32(img, off, lt + da) - ld_u32(img, off, lt + db) + ld_u32(img, off, lt + da + db));
}

// One node's weighted rectangle sum.  F64 = a stump stage flagged two_rects (tempcv.cpp:872-888):
// `double rect0 = calc_sum(..); rect0 *= weight; ... sum = rect1 + rect0` — f64 products.  Otherwise (:783-788,
// :907-911) `calc_sum(..) * weight` is int * float: the int is converted to binary32 (rounding above 2^24), the
// product is a binary32 product, and only then is it widened to double and accumulated.
template <bool F64>
__device__ __forceinline__ double cv_node_sum(rsrc_t sum_img, rsrc_t tilt_img, const NodeRecDev& r, uint32_t off) {
    const rsrc_t img = (r[15] & CV_NODE_TILTED) ? tilt_img : sum_img;   // uniform
    const int32_t r0 = cv_calc_sum(img, off, r[0], r[3], r[6]);
    const int32_t r1 = cv_calc_sum(img, off, r[1], r[4], r[7]);
    const float w0 = __uint_as_float(r[9]), w1 = __uint_as_float(r[10]), w2 = __uint_as_float(r[11]);
    if (F64) {
        const double rect0 = (double)r0 * (double)w0;
        const double rect1 = (double)r1 * (double)w1;
        return rect1 + rect0;   // two_rects: there is no third rectangle
    }
    double s = (double)((float)r0 * w0);
    s += (double)((float)r1 * w1);
    if (w2 != 0.0f) {   // uniform (node->feature.rect[2].p0 != 0)
        const int32_t r2 = cv_calc_sum(img, off, r[2], r[5], r[8]);
        s += (double)((float)r2 * w2);
    }
    return s;
}

// One stage on one window: stumps through the scalar cache; multi-node trees visit their records in index
// order under the lanes whose walk sits on them (a child always follows its parent), as stage_sum_trees does.
template <bool TREES, bool F64>
__device__ __forceinline__ double cv_stage_sum(rsrc_t img, rsrc_t timg, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off,
                                               double vnf) {
    double stage_sum = 0.0;
    if (!TREES) {
        NodeRecDev r = tab[0];
        for (uint32_t j = 0; j < n_nodes; ++j) {
            const NodeRecDev rn = tab[j + 1 < n_nodes ? j + 1 : j];
            const double t = (double)__uint_as_float(r[12]) * vnf;
            const double s = cv_node_sum<F64>(img, timg, r, off);
            stage_sum += (double)(s < t ? __uint_as_float(r[13]) : __uint_as_float(r[14]));   // alpha[sum >= t]
            r = rn;
        }
        return stage_sum;
    }
    uint32_t cur = 0, k = 0;
    float value = 0.0f;
    bool done = false;
    for (uint32_t j = 0; j < n_nodes; ++j) {
        const NodeRecDev r = tab[j];
        const uint32_t flags = r[15];
        if (!done && cur == k) {
            const double t = (double)__uint_as_float(r[12]) * vnf;
            const bool go_left = cv_node_sum<false>(img, timg, r, off) < t;
            const uint32_t nxt = go_left ? r[13] : r[14];
            if (go_left ? (flags & 1u) != 0u : (flags & 2u) != 0u) {
                cur = nxt;
            } else {
                value = __uint_as_float(nxt);
                done = true;
            }
        }
        ++k;
        if (flags & 4u) {   // last record of the tree (uniform)
            stage_sum += (double)value;
            cur = 0;
            k = 0;
            done = false;
        }
    }
    return stage_sum;
}

// Two-node trees (a root and its only node child — every tree of frontalface_alt2; upright features) with BOTH nodes' gathers
// in flight: the walk above pays two memory round trips per tree — the child's under the lanes that go there — and a thin
// sweep waits for each.  The tree's value is the walk's (tempcv.cpp:771-792: idx = sum < t ? left : right until idx <= 0):
// the child's leaf where the root's side is a node, else the root's leaf; node sums int * float widened to double (:783-788).
__device__ __forceinline__ double cv_stage_sum_tree2(rsrc_t img, kptr<NodeRecDev> tab, uint32_t n_trees, uint32_t off, double vnf) {
    double stage_sum = 0.0;
    NodeRecDev ra = tab[0], rb = tab[1];
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t tn = t + 1u < n_trees ? t + 1u : t;
        const NodeRecDev na = tab[2u * tn], nb = tab[2u * tn + 1u];   // the next tree travels meanwhile
        const int32_t a0 = cv_calc_sum(img, off, ra[0], ra[3], ra[6]), a1 = cv_calc_sum(img, off, ra[1], ra[4], ra[7]);
        const int32_t b0 = cv_calc_sum(img, off, rb[0], rb[3], rb[6]), b1 = cv_calc_sum(img, off, rb[1], rb[4], rb[7]);
        double sa = (double)((float)a0 * __uint_as_float(ra[9]));
        sa += (double)((float)a1 * __uint_as_float(ra[10]));
        double sb = (double)((float)b0 * __uint_as_float(rb[9]));
        sb += (double)((float)b1 * __uint_as_float(rb[10]));
        const float wa2 = __uint_as_float(ra[11]), wb2 = __uint_as_float(rb[11]);
        if (wa2 != 0.0f || wb2 != 0.0f) {   // uniform (an absent third rectangle has lt = da = db = 0: four reads of the origin)
            const int32_t a2 = cv_calc_sum(img, off, ra[2], ra[5], ra[8]), b2 = cv_calc_sum(img, off, rb[2], rb[5], rb[8]);
            if (wa2 != 0.0f) sa += (double)((float)a2 * wa2);
            if (wb2 != 0.0f) sb += (double)((float)b2 * wb2);
        }
        const uint32_t flags = ra[15];
        const bool left_a = sa < (double)__uint_as_float(ra[12]) * vnf, left_b = sb < (double)__uint_as_float(rb[12]) * vnf;
        const bool to_child = left_a ? (flags & 1u) != 0u : (flags & 2u) != 0u;
        const float leaf_a = left_a ? __uint_as_float(ra[13]) : __uint_as_float(ra[14]);
        const float leaf_b = left_b ? __uint_as_float(rb[13]) : __uint_as_float(rb[14]);
        stage_sum += (double)(to_child ? leaf_b : leaf_a);
        ra = na;
        rb = nb;
    }
    return stage_sum;
}

// Stage sum with the stage's arithmetic mode (StageDev::cv_f64, host-computed: two_rects && stump cascade && no
// stage tree); `tree2`: CvArgs::tree2 (uniform).
template <bool TREES>
__device__ __forceinline__ double cv_stage_sum_mode(rsrc_t img, rsrc_t timg, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off,
                                                    double vnf, uint32_t f64, uint32_t tree2 = 0u) {
    if (!TREES && f64 != 0u) return cv_stage_sum<false, true>(img, timg, tab, n_nodes, off, vnf);
    if (TREES && tree2 != 0u) return cv_stage_sum_tree2(img, tab, n_nodes >> 1, off, vnf);
    return cv_stage_sum<TREES, false>(img, timg, tab, n_nodes, off, vnf);
}

// ------------------------------------------------------------------------ stage trees made of chains (CvChainDev)
// The windows that survive a stage tree's linear prefix used to carry a target stage each and ride through ONE sweep of all
// remaining stages in chunks of 64 — ever fewer lanes evaluating, 40 stages long.  A tree made of chains (frontalface_alt_tree)
// is swept like a linear cascade instead: the population of a chain is compacted after every stage (full lanes while more than
// 64 windows are left), its rejects are set aside and become the population of the next chain, and a population of at most
// CV_TAIL_MAX windows evaluates a stage stump-parallel (lane = stump, the verdict bits replayed in stump order).  Arithmetic
// and order of the additions per window are those of cv_stage_sum (tempcv.cpp:771-792, :834-861).

// One stump stage on the lane's window, two stumps per step with all of their gathers in flight (a thin sweep pays a memory
// round trip per step); the leaf values are added in stump order.  Stage trees never take the two_rects f64 branch
// (StageDev::cv_f64 is 0 for them): int * float products widened to double (:783-788).
__device__ __forceinline__ double cv_stage_sum_pairs(rsrc_t img, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off, double vnf) {
    double stage_sum = 0.0;
    uint32_t j = 0;
    if (n_nodes >= 2u) {
        NodeRecDev ra = tab[0], rb = tab[1];
        for (; j + 1u < n_nodes; j += 2u) {
            const uint32_t ja = j + 2u < n_nodes ? j + 2u : j, jb = j + 3u < n_nodes ? j + 3u : j + 1u;
            const NodeRecDev na = tab[ja], nb = tab[jb];   // the next pair travels meanwhile
            const int32_t a0 = cv_calc_sum(img, off, ra[0], ra[3], ra[6]), a1 = cv_calc_sum(img, off, ra[1], ra[4], ra[7]);
            const int32_t b0 = cv_calc_sum(img, off, rb[0], rb[3], rb[6]), b1 = cv_calc_sum(img, off, rb[1], rb[4], rb[7]);
            double sa = (double)((float)a0 * __uint_as_float(ra[9]));
            sa += (double)((float)a1 * __uint_as_float(ra[10]));
            double sb = (double)((float)b0 * __uint_as_float(rb[9]));
            sb += (double)((float)b1 * __uint_as_float(rb[10]));
            const float wa2 = __uint_as_float(ra[11]), wb2 = __uint_as_float(rb[11]);
            if (wa2 != 0.0f || wb2 != 0.0f) {   // uniform (an absent third rectangle has lt = da = db = 0: four reads of the origin)
                const int32_t a2 = cv_calc_sum(img, off, ra[2], ra[5], ra[8]), b2 = cv_calc_sum(img, off, rb[2], rb[5], rb[8]);
                if (wa2 != 0.0f) sa += (double)((float)a2 * wa2);
                if (wb2 != 0.0f) sb += (double)((float)b2 * wb2);
            }
            stage_sum += (double)(sa < (double)__uint_as_float(ra[12]) * vnf ? __uint_as_float(ra[13]) : __uint_as_float(ra[14]));
            stage_sum += (double)(sb < (double)__uint_as_float(rb[12]) * vnf ? __uint_as_float(rb[13]) : __uint_as_float(rb[14]));
            ra = na;
            rb = nb;
        }
    }
    if (j < n_nodes) {
        const NodeRecDev r = tab[j];
        const double s = cv_node_sum<false>(img, img, r, off);
        stage_sum += (double)(s < (double)__uint_as_float(r[12]) * vnf ? __uint_as_float(r[13]) : __uint_as_float(r[14]));
    }
    return stage_sum;
}

// One stump stage for a THIN population q[0, n), n <= CV_TAIL_MAX: lane j takes stump j of a block of 64 (its record arrives
// with four coalesced 16-byte loads), every window is evaluated by all lanes at once (window offset uniform, corner offsets
// per lane), a __ballot gives the block's verdict bits; then lane w adds window w's leaf values IN STUMP ORDER (the leaf values
// come through the scalar cache).  Returns the pass mask (bit w: window w passes).  Upright features only (the caller checks).
// `masks`: n x CV_TAIL_BLOCKS words of LDS scratch.  cv_tail_stage_sum: lane w's return value is window w's stage sum (0 from n on).
template <bool F64 = false, typename E>
__device__ __forceinline__ double cv_tail_stage_sum(rsrc_t img, const uint32_t* recs_g, kptr<NodeRecDev> tab, uint32_t n_nodes, const E* q, uint32_t n,
                                                    unsigned long long* masks, uint32_t lane) {
    const uint32_t n_blocks = (n_nodes + 63u) >> 6;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t j = b * 64u + lane;
        const bool active = j < n_nodes;
        const uint4* rp = reinterpret_cast<const uint4*>(recs_g + (size_t)(active ? j : 0u) * 16u);
        const uint4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
        // CvNodeRec: lt[3] da[3] db[3] w[3] thr left right flags
        const uint32_t lt0 = r0.x, lt1 = r0.y, lt2 = r0.z, da0 = r0.w, da1 = r1.x, da2 = r1.y, db0 = r1.z, db1 = r1.w, db2 = r2.x;
        const float w0 = __uint_as_float(r2.y), w1 = __uint_as_float(r2.z), w2 = __uint_as_float(r2.w), thr_node = __uint_as_float(r3.x);
        for (uint32_t w = 0; w < n; ++w) {
            const E e = q[w];   // broadcast
            const uint32_t uo = __builtin_amdgcn_readfirstlane(e.off);
            auto rect = [&](uint32_t lt, uint32_t da, uint32_t db) {
                return (int32_t)(ld_u32(img, lt, uo) - ld_u32(img, lt + da, uo) - ld_u32(img, lt + db, uo) + ld_u32(img, lt + da + db, uo));
            };
            const int32_t c0 = rect(lt0, da0, db0), c1 = rect(lt1, da1, db1);
            double sum;
            if (F64) {   // two_rects stump stage: f64 products, rect1 + rect0 (tempcv.cpp:872-888)
                sum = (double)c1 * (double)w1 + (double)c0 * (double)w0;
            } else {
                const int32_t c2 = rect(lt2, da2, db2);
                sum = (double)((float)c0 * w0);
                sum += (double)((float)c1 * w1);
                const double with2 = sum + (double)((float)c2 * w2);
                sum = w2 != 0.0f ? with2 : sum;
            }
            const unsigned long long m = __ballot(active && !(sum < (double)thr_node * e.vnf));   // bit: alpha[1] (right)
            if (lane == 0) masks[w * CV_TAIL_BLOCKS + b] = m;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const bool have = lane < n;
    double stage_sum = 0.0;
    kptr<uint32_t> leaf = reinterpret_cast<kptr<uint32_t>>(tab);   // record k: dwords 13 / 14 = left / right value
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const unsigned long long m = masks[(have ? lane : 0u) * CV_TAIL_BLOCKS + b];
        const uint32_t jn = min(64u, n_nodes - b * 64u);
#pragma unroll 4
        for (uint32_t k = 0; k < jn; ++k) {
            const uint32_t j = b * 64u + k;
            const float l = __uint_as_float(leaf[j * 16u + 13u]), r = __uint_as_float(leaf[j * 16u + 14u]);
            stage_sum += (double)(((m >> k) & 1ull) != 0ull ? r : l);
        }
    }
    __builtin_amdgcn_wave_barrier();   // every lane has read its masks
    return stage_sum;
}

template <bool F64 = false, typename E>
__device__ __forceinline__ unsigned long long cv_tail_stage(rsrc_t img, const uint32_t* recs_g, kptr<NodeRecDev> tab, uint32_t n_nodes, double thr_stage,
                                                            const E* q, uint32_t n, unsigned long long* masks, uint32_t lane) {
    const double stage_sum = cv_tail_stage_sum<F64>(img, recs_g, tab, n_nodes, q, n, masks, lane);
    return __ballot(lane < n && stage_sum >= thr_stage);
}

// variance_norm_factor of the window at `off` bytes / `po` elements (cvRunHaarClassifierCascadeSum, tempcv.cpp:822-832): mean and
// squared mean over equRect (corners q0..q3, element offsets), f64; sqrt(variance), or 1 when it is negative
__device__ __forceinline__ void cv_window_vnf(rsrc_t img, rsrc_t sq_f, uint32_t off, uint32_t po, uint32_t q0, uint32_t q1, uint32_t q2,
                                              uint32_t q3, double inv_area, double& vnf) {
    const int32_t isum = (int32_t)(ld_u32(img, off, q0 * 4u) - ld_u32(img, off, q1 * 4u) - ld_u32(img, off, q2 * 4u) +
                                   ld_u32(img, off, q3 * 4u));
    const uint64_t qq = ld_u64(sq_f, po * 8u, q0 * 8u) - ld_u64(sq_f, po * 8u, q1 * 8u) - ld_u64(sq_f, po * 8u, q2 * 8u) +
                        ld_u64(sq_f, po * 8u, q3 * 8u);
    const double mean = (double)isum * inv_area;
    vnf = (double)qq;
    vnf = vnf * inv_area - mean * mean;
    vnf = vnf >= 0.0 ? sqrt(vnf) : 1.0;
}

// The later stages (1 ..) of a linear cascade on the wave's queue of stage-0 survivors q[0, n), compacted after every stage; who
// passes the last one is handed to `emit(q, n)` (wave-uniform control flow; n != 0).  Leaves the queue empty.
template <bool TREES, bool COUNT, typename Emit>
__device__ __forceinline__ void cv_flush_to(const CvArgs& a, rsrc_t img, rsrc_t timg, kptr<NodeRecDev> table, CvQEntry* q, uint32_t& n,
                                            uint32_t lane, Emit emit) {
    kptr<StageDev> stages = as_k(a.stages);
    for (uint32_t s = 1; s < a.n_stages && n != 0u; ++s) {
        if (COUNT && lane == 0) atomicAdd(a.stage_entered + s, (unsigned long long)n);
        kptr<NodeRecDev> tab = table + stages[s].first_node;
        const uint32_t n_nodes = stages[s].n_nodes, f64 = stages[s].cv_f64;
        const double thr = (double)stages[s].threshold;
        uint32_t m = 0;
        const bool upright = !TREES && a.tilted == nullptr;   // (the stump-parallel form reads the upright sum image only)
        if (upright && n <= a.tail_max && n_nodes >= 16u && n_nodes <= CV_TAIL_BLOCKS * 64u) {
            // a thin population: the stage stump-parallel (lane = stump), verdict bits replayed in stump order (cv_tail_stage)
            const uint32_t* recs_g = reinterpret_cast<const uint32_t*>((uintptr_t)(table + stages[s].first_node));
            unsigned long long* masks = reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX);
            const unsigned long long pm = f64 != 0u ? cv_tail_stage<true>(img, recs_g, tab, n_nodes, thr, q, n, masks, lane)
                                                    : cv_tail_stage<false>(img, recs_g, tab, n_nodes, thr, q, n, masks, lane);
            const CvQEntry e = q[lane < n ? lane : 0u];
            __builtin_amdgcn_wave_barrier();
            if ((pm >> lane) & 1ull) q[mbcnt(pm)] = e;
            n = (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool act = i < n;
            const CvQEntry e = q[act ? i : 0u];
            bool pass = false;
            if (act) pass = cv_stage_sum_mode<TREES>(img, timg, tab, n_nodes, e.off, e.vnf, f64, a.tree2) >= thr;
            const unsigned long long mask = __ballot(pass);
            __builtin_amdgcn_wave_barrier();
            if (pass) q[m + mbcnt(mask)] = e;
            m += (uint32_t)__popcll(mask);
            __builtin_amdgcn_wave_barrier();
        }
        n = m;
    }
    if (n != 0u) emit(q, n);
    n = 0;
}

// cvHaarDetectObjectsForROC's report of a window (tempcv.cpp:1084-1095): the lanes with `mine` set append a CvRocDet each through the
// detection ticket (a.det holds CvRocDet records in a ROC call, a.det_cap counts them).  Wave-uniform control flow.
__device__ __forceinline__ void cv_roc_report(const CvArgs& a, bool mine, uint32_t x, uint32_t y, uint32_t slot, uint32_t frame, uint32_t level,
                                              double weight, uint32_t lane) {
    const unsigned long long rm = __ballot(mine);
    if (rm == 0ull) return;
    uint32_t g = 0;
    if (lane == 0) g = atomicAdd(a.det_count, (uint32_t)__popcll(rm));
    g = __builtin_amdgcn_readfirstlane(g);
    const uint32_t pos = g + mbcnt(rm);
    if (mine && pos < a.det_cap) reinterpret_cast<CvRocDet*>(a.det)[pos] = CvRocDet{x, y, slot, frame, level, 0u, weight};
}

// cv_flush_to for a ROC call: the same sweep, the same sums; from stage n_stages - 3 on, who fails a stage is reported with (that stage,
// its sum) before the compaction drops it, and who passes the last stage with (n_stages, the last stage's sum) — `n + result < 4`,
// -result and stage_sum of tempcv.cpp:1086-1093.  The host refuses cascades of fewer than 4 stages, so stage 0 never reports.
template <bool TREES, bool COUNT>
__device__ __forceinline__ void cv_flush_roc(const CvArgs& a, rsrc_t img, rsrc_t timg, kptr<NodeRecDev> table, CvQEntry* q, uint32_t& n,
                                             uint32_t slot, uint32_t frame, uint32_t lane) {
    kptr<StageDev> stages = as_k(a.stages);
    for (uint32_t s = 1; s < a.n_stages && n != 0u; ++s) {
        if (COUNT && lane == 0) atomicAdd(a.stage_entered + s, (unsigned long long)n);
        kptr<NodeRecDev> tab = table + stages[s].first_node;
        const uint32_t n_nodes = stages[s].n_nodes, f64 = stages[s].cv_f64;
        const double thr = (double)stages[s].threshold;
        const bool near_end = s + 3u >= a.n_stages, last = s + 1u == a.n_stages;
        uint32_t m = 0;
        const bool upright = !TREES && a.tilted == nullptr;
        if (upright && n <= a.tail_max && n_nodes >= 16u && n_nodes <= CV_TAIL_BLOCKS * 64u) {
            const uint32_t* recs_g = reinterpret_cast<const uint32_t*>((uintptr_t)(table + stages[s].first_node));
            unsigned long long* masks = reinterpret_cast<unsigned long long*>(q + CV_TAIL_MAX);
            const double ssum = f64 != 0u ? cv_tail_stage_sum<true>(img, recs_g, tab, n_nodes, q, n, masks, lane)
                                          : cv_tail_stage_sum<false>(img, recs_g, tab, n_nodes, q, n, masks, lane);
            const bool have = lane < n, pass = have && ssum >= thr;
            const unsigned long long pm = __ballot(pass);
            const CvQEntry e = q[have ? lane : 0u];
            if (near_end)
                cv_roc_report(a, have && (!pass || last), e.xy & 0xffffu, e.xy >> 16, slot, frame, pass ? a.n_stages : s, ssum, lane);
            __builtin_amdgcn_wave_barrier();
            if (pass) q[mbcnt(pm)] = e;
            n = (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool act = i < n;
            const CvQEntry e = q[act ? i : 0u];
            double ssum = 0.0;
            bool pass = false;
            if (act) {
                ssum = cv_stage_sum_mode<TREES>(img, timg, tab, n_nodes, e.off, e.vnf, f64, a.tree2);
                pass = ssum >= thr;
            }
            if (near_end)
                cv_roc_report(a, act && (!pass || last), e.xy & 0xffffu, e.xy >> 16, slot, frame, pass ? a.n_stages : s, ssum, lane);
            const unsigned long long mask = __ballot(pass);
            __builtin_amdgcn_wave_barrier();
            if (pass) q[m + mbcnt(mask)] = e;
            m += (uint32_t)__popcll(mask);
            __builtin_amdgcn_wave_barrier();
        }
        n = m;
    }
    n = 0;
}

// Which of 64 consecutive grid positions the sequential walk visits, given the reject bits F of all of them and
// the parity `carry` of the reject run that ends just before the first one; updates carry for the next 64.
__device__ __forceinline__ bool cv_visited(unsigned long long F, uint32_t lane, uint32_t n_valid, uint32_t& carry) {
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long zeros = ~F & below;
    uint32_t parity;
    if (zeros == 0ull) parity = (lane & 1u) ^ carry;
    else parity = (lane - 1u - (63u - (uint32_t)__clzll((long long)zeros))) & 1u;
    const unsigned long long vmask = n_valid == 64u ? ~0ull : (1ull << n_valid) - 1ull;
    const unsigned long long zall = ~F & vmask;
    if (zall == 0ull) carry ^= n_valid & 1u;
    else carry = (n_valid - 1u - (63u - (uint32_t)__clzll((long long)zall))) & 1u;
    return lane < n_valid && parity == 0u;
}

}  // namespace vj
