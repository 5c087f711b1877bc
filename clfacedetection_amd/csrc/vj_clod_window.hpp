// Per-window arithmetic of the clod profile for the window-list pass (vj_run_windows; vj_points.hip): the device
// functions of vj_kernels.hip the pass needs — window_variance, node_rect_sum, the stump and tree stage sums — RESTATED here in
// their plainest form, so that the tuned kernel file (which sits on a register-allocation granule) stays untouched.  Operation for
// operation they are the same: the four corners wrap in u32 before the cast to float, one multiply per rectangle, additions in the
// written order, one f32 accumulator per stage added in tree order.  tests/test_gpu_clod_windows.py (detector equivalence) ties
// the two together.  Included only by vj_points.hip.  MUST be compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include "vj_devutil.hpp"

namespace vj {

// computeVariance (clod.cpp:418-446) for the window whose origin is element `e` of the batch images (sum_b, sq_b); the equ_rect
// offsets are elements too, wave-uniform
__device__ __forceinline__ float clodw_variance(rsrc_t sum_b, rsrc_t sq_b, uint32_t e, uint32_t e_lt, uint32_t e_dw, uint32_t e_dh,
                                                float area, bool signed_mean) {
    const uint32_t c0 = e_lt, c1 = e_lt + e_dw, c2 = e_lt + e_dh, c3 = e_lt + e_dh + e_dw;
    const uint32_t s = ld_u32(sum_b, e * 4u, c0 * 4u) - ld_u32(sum_b, e * 4u, c1 * 4u) - ld_u32(sum_b, e * 4u, c2 * 4u) +
                       ld_u32(sum_b, e * 4u, c3 * 4u);
    const uint64_t q = ld_u64(sq_b, e * 8u, c0 * 8u) - ld_u64(sq_b, e * 8u, c1 * 8u) - ld_u64(sq_b, e * 8u, c2 * 8u) +
                       ld_u64(sq_b, e * 8u, c3 * 8u);
    // (float)mats(...) / (float)area (:426-430): the sum is read unsigned, or through int* as the reference's data.i does
    const float mean = (signed_mean ? (float)(int32_t)s : (float)s) / area;
    float variance = (float)q;                       // u64 -> f32, round to nearest even
    variance = (variance / area) - (mean * mean);    // separate divide, multiply, subtract (:438)
    return variance >= 0.0f ? sqrtf(variance) : 1.0f;
}

// The weighted rectangle sums of one node (clod.cl:60-76) for the window at byte offset `off`; the record's offsets are bytes
__device__ __forceinline__ float clodw_node_rect_sum(rsrc_t img, const NodeRecDev& r, uint32_t off) {
    const uint32_t lt0 = r[0], lt1 = r[1], lt2 = r[2];
    const uint32_t dh0 = r[3], dh1 = r[4], dh2 = r[5];
    const uint32_t dw0 = r[6] & 0xffffu, dw1 = r[6] >> 16, dw2 = r[7] & 0xffffu;   // (image-stride tables: never negative)
    const float w0 = __uint_as_float(r[8]), w1 = __uint_as_float(r[9]), w2 = __uint_as_float(r[10]);
    const uint32_t r0 = ld_u32(img, off, lt0) - ld_u32(img, off, lt0 + dw0) - ld_u32(img, off, lt0 + dh0) + ld_u32(img, off, lt0 + dh0 + dw0);
    const uint32_t r1 = ld_u32(img, off, lt1) - ld_u32(img, off, lt1 + dw1) - ld_u32(img, off, lt1 + dh1) + ld_u32(img, off, lt1 + dh1 + dw1);
    // (rect_sum = 0; rect_sum += t0: the leading "0 +" only maps -0 to +0, which no comparison can observe)
    float rect_sum = (float)r0 * w0;
    rect_sum += (float)r1 * w1;
    if (w2 != 0.0f) {   // uniform branch (clod.cl:70)
        const uint32_t r2 = ld_u32(img, off, lt2) - ld_u32(img, off, lt2 + dw2) - ld_u32(img, off, lt2 + dh2) + ld_u32(img, off, lt2 + dh2 + dw2);
        rect_sum += (float)r2 * w2;
    }
    return rect_sum;
}

// One stump-based stage on one window (clod.cl:49-82): alpha[rect_sum >= norm_threshold], one running sum in stump order.  The
// next record is fetched while this one is evaluated (scalar loads are long).
__device__ __forceinline__ float clodw_stage_sum_stumps(rsrc_t img, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off, float var) {
    float stage_sum = 0.0f;
    if (n_nodes == 0u) return stage_sum;
    NodeRecDev r = tab[0];
    for (uint32_t j = 0; j < n_nodes; ++j) {
        const NodeRecDev rn = tab[j + 1u < n_nodes ? j + 1u : j];
        const float rect_sum = clodw_node_rect_sum(img, r, off);
        stage_sum += (rect_sum >= __uint_as_float(r[11]) * var) ? __uint_as_float(r[13]) : __uint_as_float(r[12]);
        r = rn;
    }
    return stage_sum;
}

// Multi-node trees: icvEvalHidHaarClassifier's walk (tempcv.cpp:771-792) on the clod f32 arithmetic.  The nodes of a tree are
// consecutive and a child follows its parent, so a tree is its records in order, each under the lanes whose walk sits on it.
__device__ __forceinline__ float clodw_stage_sum_trees(rsrc_t img, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off, float var) {
    float stage_sum = 0.0f, value = 0.0f;
    uint32_t cur = 0;     // node (inside the current tree) this lane evaluates next
    uint32_t k = 0;       // position of the record inside its tree (uniform)
    bool done = false;
    for (uint32_t j = 0; j < n_nodes; ++j) {
        const NodeRecDev r = tab[j];
        const uint32_t flags = r[7] >> 16;
        if (!done && cur == k) {
            const float t = __uint_as_float(r[11]) * var;
            const float sum = clodw_node_rect_sum(img, r, off);
            const bool go_left = sum < t;   // idx = sum < t ? left : right
            const uint32_t nxt = go_left ? r[12] : r[13];
            const bool is_node = go_left ? (flags & 1u) != 0u : (flags & 2u) != 0u;
            if (is_node) {
                cur = nxt;
            } else {
                value = __uint_as_float(nxt);
                done = true;
            }
        }
        ++k;
        if (flags & 4u) {   // last record of the tree (uniform)
            stage_sum += value;
            cur = 0;
            k = 0;
            done = false;
        }
    }
    return stage_sum;
}

template <bool TREES>
__device__ __forceinline__ float clodw_stage_sum(rsrc_t img, kptr<NodeRecDev> tab, uint32_t n_nodes, uint32_t off, float var) {
    return TREES ? clodw_stage_sum_trees(img, tab, n_nodes, off, var) : clodw_stage_sum_stumps(img, tab, n_nodes, off, var);
}

}  // namespace vj
