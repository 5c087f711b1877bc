// gfx950 kernels of vj_detect_opencv_chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE): what the first cascade
// reports (CvDet records in the order the waves found them) becomes the region list (CvRoiDev) and the unit list (CvRoiUnit) of the
// region pass (vj_cv_roi.hip) without a trip through the host — what cv_chain_regions and cv_roi_build_units (vj_cv_roi_host.cpp)
// do on the CPU.
//
//   regions, raw candidates   cv_chain_count -> cv_chain_offsets -> cv_chain_scatter: every record is a region, bucketed by frame (the
//                             region pass walks one frame's regions together); pad[0] = the record's index, through which the host
//                             finds the region's place in the sorted out_first.  Order inside a frame is free.
//   regions, grouped          the same three with 64-bit keys (slot << 32 | element) instead of regions, then cv_chain_group — one
//                             workgroup per frame, group_classes (vj_group_frame.hpp: cv::groupRectangles with the host's classes,
//                             averages and order) — and cv_chain_collect, which concatenates the frames' rectangles in frame order.
//                             pad[0] = the class's members (the rectangle's weight in out_first).
//   units                     cv_chain_unit_count (one thread per region: the scale loop of cv_roi_build_units, restated once for host
//                             and device in vj_cv_roi_units.hpp, with every refusal counted) -> cv_chain_unit_offsets (one workgroup:
//                             exclusive prefix, 64-bit total) -> cv_chain_unit_fill (one wave per region: {roi, slot, iy, end_x} in
//                             (region, factor, row) order at the region's offset).
// The count pass's totals are exact whatever the buffers hold; a fill that would not fit writes nothing and leaves n_units_run = 0, so
// that the region pass behind it has nothing to walk and the host enqueues the sub-batch again with the room the totals ask for.
// -ffp-contract=off as everywhere (the f64 divide and round of the grid ends must be the host's).
#include <hip/hip_runtime.h>
#include <climits>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_group_frame.hpp"

namespace vj {

namespace {
__device__ __forceinline__ uint32_t chain_n_det(const CvChainArgs& a) { return min(*a.det_count, a.det_cap); }
}  // namespace

__global__ __launch_bounds__(256) void cv_chain_count(CvChainArgs a) {
    const uint32_t n = chain_n_det(a);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t frame = a.det[i].frame;
        if (frame < a.n_frames) atomicAdd(a.frame_count + frame, 1u);
    }
}

// Exclusive prefix of in[0..n) into out[0..n) (32-bit: offsets into a buffer of fewer than 2^31 entries; meaningless, and unused, when
// the total is larger); returns the 64-bit total to every thread.  One workgroup of GROUP_THREADS; lds >= GROUP_THREADS / 64 words.
__device__ __forceinline__ unsigned long long chain_exclusive_prefix(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* lds) {
    const uint32_t lane = lane_id(), wib = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += GROUP_THREADS) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t incl = v;   // (a wave's 64 values: each below 2^22 — at most 65535 rows of a few dozen factors — so no wrap here)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += t;
        }
        if (lane == 63u) lds[wib] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (uint32_t w = 0; w < GROUP_THREADS / 64; ++w) {
            const uint32_t c = lds[w];
            before += w < wib ? c : 0u;
            total += c;
        }
        if (i < n) out[i] = (uint32_t)(carry + before + incl - v);
        carry += total;
        __syncthreads();
    }
    return carry;
}

__global__ __launch_bounds__(GROUP_THREADS) void cv_chain_offsets(CvChainArgs a) {
    __shared__ uint32_t lds[GROUP_THREADS / 64];
    const unsigned long long total = chain_exclusive_prefix(a.frame_count, a.frame_first, a.n_frames, lds);
    if (threadIdx.x == 0u) {
        a.frame_first[a.n_frames] = (uint32_t)total;
        if (!a.grouped) a.state->n_regions = (uint32_t)total;
    }
}

__global__ __launch_bounds__(256) void cv_chain_scatter(CvChainArgs a) {
    const uint32_t n = chain_n_det(a);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const CvDet d = a.det[i];
        if (d.frame >= a.n_frames || d.slot >= a.n_scales) continue;
        const uint32_t pos = a.frame_first[d.frame] + atomicAdd(a.frame_cursor + d.frame, 1u);
        if (pos >= a.det_cap) continue;   // (cannot happen: the offsets are those of the same records)
        if (a.grouped) a.keys[pos] = (uint64_t)d.slot << 32 | (uint64_t)(d.y * a.stride + d.x);   // (slot, y, x) order == (slot, element) order
        else a.rois[pos] = CvRoiDev{d.frame, d.x, d.y, a.scales[d.slot].win_w, a.scales[d.slot].win_h, {i, 0u, 0u}};
    }
}

__global__ __launch_bounds__(GROUP_THREADS) void cv_chain_group(CvChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const GroupLds L = group_lds(lds);   // (layout and algorithm: vj_group_frame.hpp)
    const uint32_t frame = blockIdx.x;
    const uint32_t first = a.frame_first[frame];
    const uint32_t n = a.frame_first[frame + 1u] - first;
    const uint32_t tid = threadIdx.x;
    if (n == 0u) return;
    if (n > min(a.group_max, GROUP_MAX)) {
        if (tid == 0u) atomicAdd(&a.state->overflow, 1u);
        return;
    }
    uint32_t ncls = 0;
    const uint32_t n_out = group_classes(
        L, n, a.threshold, a.eps, [&](uint32_t i) { return a.keys[first + i]; },
        [&](uint64_t key, int32_t* x, int32_t* y, int32_t* w, int32_t* h) {
            const uint32_t slot = (uint32_t)(key >> 32), el = (uint32_t)key;
            const uint32_t yy = el / a.stride;
            *x = (int32_t)(el - yy * a.stride);
            *y = (int32_t)yy;
            *w = (int32_t)a.scales[slot].win_w;
            *h = (int32_t)a.scales[slot].win_h;
        },
        &ncls);
    for (uint32_t i = tid; i < ncls; i += GROUP_THREADS)
        if (L.label[i])   // (n_out <= n: inside the frame's own segment)
            a.staged[first + L.aux[i]] = CvRoiDev{frame, (uint32_t)L.cx[i], (uint32_t)L.cy[i], (uint32_t)L.cw[i], (uint32_t)L.ch[i], {L.cn[i], 0u, 0u}};
    if (tid == 0u) a.grouped_count[frame] = n_out;
}

// Concatenate the frames' grouped rectangles in frame order: the region list of the second cascade.
__global__ __launch_bounds__(GROUP_THREADS) void cv_chain_collect(CvChainArgs a) {
    __shared__ uint32_t lds[GROUP_THREADS / 64];
    // frame_cursor is free again: it takes the output offsets
    const unsigned long long total = chain_exclusive_prefix(a.grouped_count, a.frame_cursor, a.n_frames, lds);
    __syncthreads();
    for (uint32_t f = threadIdx.x; f < a.n_frames; f += GROUP_THREADS) {
        const uint32_t dst = a.frame_cursor[f], src = a.frame_first[f], v = a.grouped_count[f];
        for (uint32_t k = 0; k < v; ++k)
            if (dst + k < a.det_cap) a.rois[dst + k] = a.staged[src + k];   // (the grouped are never more than the candidates)
    }
    if (threadIdx.x == 0u) a.state->n_regions = (uint32_t)min(total, (unsigned long long)a.det_cap);
}

// One thread per region: the scale loop of cv_roi_build_units (vj_cv_roi_host.cpp) for the region's w x h, counting
__global__ __launch_bounds__(256) void cv_chain_unit_count(CvChainArgs a) {
    const uint32_t n = a.state->n_regions;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const CvRoiDev r = a.rois[i];
        uint32_t units = 0;
        unsigned long long windows = 0;
        // (the members are unsigned: a negative origin or size of a grouped rectangle shows as a value above every frame size)
        if (r.frame >= a.n_frames || r.w == 0u || r.h == 0u || r.w > a.width || r.h > a.height || r.x > a.width - r.w || r.y > a.height - r.h) {
            atomicAdd(&a.state->err_outside, 1u);
        } else {
            const uint32_t nk = cv_chain_count_factors(a.factors, a.n_factors, a.win_w, a.win_h, (int)r.w, (int)r.h);
            // (would the region take the factor after the table's last?  the enumeration's next double)
            const double next = a.factors[a.n_factors - 1u].factor * a.scale_factor;
            if (nk == a.n_factors && next * a.win_w < (double)r.w - 10 && next * a.win_h < (double)r.h - 10) {
                atomicAdd(&a.state->err_factors, 1u);
            } else {
                for (uint32_t k = 0; k < nk; ++k) {
                    int end_x, end_y;
                    const int what = cv_chain_slot(a.factors[k], (int)r.x, (int)r.y, (int)r.w, (int)r.h, a.min_w, a.min_h, a.stride, a.frame_elems, &end_x, &end_y);
                    if (what == CV_CHAIN_SLOT_SKIP) continue;
                    if (what == CV_CHAIN_SLOT_REACH) {
                        atomicAdd(&a.state->err_reach, 1u);
                        continue;
                    }
                    units += (uint32_t)end_y;
                    windows += (unsigned long long)end_x * (unsigned long long)end_y;
                }
            }
        }
        a.roi_units[i] = units;
        if (windows != 0ull) atomicAdd((unsigned long long*)&a.state->windows, windows);
    }
}

__global__ __launch_bounds__(GROUP_THREADS) void cv_chain_unit_offsets(CvChainArgs a) {
    __shared__ uint32_t lds[GROUP_THREADS / 64];
    const unsigned long long total = chain_exclusive_prefix(a.roi_units, a.roi_first, a.state->n_regions, lds);
    if (threadIdx.x == 0u) {
        CvChainState* s = a.state;
        s->n_units = total;
        // the detection counter and the unit index are 32-bit (cv_roi_build_units' limits); anything refused, short or to be redone
        // through the host leaves the region pass nothing to walk
        const bool fits = total <= (unsigned long long)a.unit_cap && total <= 0x7fffffffull && s->windows <= 0xffffffffull;
        const bool clean = s->overflow == 0u && s->err_outside == 0u && s->err_factors == 0u && s->err_reach == 0u && *a.det_count <= a.det_cap;
        s->n_units_run = fits && clean ? (uint32_t)total : 0u;
    }
}

// One wave per region (the rest by stride): the units of (region, factor) in row order, factors in order, at the region's offset
__global__ __launch_bounds__(256) void cv_chain_unit_fill(CvChainArgs a) {
    if (a.state->n_units_run == 0u) return;
    const uint32_t n = a.state->n_regions;
    const uint32_t lane = lane_id();
    const uint32_t waves = gridDim.x * 4u;
    for (uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6); i < n; i += waves) {
        if (a.roi_units[i] == 0u) continue;
        const CvRoiDev r = a.rois[i];
        const uint32_t nk = cv_chain_count_factors(a.factors, a.n_factors, a.win_w, a.win_h, (int)r.w, (int)r.h);
        uint32_t at = a.roi_first[i];
        for (uint32_t k = 0; k < nk; ++k) {
            int end_x, end_y;
            if (cv_chain_slot(a.factors[k], (int)r.x, (int)r.y, (int)r.w, (int)r.h, a.min_w, a.min_h, a.stride, a.frame_elems, &end_x, &end_y) != CV_CHAIN_SLOT_OK)
                continue;
            for (uint32_t iy = lane; iy < (uint32_t)end_y; iy += 64u)
                if (at + iy < a.unit_cap) a.units[at + iy] = CvRoiUnit{i, k, iy, (uint32_t)end_x};
            at += (uint32_t)end_y;
        }
    }
}

int prepare_cv_chain_kernels() {
    return (int)hipFuncSetAttribute((const void*)cv_chain_group, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GROUP_LDS_BYTES);
}

int launch_cv_chain_handoff(const CvChainArgs& a, int n_cu, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 wide((uint32_t)(n_cu > 0 ? n_cu : 1));
    hipLaunchKernelGGL(cv_chain_count, dim3(256), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(cv_chain_offsets, dim3(1), dim3(GROUP_THREADS), 0, stream, a);
    hipLaunchKernelGGL(cv_chain_scatter, dim3(256), dim3(256), 0, stream, a);
    if (a.grouped) {
        hipLaunchKernelGGL(cv_chain_group, dim3(a.n_frames), dim3(GROUP_THREADS), GROUP_LDS_BYTES, stream, a);
        hipLaunchKernelGGL(cv_chain_collect, dim3(1), dim3(GROUP_THREADS), 0, stream, a);
    }
    hipLaunchKernelGGL(cv_chain_unit_count, wide, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(cv_chain_unit_offsets, dim3(1), dim3(GROUP_THREADS), 0, stream, a);
    hipLaunchKernelGGL(cv_chain_unit_fill, dim3(wide.x * 4u), dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}

}  // namespace vj
