// cv::groupRectangles on the device, per frame — what vj_group.cpp does on the host (tempcv.cpp:130-243; the
// reference's filterResult, clod.cpp:182-357, is its broken port) — so that the GROUPED faces of a first cascade can
// become the regions of a second one without leaving the device (vj_detect_chain).
//
// The result must equal the host's on the candidates in their canonical order (frame, scale, y, x):
//   * cv::partition labels the connected components of the "similar" graph in order of first appearance, i.e. by
//     their smallest member index.  Here: the frame's candidates are sorted in LDS (bitonic, 64-bit keys), every
//     candidate starts as its own label, and labels are lowered to the smallest label among similar candidates
//     (followed by pointer jumping) until nothing changes: a label then is the smallest index of its component, and the
//     classes in the order of their labels are partition()'s classes.
//   * the class sums are integer (LDS atomics: order-free), the averages use the same f32 operations, and the
//     containment filter the same integer / f64 comparisons as the host code.
// -ffp-contract=off as everywhere.
#include <hip/hip_runtime.h>
#include <climits>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_group_frame.hpp"

namespace vj {

__global__ __launch_bounds__(256) void group_count(GroupArgs g) {
    const uint32_t n = min(*g.det_count, g.det_cap);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t frame = g.det[i].off / g.frame_bytes;
        if (frame < g.n_frames) atomicAdd(g.frame_count + frame, 1u);
    }
}

// Exclusive prefix of `in[0..n)` into out[0..n], out[n] = total; one workgroup.
__device__ __forceinline__ void block_exclusive_prefix(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* lds /* >= 17 */) {
    const uint32_t lane = lane_id(), wib = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += blockDim.x) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = i < n ? in[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += t;
        }
        if (lane == 63u) lds[wib] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < n_waves; ++w) {
            const uint32_t c = lds[w];
            before += w < wib ? c : 0u;
            total += c;
        }
        if (i < n) out[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
}

__global__ __launch_bounds__(GROUP_THREADS) void group_offsets(GroupArgs g) {
    __shared__ uint32_t lds[GROUP_THREADS / 64 + 1];
    block_exclusive_prefix(g.frame_count, g.frame_first, g.n_frames, lds);
}

__global__ __launch_bounds__(256) void group_scatter(GroupArgs g) {
    const uint32_t n = min(*g.det_count, g.det_cap);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const DetEntry d = g.det[i];
        const uint32_t frame = d.off / g.frame_bytes;
        if (frame >= g.n_frames) continue;
        const uint32_t el = (d.off - frame * g.frame_bytes) >> 2;
        const uint32_t pos = g.frame_first[frame] + atomicAdd(g.frame_cursor + frame, 1u);
        g.keys[pos] = (uint64_t)d.scale << 32 | el;   // (scale, y, x) order == (scale, element) order
    }
}

// (ASimilarRects, block_rank and the grouping of one frame, group_classes: vj_group_frame.hpp, shared with vj_cv_biggest.hip)

__global__ __launch_bounds__(GROUP_THREADS) void group_frame(GroupArgs g) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const GroupLds L = group_lds(lds);   // (layout and algorithm: vj_group_frame.hpp)
    const uint32_t frame = blockIdx.x;
    const uint32_t first = g.frame_first[frame];
    const uint32_t n = g.frame_first[frame + 1u] - first;
    const uint32_t tid = threadIdx.x;
    if (n == 0u) return;
    if (n > min(g.group_max, GROUP_MAX)) {
        if (tid == 0u) atomicAdd(g.overflow, 1u);
        return;
    }
    // the keys order a frame's candidates by (scale, y, x); a candidate is its scale's window at element y * stride + x
    uint32_t ncls = 0;
    const uint32_t n_out = group_classes(
        L, n, g.threshold, g.eps, [&](uint32_t i) { return g.keys[first + i]; },
        [&](uint64_t key, int32_t* x, int32_t* y, int32_t* w, int32_t* h) {
            const uint32_t slot = (uint32_t)(key >> 32), el = (uint32_t)key;
            const uint32_t yy = el / g.stride;
            *x = (int32_t)(el - yy * g.stride);
            *y = (int32_t)yy;
            *w = (int32_t)g.scales[slot].win_w;
            *h = (int32_t)g.scales[slot].win_h;
        },
        &ncls);
    for (uint32_t i = tid; i < ncls; i += GROUP_THREADS)
        if (L.label[i]) {
            g.grouped[first + L.aux[i]] = RoiDev{(int32_t)frame, L.cx[i], L.cy[i], L.cw[i], L.ch[i]};
            g.grouped_weight[first + L.aux[i]] = L.cn[i];
        }
    if (tid == 0u) g.grouped_count[frame] = n_out;
}

// Concatenate the frames' grouped rectangles in frame order: the region list of the second cascade.
__global__ __launch_bounds__(GROUP_THREADS) void group_collect(GroupArgs g) {
    __shared__ uint32_t lds[GROUP_THREADS / 64 + 1];
    // frame_cursor is free again: it takes the output offsets (n_frames + 1 would overrun it by one: the total goes to lds)
    const uint32_t lane = lane_id(), wib = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < g.n_frames; i0 += GROUP_THREADS) {
        const uint32_t f = i0 + threadIdx.x;
        const uint32_t v = f < g.n_frames ? g.grouped_count[f] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += t;
        }
        if (lane == 63u) lds[wib] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < GROUP_THREADS / 64; ++w) {
            const uint32_t c = lds[w];
            before += w < wib ? c : 0u;
            total += c;
        }
        if (f < g.n_frames) {
            const uint32_t dst = carry + before + incl - v, src = g.frame_first[f];
            for (uint32_t k = 0; k < v; ++k)
                if (dst + k < g.max_rois) {
                    g.rois[dst + k] = g.grouped[src + k];
                    g.roi_weight[dst + k] = g.grouped_weight[src + k];
                }
        }
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *g.n_rois = carry;
}

int prepare_group_kernels() {
    return (int)hipFuncSetAttribute((const void*)group_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GROUP_LDS_BYTES);
}

int launch_group_rois(const GroupArgs& g, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    // frame_count | frame_cursor | grouped_count | overflow are one block
    hipError_t e = hipMemsetAsync(g.frame_count, 0, ((size_t)3u * g.n_frames + 1u) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(group_count, dim3(256), dim3(256), 0, stream, g);
    hipLaunchKernelGGL(group_offsets, dim3(1), dim3(GROUP_THREADS), 0, stream, g);
    hipLaunchKernelGGL(group_scatter, dim3(256), dim3(256), 0, stream, g);
    hipLaunchKernelGGL(group_frame, dim3(g.n_frames), dim3(GROUP_THREADS), GROUP_LDS_BYTES, stream, g);
    hipLaunchKernelGGL(group_collect, dim3(1), dim3(GROUP_THREADS), 0, stream, g);
    return (int)hipGetLastError();
}

}  // namespace vj
