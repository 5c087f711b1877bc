// gfx950 kernel of the OpenCV arithmetic profile's region pass (vj_detect_opencv_rois / vj_detect_opencv_chain):
// cvHaarDetectObjects' scale-cascade path (tempcv.cpp:1344-1417, the walk of a window row :1132-1175) on REGIONS of the frames,
// reading the frames' own integral images.  A region stands for the sub-image header an OpenCV caller hands over (cvSetImageROI):
// everything the function derives from the image size comes from the region's w x h — the factors a region takes, endX / endY
// (both on the host: CvRoiUnit) and the border rule x + win_w >= w + 1, y + win_h >= h + 1 (:817-820) — while a rectangle sum
// does not depend on where the integral image starts: the window origin is (region.y + y) * stride + region.x + x in the FRAME's
// images, the node tables (byte offsets from the window origin, built with the frame's stride) are those of the factor whatever the
// region.  Tilted rectangles: the four corners in the frame's tilted integral give the sum over the same rotated rectangle of
// pixels as the four corners in the crop's (the rectangle lies inside the window, the window inside the region; what the two
// integrals' triangles hold beyond it cancels in the difference — tests/test_cv_rois_cpu.py states it on the CPU).
//
// One work unit is (region, factor slot, window row): one wave walks one row as cv_profile_pass does — stage 0 (a stage tree: the
// whole tree) on every grid position, the skip-after-reject recurrence from one __ballot per 64 positions plus a carry bit
// (cv_visited), the later stages on the wave's queue of visited survivors (cv_flush_to).  Per-window arithmetic: vj_cv_window.hpp,
// unchanged.  (Packing 2 / 4 short rows into one wave was measured and is slower: DESIGN.md §4.10.)
// MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_cv_window.hpp"

namespace vj {

template <bool TREES, bool COUNT, bool STAGE_TREE>
__global__ __launch_bounds__(CV_WAVES_PER_BLOCK * 64) void cv_roi_pass(CvRoiArgs r) {
    __shared__ CvQEntry lds_q[CV_WAVES_PER_BLOCK * CV_QCAP];
    const CvArgs& a = r.cv;
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CvQEntry* q = lds_q + wib * CV_QCAP;
    const uint32_t rank = blockIdx.x * CV_WAVES_PER_BLOCK + wib;
    kptr<CvScaleDev> scales = as_k(a.scales);
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvRoiDev> rois = as_k(r.rois);
    kptr<CvRoiUnit> units = as_k(r.units);
    const uint32_t frame_bytes4 = a.frame_elems * 4u;
    const rsrc_t img = make_rsrc(a.sum, a.n_frames * frame_bytes4);
    const rsrc_t timg = make_rsrc(a.tilted != nullptr ? a.tilted : a.sum, a.n_frames * frame_bytes4);
    const double thr0 = (double)stages[0].threshold;
    // (a unit list built on the device, vj_cv_chain.hip, brings its count with it: one scalar load, uniform for the launch)
    const uint32_t n_units = r.n_units_dev != nullptr ? *r.n_units_dev : r.n_units;

    // the waves of an XCD walk one contiguous eighth of the unit list (units are ordered by frame, region, factor, row): what they
    // gather from at one time is one neighbourhood of one frame's images (as cv_profile_pass deals its rows)
    uint32_t u_first = rank, u_end = n_units, u_step = a.total_waves;
    if (gridDim.x >= 8u) {
        const uint32_t xcd = blockIdx.x & 7u;
        const uint32_t u_begin = (uint32_t)((unsigned long long)n_units * xcd / 8u);
        u_end = (uint32_t)((unsigned long long)n_units * (xcd + 1u) / 8u);
        u_step = ((gridDim.x - xcd + 7u) >> 3) * CV_WAVES_PER_BLOCK;
        u_first = u_begin + (blockIdx.x >> 3) * CV_WAVES_PER_BLOCK + wib;
    }
    for (uint32_t u = u_first; u < u_end; u += u_step) {
        const uint32_t roi = units[u].roi, slot = units[u].slot, iy = units[u].iy, end_x = units[u].end_x;
        const uint32_t frame = rois[roi].frame, rx = rois[roi].x, ry = rois[roi].y, rw = rois[roi].w, rh = rois[roi].h;
        const double ystep = scales[slot].ystep, inv_area = scales[slot].inv_area;
        const uint32_t win_w = scales[slot].win_w, win_h = scales[slot].win_h;
        const uint32_t q0 = scales[slot].q0, q1 = scales[slot].q1, q2 = scales[slot].q2, q3 = scales[slot].q3;
        kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(a.table)) + scales[slot].table_first;
        const rsrc_t sq_f = make_rsrc(a.sqsum + (size_t)frame * a.frame_elems, frame_bytes4 * 2u);
        const uint32_t frame_bytes = frame * frame_bytes4;
        const uint32_t y = (uint32_t)cv_round((double)iy * ystep);
        const bool row_border = y + win_h >= rh + 1u;   // pt.y + height >= sum.height -> -1 (tempcv.cpp:817-820), sum = the region's
        uint32_t carry = 0;   // parity of the run of rejects that ends at the last position seen (a row starts with ixstep = 1)
        uint32_t n_q = 0;
        auto emit = [&](const CvQEntry* qq, uint32_t m) {
            uint32_t g = 0;
            if (lane == 0) g = atomicAdd(a.det_count, m);
            g = __builtin_amdgcn_readfirstlane(g);
            for (uint32_t i = lane; i < m; i += 64u)
                if (g + i < a.det_cap) a.det[g + i] = CvDet{qq[i].xy & 0xffffu, qq[i].xy >> 16, slot, roi};
        };
        for (uint32_t ix0 = 0; ix0 < end_x; ix0 += 64u) {
            const uint32_t ix = ix0 + lane;
            const bool valid = ix < end_x;
            const uint32_t x = (uint32_t)cv_round((double)(valid ? ix : 0u) * ystep);
            const bool border = row_border || x + win_w >= rw + 1u;
            const uint32_t po = (ry + y) * a.stride + rx + x;
            const uint32_t off = frame_bytes + po * 4u;
            double vnf = 1.0;
            const bool eval = valid && !border;
            if (eval) cv_window_vnf(img, sq_f, off, po, q0, q1, q2, q3, inv_area, vnf);
            const uint32_t n_valid = min(64u, end_x - ix0);
            if (STAGE_TREE) {
                // the whole stage tree for every grid position (tempcv.cpp:834-861: any reject returns 0 and skips): every lane
                // carries the stage it visits next; the stages are swept once in a topological order of the pass / fail graph
                int32_t ptr = eval ? (int32_t)stages[0].order : -3;   // -1 accepted, -2 rejected, -3 not evaluated
                static_assert(VJ_MAX_STAGES_DEV <= 64, "the stages a window entered are one bit each of a 64-bit mask");
                unsigned long long entered = 0ull;
                for (uint32_t oi = 0; oi < a.n_order; ++oi) {
                    const uint32_t s = stages[oi].order;
                    const bool here = ptr == (int32_t)s;
                    if (__ballot(here) == 0ull) continue;
                    if (here) {
                        const bool pass = cv_stage_sum<TREES, false>(img, timg, table + stages[s].first_node, stages[s].n_nodes, off, vnf) >=
                                          (double)stages[s].threshold;
                        ptr = pass ? stages[s].on_pass : stages[s].on_fail;
                        entered |= 1ull << s;
                    }
                }
                const bool visited = cv_visited(__ballot(ptr == -2), lane, n_valid, carry);
                if (COUNT) {
                    const unsigned long long vm = __ballot(visited);
                    if (lane == 0) atomicAdd(a.stage_entered + VJ_MAX_STAGES_DEV, (unsigned long long)__popcll(vm));
                    for (uint32_t s = 0; s < a.n_stages; ++s) {
                        const unsigned long long em = __ballot(visited && ((entered >> s) & 1ull) != 0ull);
                        if (lane == 0 && em != 0ull) atomicAdd(a.stage_entered + s, (unsigned long long)__popcll(em));
                    }
                }
                const bool hit = visited && ptr == -1;
                const unsigned long long am = __ballot(hit);
                if (am != 0ull) {
                    uint32_t g = 0;
                    if (lane == 0) g = atomicAdd(a.det_count, (uint32_t)__popcll(am));
                    g = __builtin_amdgcn_readfirstlane(g);
                    const uint32_t pos = g + mbcnt(am);
                    if (hit && pos < a.det_cap) a.det[pos] = CvDet{x, y, slot, roi};
                }
                continue;
            }
            bool fail0 = false;
            if (eval)
                fail0 = !(cv_stage_sum_mode<TREES>(img, timg, table + stages[0].first_node, stages[0].n_nodes, off, vnf, stages[0].cv_f64, a.tree2) >= thr0);
            // which positions does the sequential walk visit?  parity of the reject run below each lane
            const bool visited = cv_visited(__ballot(fail0), lane, n_valid, carry);
            const bool pass0 = visited && !border && !fail0;
            if (COUNT) {
                const unsigned long long vm = __ballot(visited), em = __ballot(visited && !border);
                if (lane == 0) {
                    atomicAdd(a.stage_entered + VJ_MAX_STAGES_DEV, (unsigned long long)__popcll(vm));
                    atomicAdd(a.stage_entered + 0, (unsigned long long)__popcll(em));
                }
            }
            const unsigned long long pm = __ballot(pass0);
            if (pass0) q[n_q + mbcnt(pm)] = CvQEntry{off, x | (y << 16), vnf};
            n_q += (uint32_t)__popcll(pm);
            __builtin_amdgcn_wave_barrier();
            if (n_q > (uint32_t)CV_QCAP - 64u) cv_flush_to<TREES, COUNT>(a, img, timg, table, q, n_q, lane, emit);
        }
        if (!STAGE_TREE && n_q != 0u) cv_flush_to<TREES, COUNT>(a, img, timg, table, q, n_q, lane, emit);
        __builtin_amdgcn_wave_barrier();
    }
}

template <bool TREES, bool STAGE_TREE>
static void cv_roi_launch(const CvRoiArgs& r, bool count, dim3 g, dim3 b, hipStream_t stream) {
    if (count) hipLaunchKernelGGL((cv_roi_pass<TREES, true, STAGE_TREE>), g, b, 0, stream, r);
    else       hipLaunchKernelGGL((cv_roi_pass<TREES, false, STAGE_TREE>), g, b, 0, stream, r);
}

int launch_cv_roi_pass(const CvRoiArgs& r, bool trees, bool count, bool stage_tree, int n_blocks, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    dim3 g(n_blocks), b(CV_WAVES_PER_BLOCK * 64);
    if (stage_tree) {
        if (trees) cv_roi_launch<true, true>(r, count, g, b, stream);
        else       cv_roi_launch<false, true>(r, count, g, b, stream);
    } else {
        if (trees) cv_roi_launch<true, false>(r, count, g, b, stream);
        else       cv_roi_launch<false, false>(r, count, g, b, stream);
    }
    return (int)hipGetLastError();
}

}  // namespace vj
