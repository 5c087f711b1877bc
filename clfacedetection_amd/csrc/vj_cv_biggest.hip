// gfx950 kernels of CV_HAAR_FIND_BIGGEST_OBJECT in the OpenCV arithmetic profile (VJ_FLAG_CV_FIND_BIGGEST):
// cvHaarDetectObjects with findBiggestObject as the reference keeps it in tempcv.cpp —
//   descending scale loop, scanROI ranges, break on minSize   tempcv.cpp:1353-1420
//   the grouping after each scale, maxRect, scanROI, minSize  tempcv.cpp:1422-1454
//   the walk of a window row                                  tempcv.cpp:1132-1175 (HaarDetectObjects_ScaleCascade_Invoker)
// The host enqueues one ROUND per scale, largest window first, in stream order and never looks at a result in between:
//   cv_biggest_pass    one wave per (frame, window row) of the round's scale.  The wave reads its frame's CvBigState — wave-uniform,
//                      through the scalar cache like the feature tables — and leaves at once when the frame stopped or the
//                      window is below the frame's minSize; else it derives the frame's start / end columns and rows (the whole
//                      grid while the frame searches, the scanROI's afterwards) and walks its row from startX: the skip
//                      recurrence per 64 positions by __ballot plus a carry, the per-window arithmetic of vj_cv_window.hpp.
//                      Candidates go to the frame's own segment of the detection buffer.
//   cv_biggest_update  one workgroup per frame.  A frame that still searches and has gained candidates groups all of them
//                      (group_classes, vj_group_frame.hpp: the canonical order is the walk's — scale slot, y, x); the first
//                      group of strictly greatest area becomes maxRect, and the frame's scanROI and minSize are set.
// Ordering between the kernels is the stream's.  MUST be compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"
#include "vj_cv_window.hpp"
#include "vj_group_frame.hpp"

namespace vj {

// `k` candidates of the wave (lanes with `mine`, in lane order) into the frame's segment
__device__ __forceinline__ void cv_big_emit(const CvBigArgs& b, uint32_t frame, unsigned long long mask, bool mine, uint32_t x, uint32_t y,
                                            uint32_t lane) {
    uint32_t g = 0;
    if (lane == 0) g = atomicAdd(b.frame_count + frame, (uint32_t)__popcll(mask));
    g = __builtin_amdgcn_readfirstlane(g);
    const uint32_t pos = g + mbcnt(mask);
    if (mine && pos < b.cv.det_cap) b.cv.det[(size_t)frame * b.cv.det_cap + pos] = CvDet{x, y, b.slot, frame};
}

template <bool TREES, bool COUNT, bool STAGE_TREE>
__global__ __launch_bounds__(CV_WAVES_PER_BLOCK * 64) void cv_biggest_pass(CvBigArgs b) {
    __shared__ CvQEntry lds_q[CV_WAVES_PER_BLOCK * CV_QCAP];
    const CvArgs& a = b.cv;
    const uint32_t lane = lane_id();
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    CvQEntry* q = lds_q + wib * CV_QCAP;
    const uint32_t rank = blockIdx.x * CV_WAVES_PER_BLOCK + wib;
    kptr<CvScaleDev> scales = as_k(a.scales);
    kptr<StageDev> stages = as_k(a.stages);
    kptr<CvBigState> state = as_k(b.state);
    const uint32_t frame_bytes4 = a.frame_elems * 4u;
    const rsrc_t img = make_rsrc(a.sum, a.n_frames * frame_bytes4);
    const rsrc_t timg = make_rsrc(a.tilted != nullptr ? a.tilted : a.sum, a.n_frames * frame_bytes4);
    const uint32_t slot = b.slot;
    const double ystep = scales[slot].ystep, inv_area = scales[slot].inv_area;
    const uint32_t win_w = scales[slot].win_w, win_h = scales[slot].win_h, grid_x = scales[slot].end_x, grid_y = scales[slot].end_y;
    const uint32_t q0 = scales[slot].q0, q1 = scales[slot].q1, q2 = scales[slot].q2, q3 = scales[slot].q3;
    kptr<NodeRecDev> table = as_k(reinterpret_cast<const NodeRecDev*>(a.table)) + scales[slot].table_first;
    const double thr0 = (double)stages[0].threshold;
    const uint32_t total = grid_y * a.n_frames;
    for (uint32_t u = rank; u < total; u += a.total_waves) {
        const uint32_t frame = u / grid_y;
        const int32_t iy = (int32_t)(u - frame * grid_y);
        // ---- the frame's search state: stopped?  below its minSize (the loop's break, :1375-1380)?  its ranges (:1407-1415)
        const uint32_t phase = state[frame].phase;
        if (phase == 2u) continue;
        const int32_t min_w = phase == 0u ? b.min_w : state[frame].min_w, min_h = phase == 0u ? b.min_h : state[frame].min_h;
        if ((int32_t)win_w < min_w || (int32_t)win_h < min_h) continue;
        int32_t start_x = 0, start_y = 0, end_x = (int32_t)grid_x, end_y = (int32_t)grid_y;
        if (phase == 1u) {
            const int32_t rx = state[frame].roi_x, ry = state[frame].roi_y, rw = state[frame].roi_w, rh = state[frame].roi_h;
            start_y = cv_round((double)ry / ystep);
            end_y = min(cv_round((double)(ry + rh - (int32_t)win_h) / ystep), (int32_t)grid_y);   // (the scanROI lies inside the frame:
            start_x = cv_round((double)rx / ystep);                                              //  its ranges inside the grid's)
            end_x = min(cv_round((double)(rx + rw - (int32_t)win_w) / ystep), (int32_t)grid_x);
        }
        if (iy < start_y || iy >= end_y || start_x >= end_x) continue;
        const uint32_t n_pos = (uint32_t)(end_x - start_x);
        const rsrc_t sq_f = make_rsrc(a.sqsum + (size_t)frame * a.frame_elems, frame_bytes4 * 2u);
        const uint32_t frame_bytes = frame * frame_bytes4;
        const uint32_t y = (uint32_t)cv_round((double)iy * ystep);
        const bool row_border = y + win_h >= a.sum_h;   // pt.y + height >= sum.height -> -1 (tempcv.cpp:817-820)
        uint32_t carry = 0;   // the walk starts with ixstep = 1 at startX of every row
        uint32_t n_q = 0;
        for (uint32_t j0 = 0; j0 < n_pos; j0 += 64u) {
            const bool valid = j0 + lane < n_pos;
            const uint32_t ix = (uint32_t)start_x + (valid ? j0 + lane : 0u);
            const uint32_t x = (uint32_t)cv_round((double)ix * ystep);
            const bool border = row_border || x + win_w >= a.stride;
            const uint32_t po = y * a.stride + x;
            const uint32_t off = frame_bytes + po * 4u;
            double vnf = 1.0;
            const bool eval = valid && !border;
            if (eval) cv_window_vnf(img, sq_f, off, po, q0, q1, q2, q3, inv_area, vnf);
            const uint32_t n_valid = min(64u, n_pos - j0);
            if (STAGE_TREE) {
                // the whole stage tree for every position of the range (tempcv.cpp:834-861: any reject returns 0 and skips): every
                // lane carries the stage it visits next; the stages are swept once in a topological order of the pass / fail graph
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
                const unsigned long long F = __ballot(ptr == -2);
                const bool visited = cv_visited(F, lane, n_valid, carry);
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
                if (am != 0ull) cv_big_emit(b, frame, am, hit, x, y, lane);
                continue;
            }
            bool fail0 = false;
            if (eval)
                fail0 = !(cv_stage_sum_mode<TREES>(img, timg, table + stages[0].first_node, stages[0].n_nodes, off, vnf, stages[0].cv_f64, a.tree2) >= thr0);
            const unsigned long long F = __ballot(fail0);
            const bool visited = cv_visited(F, lane, n_valid, carry);
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
            if (n_q > (uint32_t)CV_QCAP - 64u || (j0 + 64u >= n_pos && n_q != 0u)) {
                // the later stages on the queued survivors; who passes them all is a candidate
                cv_flush_to<TREES, COUNT>(a, img, timg, table, q, n_q, lane, [&](const CvQEntry* qq, uint32_t m) {
                    for (uint32_t i0 = 0; i0 < m; i0 += 64u) {
                        const bool mine = i0 + lane < m;
                        const uint32_t xy = qq[mine ? i0 + lane : 0u].xy;
                        cv_big_emit(b, frame, __ballot(mine), mine, xy & 0xffffu, xy >> 16, lane);
                    }
                });
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The step after each scale (tempcv.cpp:1422-1454) for one frame: all candidates so far, grouped; the first group of strictly
// greatest area is maxRect.  The candidates' canonical order is the walk's: (scale slot, y, x).
__global__ __launch_bounds__(GROUP_THREADS) void cv_biggest_update(CvBigArgs b) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const GroupLds L = group_lds(lds);
    const uint32_t frame = blockIdx.x, tid = threadIdx.x;
    CvBigState* st = b.state + frame;
    if (st->phase != 0u) return;   // found earlier (scanROI.area() != 0), or stopped
    const uint32_t n = b.frame_count[frame];
    if (n == 0u || n == st->n_seen) return;   // allCandidates.empty(), or the list the last grouping saw
    __syncthreads();                           // (everyone has read the state before thread 0 writes it)
    if (n > b.cv.det_cap || n > GROUP_MAX) {
        if (tid == 0u) {
            st->flags = n > b.cv.det_cap ? CV_BIG_OVERFLOW : CV_BIG_LIMIT;
            st->phase = 2u;
        }
        return;
    }
    const CvDet* det = b.cv.det + (size_t)frame * b.cv.det_cap;
    const uint32_t stride = b.cv.stride;
    const CvScaleDev* scales = b.cv.scales;
    uint32_t ncls = 0;
    const uint32_t n_out = group_classes(
        L, n, b.threshold, b.eps, [&](uint32_t i) { return (uint64_t)det[i].slot << 32 | (uint64_t)(det[i].y * stride + det[i].x); },
        [&](uint64_t key, int32_t* x, int32_t* y, int32_t* w, int32_t* h) {
            const uint32_t slot = (uint32_t)(key >> 32), el = (uint32_t)key;
            const uint32_t yy = el / stride;
            *x = (int32_t)(el - yy * stride);
            *y = (int32_t)yy;
            *w = (int32_t)scales[slot].win_w;
            *h = (int32_t)scales[slot].win_h;
        },
        &ncls);
    if (tid != 0u) return;
    if (n_out == 0u) {
        st->n_seen = n;
        return;
    }
    int32_t mx = 0, my = 0, mw = 0, mh = 0;
    for (uint32_t c = 0; c < ncls; ++c)   // the surviving classes in their order: the first of strictly greatest area
        if (L.label[c] != 0u && L.cw[c] * L.ch[c] > mw * mh) {
            mx = L.cx[c];
            my = L.cy[c];
            mw = L.cw[c];
            mh = L.ch[c];
        }
    // scanROI = maxRect widened by a fifth on every side, inside the frame (:1442-1448); minSize (:1450-1452)
    const int32_t dx = cv_round((double)mw * b.eps), dy = cv_round((double)mh * b.eps);
    const int32_t rx = max(mx - dx, 0), ry = max(my - dy, 0);
    const double min_scale = b.rough != 0u ? 0.6 : 0.4;
    st->max_x = mx;
    st->max_y = my;
    st->max_w = mw;
    st->max_h = mh;
    st->roi_x = rx;
    st->roi_y = ry;
    st->roi_w = min(mw + dx * 2, (int32_t)b.width - 1 - rx);
    st->roi_h = min(mh + dy * 2, (int32_t)b.height - 1 - ry);
    st->min_w = cv_round((double)mw * min_scale);
    st->min_h = cv_round((double)mh * min_scale);
    st->hit_slot = b.slot;
    st->phase = 1u;
}

int prepare_cv_biggest_kernels() {
    return (int)hipFuncSetAttribute((const void*)cv_biggest_update, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GROUP_LDS_BYTES);
}

template <bool TREES, bool STAGE_TREE>
static void cv_big_launch(const CvBigArgs& a, bool count, dim3 g, dim3 b, hipStream_t stream) {
    if (count) hipLaunchKernelGGL((cv_biggest_pass<TREES, true, STAGE_TREE>), g, b, 0, stream, a);
    else       hipLaunchKernelGGL((cv_biggest_pass<TREES, false, STAGE_TREE>), g, b, 0, stream, a);
}

int launch_cv_biggest_round(const CvBigArgs& a, bool trees, bool count, bool stage_tree, int n_blocks, bool update, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    dim3 g(n_blocks), b(CV_WAVES_PER_BLOCK * 64);
    if (stage_tree) {
        if (trees) cv_big_launch<true, true>(a, count, g, b, stream);
        else       cv_big_launch<false, true>(a, count, g, b, stream);
    } else {
        if (trees) cv_big_launch<true, false>(a, count, g, b, stream);
        else       cv_big_launch<false, false>(a, count, g, b, stream);
    }
    if (update) hipLaunchKernelGGL(cv_biggest_update, dim3(a.cv.n_frames), dim3(GROUP_THREADS), GROUP_LDS_BYTES, stream, a);
    return (int)hipGetLastError();
}

}  // namespace vj
