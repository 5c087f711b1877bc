// vj_extract_yuv / vj_extract_affine_yuv: regions of the call's NV12 / NV21 / I420 frames, decoded tap by tap and
// resized (or warped) to one size, written into a device buffer of the caller's — vj_extract of vj_yuv_to_bgr without the BGR copy.
// The planner (vj_extract_yuv_host.cpp) checks the call with the planners of those two; here a slice of the call — all of it unless
// "max_subbatch" is set: then runs of regions that name at most that many distinct frames — is one copy (its region records, its taps
// and every plane of the host frames it names, gathered at a 4-byte pitch in the lane's page-locked staging buffer) and one launch.
// Device-resident planes are read where they lie.  The device block is vj_extract's (d_extract), the call's skeleton the shared one
// (vj_slice.hpp, §4.24).
#include "vj_slice.hpp"
#include "vj_extract_yuv_host.hpp"

namespace vj {

namespace {

// One slice of either call: [records | taps | planes of the host frames in `named`] in one copy, then launch(block, taps).
// frame_of(i): the frame record i of the slice names.
template <typename Rec, typename FrameOf, typename Launch>
int enqueue_slice(vj_env* e, const vj_yuv_image* frames, std::vector<Rec>& recs, const std::vector<PyrTap>& taps, const std::vector<int>& named,
                  FrameOf frame_of, Launch launch) {
    const size_t n = recs.size();
    StageBlock head;
    head.section(n * sizeof(Rec));
    const size_t tap_at = head.section(taps.size() * sizeof(PyrTap));
    StageBlock b = head;
    for (int fi : named) {
        const vj_yuv_image& f = frames[fi];
        if (f.on_device) continue;
        b.rows((size_t)f.width, (size_t)f.height);
        b.rows(yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width), (f.layout == VJ_YUV_I420 ? 2u : 1u) * ((size_t)f.height / 2u));
    }
    int rc;
    if ((rc = stage_reserve(&e->lane0, b.bytes))) return rc;
    if ((rc = e->d_extract.ensure(b.bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_extract.p;
    b = head;
    for (int fi : named) {
        const vj_yuv_image& f = frames[fi];
        if (f.on_device) continue;
        const size_t crow = yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width), crows = (size_t)f.height / 2u;
        const uint8_t* y = dev + stage_rows(hs, &b, f.y, (size_t)f.y_stride, (size_t)f.height, (size_t)f.width);
        const uint8_t* c0 = dev + stage_rows(hs, &b, f.c0, (size_t)f.c_stride, crows, crow);
        const uint8_t* c1 = f.layout == VJ_YUV_I420 ? dev + stage_rows(hs, &b, f.c1, (size_t)f.c_stride, crows, crow) : nullptr;
        for (size_t i = 0; i < n; ++i)
            if (frame_of(i) == fi) {
                YuvPlanesDev& d = recs[i].f;
                d.y = y, d.c0 = c0, d.c1 = c1;
                d.y_stride = (uint32_t)align4((size_t)f.width);
                d.c_stride = (uint32_t)align4(crow);
            }
    }
    memcpy(hs, recs.data(), n * sizeof(Rec));
    if (!taps.empty()) memcpy(hs + tap_at, taps.data(), taps.size() * sizeof(PyrTap));
    HIP_TRY(hipMemcpyAsync(e->d_extract.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
    return launch(dev, (const PyrTap*)(dev + tap_at));
}

template <typename Layout>
ExtractYuvArgs args_of(const Layout& lay, const YuvSource& src, const uint8_t* dev, size_t n, uint32_t n_units, uint8_t* d_dst) {
    ExtractYuvArgs a;
    memset(&a, 0, sizeof(a));
    a.regions = dev;
    a.n_regions = (uint32_t)n;
    a.n_units = n_units;
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    a.out_w = lay.out_w;
    a.out_h = lay.out_h;
    a.C = lay.C;
    a.gray = lay.gray ? 1u : 0u;
    a.planar = lay.planar ? 1u : 0u;
    a.swap_rb = src.swap_rb ? 1u : 0u;
    a.rows = lay.rows;
    a.row_bytes = lay.row_bytes;
    return a;
}

int launched(const char* what, int hrc) {
    if (!hrc) return VJ_OK;
    set_error("%s launch failed: %s", what, hipGetErrorString((hipError_t)hrc));
    return VJ_ERR_HIP;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_extract_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                   const vj_yuv_params* yp, uint8_t* d_dst, uint64_t dst_bytes) {
    if (!e || !p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && (!regions || !d_dst))) {
        set_error("vj_extract_yuv: null argument");
        return VJ_ERR_ARG;
    }
    ExtractYuvLayout lay;
    int rc = extract_yuv_layout(frames, n_frames, regions, n_regions, p, yp, &lay);
    if (rc) return rc;
    if (n_regions == 0) return VJ_OK;
    if ((rc = check_dst("vj_extract_yuv", frames, n_frames, d_dst, dst_bytes, lay.lay.bytes, false, yuv_decode_check_overlap))) return rc;
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    ExtractYuvSlice sl;
    return run_slices(
        e, e->call_ev, &e->extract_yuv_ms, (size_t)n_regions, [&](size_t first) { return extract_slice_end(regions, (size_t)n_regions, first, max_frames); },
        [&](size_t first, size_t end) {
            int src;
            if ((src = extract_yuv_plan_slice(frames, regions, lay, first, end - first, &sl))) return src;
            return enqueue_slice(
                e, frames, sl.recs, sl.luma.taps, sl.luma.frames, [&](size_t i) { return regions[first + i].frame; },
                [&](const uint8_t* dev, const PyrTap* taps) {
                    ExtractYuvArgs a = args_of(lay.lay, lay.src, dev, sl.recs.size(), sl.luma.n_units, d_dst);
                    a.taps = taps;
                    return launched("extract_yuv", launch_extract_yuv(a, e->stream));
                });
        });
}

int vj_extract_affine_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                          const vj_yuv_params* yp, uint8_t* d_dst, uint64_t dst_bytes) {
    if (!e || !p || n_frames < 0 || n < 0 || (n_frames > 0 && !frames) || (n > 0 && (!affines || !d_dst))) {
        set_error("vj_extract_affine_yuv: null argument");
        return VJ_ERR_ARG;
    }
    AffineYuvLayout lay;
    int rc = affine_yuv_layout(frames, n_frames, affines, n, p, yp, &lay);
    if (rc) return rc;
    if (n == 0) return VJ_OK;
    if ((rc = check_dst("vj_extract_affine_yuv", frames, n_frames, d_dst, dst_bytes, lay.lay.bytes, false, yuv_decode_check_overlap))) return rc;
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    AffineYuvSlice sl;
    const std::vector<PyrTap> no_taps;
    return run_slices(
        e, e->call_ev, &e->extract_yuv_ms, (size_t)n, [&](size_t first) { return affine_slice_end(affines, (size_t)n, first, max_frames); },
        [&](size_t first, size_t end) {
            int src;
            if ((src = affine_yuv_plan_slice(frames, affines, lay, first, end - first, &sl))) return src;
            return enqueue_slice(
                e, frames, sl.recs, no_taps, sl.luma.frames, [&](size_t i) { return affines[first + i].frame; },
                [&](const uint8_t* dev, const PyrTap*) {
                    const ExtractYuvArgs a = args_of(lay.lay, lay.src, dev, sl.recs.size(), sl.luma.n_units, d_dst);
                    return launched("affine_yuv", launch_affine_yuv(a, e->stream));
                });
        });
}

int vj_extract_yuv_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->extract_yuv_ms;
    return VJ_OK;
}

}  // extern "C"
