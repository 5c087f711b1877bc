// vj_paint_yuv: the rectangles of a call painted into NV12 / NV21 / I420 frames in place.  The planner
// (vj_paint_yuv_host.cpp) checks the call and lays out one record per (region, plane); here a slice of the call — all frames that hold
// a region unless "max_subbatch" is set — is one copy (its records, its overlap lists and, of every plane of a host frame, the rows
// its records touch, gathered at a 4-byte pitch in the lane's page-locked staging buffer), ONE phase-1 launch and ONE phase-2 launch
// for all planes, and for host frames one copy back, of which only the rectangle's span of every touched row is written to the
// caller's memory.  Device-resident planes are painted where they lie.  The block lives in d_extract as vj_paint's does:
// [records | overlap lists | staged rows | scratch].
#include "vj_env_internal.hpp"
#include "vj_paint_yuv_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

struct StagedPlane { int frame; uint32_t id; int32_t y0, y1; size_t at, pitch; };

int run_paint_yuv_slice(vj_env* e, const vj_yuv_image* frames, const PaintYuvLayout& lay, size_t first, size_t end, PaintYuvSlice* sl) {
    int rc;
    if ((rc = paint_yuv_plan_slice(frames, lay, first, end, sl))) return rc;
    const size_t n = sl->recs.size();
    if (n == 0) return VJ_OK;
    const size_t rec_bytes = align16(n * sizeof(PaintYuvRec)), ovl_bytes = align16(sl->overlaps.size() * sizeof(uint32_t));
    auto frame_of = [&](size_t i) { return lay.luma.clipped[(size_t)sl->region[i]].frame; };
    // the rows of every plane of a host frame that its records touch
    std::vector<StagedPlane> staged;
    size_t up_bytes = rec_bytes + ovl_bytes;
    for (int fi : sl->frames) {
        const vj_yuv_image& f = frames[fi];
        if (f.on_device) continue;
        for (uint32_t id = 0; id < 3u; ++id) {
            const PaintYuvPlane q = paint_yuv_plane(f, id);
            if (!q.p) continue;
            StagedPlane s{fi, id, q.h, 0, up_bytes, (((size_t)q.w * q.comps) + 3u) & ~(size_t)3};
            for (size_t i = 0; i < n; ++i)
                if (frame_of(i) == fi && sl->recs[i].plane_id == id) {
                    s.y0 = std::min(s.y0, sl->recs[i].ky0);
                    s.y1 = std::max(s.y1, sl->recs[i].ky1);
                }
            if (s.y1 <= s.y0) continue;
            up_bytes = align16(up_bytes + s.pitch * (size_t)(s.y1 - s.y0));
            staged.push_back(s);
        }
    }
    const size_t stage_bytes = up_bytes - (rec_bytes + ovl_bytes);
    const uint64_t total = (uint64_t)up_bytes + sl->scratch_bytes;
    Lane* L = &e->lane0;
    if (L->h_stage_bytes < up_bytes) {
        if (L->h_stage) (void)hipHostFree(L->h_stage);
        L->h_stage = nullptr;
        L->h_stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&L->h_stage, up_bytes, hipHostMallocDefault));
        L->h_stage_bytes = up_bytes;
    }
    if ((rc = e->d_extract.ensure((size_t)total))) return rc;
    uint8_t* hs = (uint8_t*)L->h_stage;
    uint8_t* dev = (uint8_t*)e->d_extract.p;
    for (const StagedPlane& s : staged) {
        const PaintYuvPlane q = paint_yuv_plane(frames[s.frame], s.id);
        const size_t row_bytes = (size_t)q.w * q.comps;
        for (int32_t y = s.y0; y < s.y1; ++y) memcpy(hs + s.at + (size_t)(y - s.y0) * s.pitch, q.p + (size_t)y * q.stride, row_bytes);
        for (size_t i = 0; i < n; ++i)
            if (frame_of(i) == s.frame && sl->recs[i].plane_id == s.id) {
                PaintYuvRec& d = sl->recs[i];
                d.plane = dev + s.at;
                d.stride = (uint32_t)s.pitch;
                d.row0 = s.y0;
            }
    }
    memcpy(hs, sl->recs.data(), n * sizeof(PaintYuvRec));
    if (!sl->overlaps.empty()) memcpy(hs + rec_bytes, sl->overlaps.data(), sl->overlaps.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(dev, hs, up_bytes, hipMemcpyHostToDevice, e->stream));
    PaintYuvArgs a;
    memset(&a, 0, sizeof(a));
    a.recs = (const PaintYuvRec*)dev;
    a.overlaps = (const uint32_t*)(dev + rec_bytes);
    a.n_recs = (uint32_t)n;
    a.n_overlaps = (uint32_t)sl->overlaps.size();
    a.n_units = sl->n_units;
    a.n_pre_units = sl->n_pre_units;
    a.scratch = dev + up_bytes;
    a.scratch_bytes = sl->scratch_bytes;
    a.mode = lay.luma.mode;
    a.ellipse = lay.luma.ellipse ? 1u : 0u;
    const int hrc = launch_paint_yuv(a, e->stream);
    if (hrc) {
        set_error("paint_yuv launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (stage_bytes != 0) {
        HIP_TRY(hipMemcpyAsync(hs + rec_bytes + ovl_bytes, dev + rec_bytes + ovl_bytes, stage_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        // the rectangle's span of every touched row goes back: never a row's padding, never a row outside the rectangle
        for (size_t i = 0; i < n; ++i) {
            const PaintYuvRec& d = sl->recs[i];
            const vj_yuv_image& f = frames[frame_of(i)];
            if (f.on_device) continue;
            const PaintYuvPlane q = paint_yuv_plane(f, d.plane_id);
            const size_t x0 = (size_t)d.kx0 * d.comps, span = (size_t)(d.kx1 - d.kx0) * d.comps;
            const uint8_t* src = hs + (size_t)(d.plane - dev);
            uint8_t* dst = const_cast<uint8_t*>(q.p);
            for (int32_t y = d.ky0; y < d.ky1; ++y)
                memcpy(dst + (size_t)y * q.stride + x0, src + (size_t)(y - d.row0) * d.stride + x0, span);
        }
    }
    return VJ_OK;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_paint_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p) {
    if (!e || !p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && !regions)) {
        set_error("vj_paint_yuv: null argument");
        return VJ_ERR_ARG;
    }
    PaintYuvLayout lay;
    int rc = paint_yuv_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    if (n_regions == 0 || lay.luma.touched.empty()) return VJ_OK;
    HIP_TRY(hipSetDevice(e->device));
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    PaintYuvSlice sl;
    HIP_TRY(hipEventRecord(e->paint_ev[0], e->stream));
    for (size_t first = 0; first < lay.luma.touched.size();) {
        const size_t end = paint_slice_end(lay.luma, first, max_frames);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = run_paint_yuv_slice(e, frames, lay, first, end, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
        first = end;
    }
    HIP_TRY(hipEventRecord(e->paint_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->paint_ev[0], e->paint_ev[1]));
    e->paint_yuv_ms = ms;
    return VJ_OK;
}

int vj_paint_yuv_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->paint_yuv_ms;
    return VJ_OK;
}

}  // extern "C"
