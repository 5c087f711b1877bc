// vj_paint: the pixels inside, or around, the rectangles of a call changed in place.  The planner
// (vj_paint_host.cpp) checks the call, maps and clips the regions; here a slice of the call — all frames that hold a region unless
// "max_subbatch" is set: then runs of at most that many — is one copy (its region records, its overlap lists and, of every host
// frame it names, the rows its regions touch, gathered at a 4-byte pitch in the lane's page-locked staging buffer), the phase-1
// launch that reads frames into scratch (BLUR, PIXELATE), the phase-2 launch that writes frames from scratch, and for host frames
// one copy back, of which only K's span of every touched row is written to the caller's memory.  Device-resident frames are painted
// where they lie.  The block lives in d_extract, which vj_extract and vj_extract_affine use the same way: [records | overlap lists |
// staged rows | scratch].
#include "vj_env_internal.hpp"
#include "vj_paint_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

struct StagedFrame { int frame; int32_t y0, y1; size_t at, pitch; };

int run_paint_slice(vj_env* e, const vj_image* frames, const PaintLayout& lay, size_t first, size_t end, PaintSlice* sl) {
    int rc;
    if ((rc = paint_plan_slice(frames, lay, first, end, sl))) return rc;
    const size_t n = sl->recs.size();
    if (n == 0) return VJ_OK;
    const size_t rec_bytes = align16(n * sizeof(PaintRegionDev)), ovl_bytes = align16(sl->overlaps.size() * sizeof(uint32_t));
    // the rows of every host frame that its regions touch
    std::vector<StagedFrame> staged;
    size_t up_bytes = rec_bytes + ovl_bytes;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (f.on_device) continue;
        StagedFrame s{fi, f.height, 0, up_bytes, (((size_t)f.width * (size_t)image_channels(f)) + 3u) & ~(size_t)3};
        for (size_t i = 0; i < n; ++i)
            if (lay.clipped[(size_t)sl->region[i]].frame == fi) {
                s.y0 = std::min(s.y0, sl->recs[i].cy0);
                s.y1 = std::max(s.y1, sl->recs[i].cy1);
            }
        if (s.y1 <= s.y0) continue;
        up_bytes = align16(up_bytes + s.pitch * (size_t)(s.y1 - s.y0));
        staged.push_back(s);
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
    for (const StagedFrame& s : staged) {
        const vj_image& f = frames[s.frame];
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f);
        for (int32_t y = s.y0; y < s.y1; ++y) memcpy(hs + s.at + (size_t)(y - s.y0) * s.pitch, f.data + (size_t)y * (size_t)f.stride, row_bytes);
        for (size_t i = 0; i < n; ++i)
            if (lay.clipped[(size_t)sl->region[i]].frame == s.frame) {
                PaintRegionDev& d = sl->recs[i];
                d.frame = dev + s.at;
                d.stride = (uint32_t)s.pitch;
                d.row0 = s.y0;
            }
    }
    memcpy(hs, sl->recs.data(), n * sizeof(PaintRegionDev));
    if (!sl->overlaps.empty()) memcpy(hs + rec_bytes, sl->overlaps.data(), sl->overlaps.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(dev, hs, up_bytes, hipMemcpyHostToDevice, e->stream));
    PaintArgs a;
    memset(&a, 0, sizeof(a));
    a.regions = (const PaintRegionDev*)dev;
    a.overlaps = (const uint32_t*)(dev + rec_bytes);
    a.n_regions = (uint32_t)n;
    a.n_overlaps = (uint32_t)sl->overlaps.size();
    a.n_units = sl->n_units;
    a.n_pre_units = sl->n_pre_units;
    a.scratch = dev + up_bytes;
    a.scratch_bytes = sl->scratch_bytes;
    a.mode = lay.mode;
    a.ellipse = lay.ellipse ? 1u : 0u;
    a.color = lay.color;
    const int hrc = launch_paint(a, e->stream);
    if (hrc) {
        set_error("paint launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (stage_bytes != 0) {
        HIP_TRY(hipMemcpyAsync(hs + rec_bytes + ovl_bytes, dev + rec_bytes + ovl_bytes, stage_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        // K's span of every touched row goes back: never a row's padding, never a row outside K
        for (size_t i = 0; i < n; ++i) {
            const PaintRegionDev& d = sl->recs[i];
            const vj_image& f = frames[lay.clipped[(size_t)sl->region[i]].frame];
            if (f.on_device) continue;
            const size_t x0 = (size_t)d.cx0 * d.channels, span = (size_t)(d.cx1 - d.cx0) * d.channels;
            const uint8_t* src = hs + (size_t)(d.frame - dev);
            uint8_t* dst = const_cast<uint8_t*>(f.data);
            for (int32_t y = d.cy0; y < d.cy1; ++y)
                memcpy(dst + (size_t)y * (size_t)f.stride + x0, src + (size_t)(y - d.row0) * d.stride + x0, span);
        }
    }
    return VJ_OK;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_paint(vj_env* e, const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p) {
    if (!e || !p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && !regions)) {
        set_error("vj_paint: null argument");
        return VJ_ERR_ARG;
    }
    PaintLayout lay;
    int rc = paint_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    if (n_regions == 0 || lay.touched.empty()) return VJ_OK;
    HIP_TRY(hipSetDevice(e->device));
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    PaintSlice sl;
    HIP_TRY(hipEventRecord(e->paint_ev[0], e->stream));
    for (size_t first = 0; first < lay.touched.size();) {
        const size_t end = paint_slice_end(lay, first, max_frames);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = run_paint_slice(e, frames, lay, first, end, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
        first = end;
    }
    HIP_TRY(hipEventRecord(e->paint_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->paint_ev[0], e->paint_ev[1]));
    e->paint_ms = ms;
    return VJ_OK;
}

int vj_paint_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->paint_ms;
    return VJ_OK;
}

}  // extern "C"
