// vj_paint_yuv: the rectangles of a call painted into NV12 / NV21 / I420 frames in place.  The planner
// (vj_paint_yuv_host.cpp) checks the call and lays out one record per (region, plane); here a slice of the call — all frames that hold
// a region unless "max_subbatch" is set — goes through the shared paint slice (vj_slice.hpp, §4.24) with a frame as up to three
// planes: of every plane of a host frame the rows its records touch are staged, ONE phase-1 launch and ONE phase-2 launch serve all
// planes, and only the rectangle's span of every touched row is written to the caller's memory.
#include "vj_slice.hpp"
#include "vj_paint_yuv_host.hpp"

namespace vj {

namespace {

int run_slice(vj_env* e, const vj_yuv_image* frames, const PaintYuvLayout& lay, size_t first, size_t end, PaintYuvSlice* sl) {
    int rc;
    if ((rc = paint_yuv_plan_slice(frames, lay, first, end, sl))) return rc;
    std::vector<TouchedRows> planes;
    for (int fi : sl->frames) {
        if (frames[fi].on_device) continue;
        for (uint32_t id = 0; id < 3u; ++id) {
            const PaintYuvPlane q = paint_yuv_plane(frames[fi], id);
            if (q.p) planes.push_back(touched_plane(fi, id, q.p, (size_t)q.stride, (size_t)q.w * q.comps, q.h));
        }
    }
    std::vector<RowSpan> spans;
    for (size_t i = 0; i < sl->recs.size(); ++i) {
        const PaintYuvRec& d = sl->recs[i];
        spans.push_back(RowSpan{lay.luma.clipped[(size_t)sl->region[i]].frame, d.plane_id, d.ky0, d.ky1, (size_t)d.kx0 * d.comps, (size_t)(d.kx1 - d.kx0) * d.comps, -1});
    }
    return run_paint_slice(
        e, sl->recs, sl->overlaps, sl->scratch_bytes, std::move(planes), std::move(spans),
        [](PaintYuvRec& d, uint8_t* rows, uint32_t pitch, int32_t row0) {
            d.plane = rows;
            d.stride = pitch;
            d.row0 = row0;
        },
        [&](const uint8_t* dev, const uint32_t* overlaps, uint8_t* scratch) {
            PaintYuvArgs a;
            memset(&a, 0, sizeof(a));
            a.recs = (const PaintYuvRec*)dev;
            a.overlaps = overlaps;
            a.n_recs = (uint32_t)sl->recs.size();
            a.n_overlaps = (uint32_t)sl->overlaps.size();
            a.n_units = sl->n_units;
            a.n_pre_units = sl->n_pre_units;
            a.scratch = scratch;
            a.scratch_bytes = sl->scratch_bytes;
            a.mode = lay.luma.mode;
            a.ellipse = lay.luma.ellipse ? 1u : 0u;
            const int hrc = launch_paint_yuv(a, e->stream);
            if (hrc) {
                set_error("paint_yuv launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return (int)VJ_ERR_HIP;
            }
            return (int)VJ_OK;
        });
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
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    PaintYuvSlice sl;
    return run_slices(
        e, e->call_ev, &e->paint_yuv_ms, lay.luma.touched.size(), [&](size_t first) { return paint_slice_end(lay.luma, first, max_frames); },
        [&](size_t first, size_t end) { return run_slice(e, frames, lay, first, end, &sl); });
}

int vj_paint_yuv_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->paint_yuv_ms;
    return VJ_OK;
}

}  // extern "C"
