// vj_paint: the pixels inside, or around, the rectangles of a call changed in place.  The planner
// (vj_paint_host.cpp) checks the call, maps and clips the regions; here a slice of the call — all frames that hold a region unless
// "max_subbatch" is set: then runs of at most that many — goes through the shared paint slice (vj_slice.hpp, §4.24) with a frame as
// one plane: of every host frame the rows its regions touch are staged, the phase-1 launch reads frames into scratch (BLUR,
// PIXELATE), the phase-2 launch writes frames from scratch, and only K's span of every touched row is written to the caller's memory.
#include "vj_slice.hpp"
#include "vj_paint_host.hpp"

namespace vj {

namespace {

int run_slice(vj_env* e, const vj_image* frames, const PaintLayout& lay, size_t first, size_t end, PaintSlice* sl) {
    int rc;
    if ((rc = paint_plan_slice(frames, lay, first, end, sl))) return rc;
    std::vector<TouchedRows> planes;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (!f.on_device) planes.push_back(touched_plane(fi, 0u, f.data, (size_t)f.stride, (size_t)f.width * (size_t)image_channels(f), f.height));
    }
    std::vector<RowSpan> spans;
    for (size_t i = 0; i < sl->recs.size(); ++i) {
        const PaintRegionDev& d = sl->recs[i];
        spans.push_back(RowSpan{lay.clipped[(size_t)sl->region[i]].frame, 0u, d.cy0, d.cy1, (size_t)d.cx0 * d.channels, (size_t)(d.cx1 - d.cx0) * d.channels, -1});
    }
    return run_paint_slice(
        e, sl->recs, sl->overlaps, sl->scratch_bytes, std::move(planes), std::move(spans),
        [](PaintRegionDev& d, uint8_t* rows, uint32_t pitch, int32_t row0) {
            d.frame = rows;
            d.stride = pitch;
            d.row0 = row0;
        },
        [&](const uint8_t* dev, const uint32_t* overlaps, uint8_t* scratch) {
            PaintArgs a;
            memset(&a, 0, sizeof(a));
            a.regions = (const PaintRegionDev*)dev;
            a.overlaps = overlaps;
            a.n_regions = (uint32_t)sl->recs.size();
            a.n_overlaps = (uint32_t)sl->overlaps.size();
            a.n_units = sl->n_units;
            a.n_pre_units = sl->n_pre_units;
            a.scratch = scratch;
            a.scratch_bytes = sl->scratch_bytes;
            a.mode = lay.mode;
            a.ellipse = lay.ellipse ? 1u : 0u;
            a.color = lay.color;
            const int hrc = launch_paint(a, e->stream);
            if (hrc) {
                set_error("paint launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return (int)VJ_ERR_HIP;
            }
            return (int)VJ_OK;
        });
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
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    PaintSlice sl;
    return run_slices(
        e, e->call_ev, &e->paint_ms, lay.touched.size(), [&](size_t first) { return paint_slice_end(lay, first, max_frames); },
        [&](size_t first, size_t end) { return run_slice(e, frames, lay, first, end, &sl); });
}

int vj_paint_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->paint_ms;
    return VJ_OK;
}

}  // extern "C"
