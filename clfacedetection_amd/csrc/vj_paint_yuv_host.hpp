// Host planner of vj_paint_yuv / vj_paint_yuv_layout that needs no device.  The luma side IS vj_paint's planner
// (paint_layout on the Y planes as gray frames: the region and parameter checks, M, K, the sizes, the touched frames); this file adds
// the 4:2:0 frame checks (vj_yuv_to_bgr's), the plane ownership check, the colour, Kc and the chroma sizes, and per slice one record
// per (region, plane) with the overlap lists of every plane.  Compiled without HIP too: tests/paint_yuv_asan_driver.cpp runs it
// under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_paint_host.hpp"
#include "vj_paint_yuv_units.hpp"

#include <vector>

namespace vj {

struct PaintYuvLayout {
    PaintLayout luma;                // vj_paint's layout of the Y planes: mapped M, clipped K, sizes, touched frames
    std::vector<vj_roi> chroma;      // Kc per region as (frame, x, y, w, h) in chroma samples; w = h = 0 when K is empty
    std::vector<int32_t> csizes;     // the chroma size per region: sc, kkc, t (OUTLINE), 0 (FILL)
    uint8_t yc = 0, uc = 0, vc = 0;  // FILL, OUTLINE: color[0..2] = B, G, R through §4.21's encode formulas
    uint64_t scratch_bytes = 0;      // of the call as one slice: per region the Y plane and the two chroma components, each rounded to 16
};
// Checks `frames` (vj_yuv_to_bgr's rules, and that no two planes of the call overlap), `regions` and `p` (vj_paint's rules).
// VJ_ERR_ARG / VJ_ERR_LIMIT with vj_last_error naming the frame, the row or the field.
int paint_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                     PaintYuvLayout* out);

// The slice of touched frames [first, end) (paint_slice_end gives `end`): its records — `plane`, `stride` and `row0` are the plane's
// own, the caller replaces those of the host planes it stages —, the overlap lists, and per record the region it stands for.
struct PaintYuvSlice {
    std::vector<PaintYuvRec> recs;
    std::vector<uint32_t> overlaps;
    std::vector<int> region;         // index in the call, per record
    std::vector<int> frames;         // lay.luma.touched[first .. end)
    uint32_t n_units = 0, n_pre_units = 0;
    uint64_t scratch_bytes = 0;
};
int paint_yuv_plan_slice(const vj_yuv_image* frames, const PaintYuvLayout& lay, size_t first, size_t end, PaintYuvSlice* out);

// Plane `id` (PAINT_YUV_PLANE_*) of a frame: its first byte (null: the layout has no such plane), stride, components and size in samples
struct PaintYuvPlane { const uint8_t* p; uint32_t stride, comps; int32_t w, h; };
PaintYuvPlane paint_yuv_plane(const vj_yuv_image& f, uint32_t id);

}  // namespace vj
