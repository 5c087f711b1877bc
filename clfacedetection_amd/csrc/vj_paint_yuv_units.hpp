// Records the kernels of vj_paint_yuv (vj_paint_yuv.hip) share with the host code that builds them
// (vj_paint_yuv_host.cpp, compiled without HIP for the sanitizer runs): plain PODs and the arithmetic both sides use.  The block
// and band sizes, the limits, the unit arithmetic and the painted-set test are vj_paint's (vj_paint_units.hpp).
#pragma once
#include "vj_paint_units.hpp"

namespace vj {

enum : uint32_t { PAINT_YUV_PLANE_Y = 0, PAINT_YUV_PLANE_C0 = 1, PAINT_YUV_PLANE_C1 = 2 };

// One (region, plane) of a slice whose K is not empty.  A plane is an image of `comps` interleaved components: the Y plane and the
// U and V planes of I420 have one, the pair plane of NV12 / NV21 two.  The records of a slice are ordered by frame, then by the
// region's index in the call, then by plane: "later" in the call is "later" among the records of a plane.
struct PaintYuvRec {
    uint8_t* plane;          // a device address: the caller's device-resident plane, or the plane's rows in the slice's staged block
    uint64_t scratch_off;    // byte offset of the record's phase-1 output in the scratch (a multiple of 16)
    uint32_t stride;         // bytes per plane row
    uint32_t comps;          // 1 or 2
    int32_t  pw, ph;         // the plane's size in samples; a staged plane holds rows [row0, ph) only from `plane` on
    int32_t  X0, Y0, Wm, Hm; // the mapped rectangle M, in luma pixels
    int32_t  cx0, cy0, cx1, cy1;   // K = M ∩ frame, in luma pixels, not empty
    int32_t  size;           // the LUMA size: t (OUTLINE) — what the painted-set test takes (paint_geom reads these nine fields)
    int32_t  kx0, ky0, kx1, ky1;   // the rectangle of the plane that the record paints, in samples: K (Y plane) or Kc (chroma)
    int32_t  psize;          // the plane's own s (PIXELATE: s or sc) or kk (BLUR: kk or kkc); 0 otherwise
    uint32_t sub;            // 1: a chroma plane — sample (u, v) is painted iff any luma pixel (2u + a, 2v + b), a, b in {0, 1}, is
    uint32_t lanes;          // PIXELATE: lanes of a wave that share one cell
    uint32_t unit_first;     // first paint_yuv_apply unit of the record
    uint32_t pre_first;      // first phase-1 unit of the record
    uint32_t ovl_first, ovl_count;   // the LATER records of the same plane whose rectangle meets this one's: indices into the lists
    int32_t  row0;           // plane row that `plane` points at (0 for device frames)
    uint32_t color;          // FILL, OUTLINE: component c takes byte c — Yc | (Uc, Vc) | (Vc, Uc) | Uc | Vc
    uint32_t plane_id;       // PAINT_YUV_PLANE_*
    uint32_t pad;
};
static_assert(sizeof(PaintYuvRec) == 128, "PaintYuvRec is 128 bytes");

// The staged prefix sums of one wave's row segment in paint_yuv_apply: at most 256 / comps + 1 samples of the block plus 2 * 127
// of the halo, times comps: 511 (one component), 766 (two).
constexpr uint32_t PAINT_YUV_PREFIX_MAX = 768;

// Chroma sizes: PIXELATE sc = (s + 1) >> 1, BLUR kkc = max((kk >> 1) | 1, 3); OUTLINE keeps t (the set is decided in luma)
VJ_PAINT_HD inline int32_t paint_yuv_chroma_size(uint32_t mode, int32_t s) {
    if (mode == PAINT_PIXELATE) return (s + 1) >> 1;
    if (mode == PAINT_BLUR) { const int32_t k = (s >> 1) | 1; return k < 3 ? 3 : k; }
    return s;
}

// Sample (x, y) of a record's plane in the region's painted set: P_k on the Y plane, Pc_k — any of the four luma pixels — on chroma
VJ_PAINT_HD inline bool paint_yuv_in_set(const PaintGeom& g, uint32_t sub, int32_t x, int32_t y, uint32_t mode, bool ellipse) {
    if (sub == 0u) return paint_in_set(g, x, y, mode, ellipse);
    return paint_in_set(g, 2 * x, 2 * y, mode, ellipse) || paint_in_set(g, 2 * x + 1, 2 * y, mode, ellipse) ||
           paint_in_set(g, 2 * x, 2 * y + 1, mode, ellipse) || paint_in_set(g, 2 * x + 1, 2 * y + 1, mode, ellipse);
}

// RECTANGLES (no ellipse): the painted set of a plane row is at most two intervals of samples, [a0, a1) and [b0, b1), found once
// per row; a sample is then tested with four 32-bit compares.  Luma row py of K: the whole span [cx0, cx1) — K lies inside M —,
// for OUTLINE minus the inner rectangle's span when py is one of its rows.  The 64-bit arithmetic is here, clamped into K.
struct PaintRowSet { int32_t a0, a1, b0, b1; };
// -> 0: empty, 1: all of [cx0, cx1), 2: split around the inner rectangle (both rows of a chroma row then split alike)
VJ_PAINT_HD inline int paint_yuv_luma_row(const PaintGeom& g, uint32_t mode, int32_t py, PaintRowSet* s) {
    s->a0 = s->a1 = s->b0 = s->b1 = 0;
    if (py < g.cy0 || py >= g.cy1) return 0;
    s->a0 = g.cx0, s->a1 = g.cx1;
    if (mode != PAINT_OUTLINE) return 1;
    const int64_t t = g.size, wi = (int64_t)g.Wm - 2 * t, hi = (int64_t)g.Hm - 2 * t;
    if (wi <= 0 || hi <= 0) return 1;
    const int64_t iy0 = (int64_t)g.Y0 + t, ix0 = (int64_t)g.X0 + t, ix1 = ix0 + wi;
    if (py < iy0 || py >= iy0 + hi) return 1;
    const int64_t lo = g.cx0, hi_x = g.cx1;
    s->a1 = (int32_t)(ix0 < lo ? lo : ix0 > hi_x ? hi_x : ix0);
    s->b0 = (int32_t)(ix1 < lo ? lo : ix1 > hi_x ? hi_x : ix1);
    s->b1 = g.cx1;
    return 2;
}
VJ_PAINT_HD inline PaintRowSet paint_yuv_row_set(const PaintGeom& g, uint32_t sub, uint32_t mode, int32_t row) {
    PaintRowSet s, t;
    if (sub == 0u) {
        (void)paint_yuv_luma_row(g, mode, row, &s);
        return s;
    }
    // the union of luma rows 2 row and 2 row + 1: a whole span wins over a split one, that over an empty one
    const int ks = paint_yuv_luma_row(g, mode, 2 * row, &s), kt = paint_yuv_luma_row(g, mode, 2 * row + 1, &t);
    if (kt == 1 || ks == 0) s = t;
    // luma [a, b), not empty, touches the chroma samples [a >> 1, (b + 1) >> 1)
    if (s.a0 < s.a1) s.a0 >>= 1, s.a1 = (s.a1 + 1) >> 1; else s.a0 = s.a1 = 0;
    if (s.b0 < s.b1) s.b0 >>= 1, s.b1 = (s.b1 + 1) >> 1; else s.b0 = s.b1 = 0;
    return s;
}
VJ_PAINT_HD inline bool paint_yuv_in_row(const PaintRowSet& s, int32_t x) { return (x >= s.a0 && x < s.a1) || (x >= s.b0 && x < s.b1); }

struct PaintYuvArgs {
    const PaintYuvRec* recs;
    const uint32_t* overlaps;     // the overlap lists: indices of records
    uint32_t n_recs;
    uint32_t n_overlaps;
    uint32_t n_units;             // paint_yuv_apply
    uint32_t n_pre_units;         // paint_yuv_colsum / paint_yuv_cells (0: FILL, OUTLINE)
    uint8_t* scratch;
    uint64_t scratch_bytes;
    uint32_t mode;
    uint32_t ellipse;
};
int launch_paint_yuv(const PaintYuvArgs& a, void* stream);

}  // namespace vj
