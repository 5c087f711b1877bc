// Records the painting kernels (vj_paint.hip) share with the host code that builds them (vj_paint_host.cpp, which
// is compiled without HIP for the sanitizer runs): plain PODs and the unit arithmetic both sides use, nothing else.
#pragma once
#include <stdint.h>

namespace vj {

#if defined(__HIP__)
#define VJ_PAINT_HD __host__ __device__
#else
#define VJ_PAINT_HD
#endif

enum : uint32_t { PAINT_FILL = 0, PAINT_OUTLINE = 1, PAINT_PIXELATE = 2, PAINT_BLUR = 3 };

// One region of a slice whose clipped rectangle K is not empty.  The records of a slice are ordered by frame, then by the region's
// index in the call, so "later" in the call is "later" in the records of a frame.
struct PaintRegionDev {
    uint8_t* frame;          // a device address: the caller's device-resident frame, or the frame's rows in the slice's staged block
    uint64_t scratch_off;    // byte offset of the region's phase-1 output in the scratch (a multiple of 16)
    uint32_t stride;         // bytes per frame row
    uint32_t channels;       // 1, 3 or 4
    int32_t  fw, fh;         // the frame's size; the staged block of a host frame holds rows [row0, fh) only from `frame` on
    int32_t  X0, Y0, Wm, Hm; // the mapped rectangle M (it may leave the frame)
    int32_t  cx0, cy0, cx1, cy1;   // K = M ∩ frame, not empty
    int32_t  size;           // t (OUTLINE), s (PIXELATE), kk (BLUR), 0 (FILL)
    uint32_t lanes;          // PIXELATE: lanes of a wave that share one cell (a power of two up to 64)
    uint32_t unit_first;     // first paint_apply unit of the region
    uint32_t pre_first;      // first phase-1 unit (paint_colsum / paint_cells) of the region
    uint32_t ovl_first, ovl_count;   // the LATER regions of its frame whose K meets its own: indices into PaintArgs::overlaps
    int32_t  row0;           // frame row that `frame` points at (0 for device frames; staged host frames begin at their first painted row)
    uint32_t pad;
};
static_assert(sizeof(PaintRegionDev) == 96, "PaintRegionDev is 96 bytes");

// paint_apply, as extract_regions: a work unit is PAINT_BLOCK_H rows of PAINT_BLOCK_SLOTS four-byte slots of the K rows of one
// region; 4 waves, each one row of 64 lanes x 4 bytes at a time.  Slot s of a K row whose first byte lies at address A holds the
// row's bytes [4 s - (A & 3), 4 s - (A & 3) + 4).  A row of B bytes has at most (B + 6) / 4 slots whatever A is.
constexpr uint32_t PAINT_BLOCK_SLOTS = 64, PAINT_BLOCK_H = 32, PAINT_WAVES = 4;
// paint_colsum: a work unit is a band of PAINT_BAND_H rows of PAINT_BAND_COLS byte columns of K (a lane a column).
constexpr uint32_t PAINT_BAND_H = 32, PAINT_BAND_COLS = 256;
// limits (vj.h)
constexpr int32_t PAINT_MAX_SIDE = 32767, PAINT_MAX_KK = 255, PAINT_MAX_CELL = 4096;

VJ_PAINT_HD inline uint32_t paint_row_blocks(uint32_t row_bytes) { return ((row_bytes + 6u) / 4u + PAINT_BLOCK_SLOTS - 1u) / PAINT_BLOCK_SLOTS; }
VJ_PAINT_HD inline uint64_t paint_apply_units(uint32_t row_bytes, uint32_t rows) {
    return (uint64_t)paint_row_blocks(row_bytes) * (uint64_t)((rows + PAINT_BLOCK_H - 1u) / PAINT_BLOCK_H);
}
VJ_PAINT_HD inline uint32_t paint_col_blocks(uint32_t row_bytes) { return (row_bytes + PAINT_BAND_COLS - 1u) / PAINT_BAND_COLS; }
VJ_PAINT_HD inline uint64_t paint_colsum_units(uint32_t row_bytes, uint32_t rows) {
    return (uint64_t)paint_col_blocks(row_bytes) * (uint64_t)((rows + PAINT_BAND_H - 1u) / PAINT_BAND_H);
}
// PIXELATE: the lanes that share a cell of s x s pixels of C channels — the smallest power of two that holds the cell's bytes, at
// most a wave — and the cells a workgroup of PAINT_WAVES waves takes
VJ_PAINT_HD inline uint32_t paint_cell_lanes(uint32_t s, uint32_t C) {
    const uint64_t bytes = (uint64_t)s * s * C;
    uint32_t g = 1;
    while (g < 64u && g < bytes) g *= 2u;
    return g;   // (>= C: at least one lane per channel)
}
VJ_PAINT_HD inline uint32_t paint_cells_per_unit(uint32_t lanes) { return PAINT_WAVES * (64u / lanes); }
VJ_PAINT_HD inline uint32_t paint_cells_x(uint32_t kw, uint32_t s) { return (kw + s - 1u) / s; }
VJ_PAINT_HD inline uint64_t paint_cell_units(uint32_t kw, uint32_t kh, uint32_t s, uint32_t lanes) {
    const uint64_t cells = (uint64_t)paint_cells_x(kw, s) * paint_cells_x(kh, s);
    return (cells + paint_cells_per_unit(lanes) - 1u) / paint_cells_per_unit(lanes);
}
// bytes of a region's phase-1 output, before the rounding to 16: BLUR: kh rows of kw * C 16-bit column sums; PIXELATE: C bytes per cell
VJ_PAINT_HD inline uint64_t paint_scratch_bytes(uint32_t mode, uint32_t kw, uint32_t kh, uint32_t C, uint32_t s) {
    if (mode == PAINT_BLUR) return 2ull * kh * ((uint64_t)kw * C);
    if (mode == PAINT_PIXELATE) return (uint64_t)paint_cells_x(kw, s) * paint_cells_x(kh, s) * C;
    return 0;
}

// (px, py) in the shape of the rectangle (X0, Y0, W, H): the rectangle, or the ellipse inscribed in it.  W, H <= PAINT_MAX_SIDE:
// inside the rectangle |2 dx + 1 - W| <= W, so both products stay below 2^60.
VJ_PAINT_HD inline bool paint_in_shape(int32_t px, int32_t py, int64_t X0, int64_t Y0, int64_t W, int64_t H, bool ellipse) {
    const int64_t dx = (int64_t)px - X0, dy = (int64_t)py - Y0;
    if (dx < 0 || dy < 0 || dx >= W || dy >= H) return false;
    if (!ellipse) return true;
    const int64_t a = 2 * dx + 1 - W, b = 2 * dy + 1 - H, W2 = W * W, H2 = H * H;
    return a * a * H2 + b * b * W2 <= W2 * H2;
}
// The geometry of a region record (read field by field: the kernels hold the records in the constant address space)
struct PaintGeom { int32_t X0, Y0, Wm, Hm, cx0, cy0, cx1, cy1, size; };
template <typename P>
VJ_PAINT_HD inline PaintGeom paint_geom(P r) {
    PaintGeom g;
    g.X0 = r->X0, g.Y0 = r->Y0, g.Wm = r->Wm, g.Hm = r->Hm;
    g.cx0 = r->cx0, g.cy0 = r->cy0, g.cx1 = r->cx1, g.cy1 = r->cy1;
    g.size = r->size;
    return g;
}
// (px, py) in the painted set of the region: K ∩ shape, for OUTLINE minus the shape of M shrunk by t on each side
VJ_PAINT_HD inline bool paint_in_set(const PaintGeom& g, int32_t px, int32_t py, uint32_t mode, bool ellipse) {
    if (px < g.cx0 || px >= g.cx1 || py < g.cy0 || py >= g.cy1) return false;
    if (!paint_in_shape(px, py, g.X0, g.Y0, g.Wm, g.Hm, ellipse)) return false;
    if (mode != PAINT_OUTLINE) return true;
    const int64_t t = g.size, wi = (int64_t)g.Wm - 2 * t, hi = (int64_t)g.Hm - 2 * t;
    if (wi <= 0 || hi <= 0) return true;
    return !paint_in_shape(px, py, (int64_t)g.X0 + t, (int64_t)g.Y0 + t, wi, hi, ellipse);
}

struct PaintArgs {
    const PaintRegionDev* regions;
    const uint32_t* overlaps;     // the overlap lists: indices of records
    uint32_t n_regions;
    uint32_t n_overlaps;
    uint32_t n_units;             // paint_apply
    uint32_t n_pre_units;         // paint_colsum / paint_cells (0: FILL, OUTLINE)
    uint8_t* scratch;
    uint64_t scratch_bytes;
    uint32_t mode;
    uint32_t ellipse;
    uint32_t color;               // color[0..3] packed, byte c = channel c
    uint32_t pad;
};
int launch_paint(const PaintArgs& a, void* stream);

}  // namespace vj
