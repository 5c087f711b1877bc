// Records the extraction kernel (vj_extract.hip) shares with the host code that builds them (vj_extract_host.cpp,
// which is compiled without HIP for the sanitizer runs): plain PODs, nothing else.
#pragma once
#include <stdint.h>

#include "vj_cv_roi_units.hpp"

namespace vj {

// One region of a vj_extract call: the frame it is cut from (a device address: the caller's device-resident frame, or the frame's
// place in the uploaded block of the slice's host frames), its crop — which may lie partly or wholly outside the frame: source
// indices are clamped to the frame — and where its output goes.  The taps index the CROP: tap + origin, then the clamp.
struct ExtractRegionDev {
    const uint8_t* src;
    uint64_t dst_off;       // byte offset of the region's output in the destination buffer: region index * rows * row_bytes
    uint32_t stride;        // bytes per source row
    uint32_t channels;      // of the source: 1, 3 (BGR) or 4 (BGRA)
    int32_t  fw, fh;        // the frame's size
    int32_t  x0, y0;        // the crop's origin in the frame (margin included; may be negative)
    uint32_t cw, ch;        // the crop's size
    uint32_t xtab, ytab;    // first PyrTap of its columns / rows in ExtractArgs::taps (EXTRACT_COPY reads none)
    uint32_t mode;          // EXTRACT_BILINEAR, EXTRACT_AREA (the crop is exactly 2 out_w x 2 out_h) or EXTRACT_COPY (the crop has the output's size)
    uint32_t unit_first;    // first work unit of the region
};
static_assert(sizeof(ExtractRegionDev) == 64, "ExtractRegionDev is 64 bytes");
enum : uint32_t { EXTRACT_BILINEAR = 0, EXTRACT_AREA = 1, EXTRACT_COPY = 2 };

// A region's output is `rows` dense rows of `row_bytes` bytes: out_h rows of out_w * C interleaved, C * out_h rows of out_w planar.
// A work unit is EXTRACT_BLOCK_H rows of EXTRACT_BLOCK_SLOTS four-byte slots: 4 waves, each one row of 64 lanes x 4 bytes at a time.
// Slot s of a row whose first byte lies at address A holds the row's bytes [4 s - (A & 3), 4 s - (A & 3) + 4): every slot that lies
// wholly inside the row is an aligned dword.  A row of B bytes has at most (B + 3 + 3) / 4 slots, whatever A is: the unit count
// does not depend on the destination's address.
constexpr uint32_t EXTRACT_BLOCK_SLOTS = 64, EXTRACT_BLOCK_H = 16;
inline uint32_t extract_row_blocks(uint32_t row_bytes) { return ((row_bytes + 6u) / 4u + EXTRACT_BLOCK_SLOTS - 1u) / EXTRACT_BLOCK_SLOTS; }
inline uint64_t extract_units(uint32_t row_bytes, uint32_t rows) {
    return (uint64_t)extract_row_blocks(row_bytes) * (uint64_t)((rows + EXTRACT_BLOCK_H - 1u) / EXTRACT_BLOCK_H);
}

struct ExtractArgs {
    const ExtractRegionDev* regions;
    uint32_t n_regions;
    uint32_t n_units;
    const PyrTap* taps;
    uint8_t* dst;           // the caller's buffer; every region's output lies inside [dst, dst + dst_bytes)
    uint64_t dst_bytes;
    uint32_t out_w, out_h;
    uint32_t C;             // channels of the output: 1, 3 or 4
    uint32_t gray;          // != 0: colour sources go through BGR2GRAY tap by tap (C = 1)
    uint32_t planar;        // != 0: n x C x out_h x out_w
    uint32_t rows, row_bytes;
};
int launch_extract(const ExtractArgs& a, void* stream);

}  // namespace vj
