// Records the affine kernel (vj_affine.hip) shares with the host code that builds them (vj_affine_host.cpp, which
// is compiled without HIP for the sanitizer runs): plain PODs, nothing else.  The work units are vj_extract's (vj_extract_units.hpp):
// a region's output is `rows` dense rows of `row_bytes` bytes, a unit EXTRACT_BLOCK_H rows of EXTRACT_BLOCK_SLOTS four-byte slots.
#pragma once
#include <stdint.h>

#include "vj_extract_units.hpp"

namespace vj {

// One region of a vj_extract_affine call: the frame it samples (a device address: the caller's device-resident frame, or the
// frame's place in the uploaded block of the slice's host frames), the matrix from output pixels to source pixels, and where its
// output goes.  Row and column terms of the fixed-point positions are computed on the device from m (no table travels).
struct AffineRegionDev {
    const uint8_t* src;
    uint64_t dst_off;       // byte offset of the region's output in the destination buffer: region index * rows * row_bytes
    uint32_t stride;        // bytes per source row
    uint32_t channels;      // of the source: 1, 3 (BGR) or 4 (BGRA)
    int32_t  fw, fh;        // the frame's size
    uint32_t unit_first;    // first work unit of the region
    uint32_t reserved[3];
    double   m[6];         // src_x = m0 x + m1 y + m2, src_y = m3 x + m4 y + m5
};
static_assert(sizeof(AffineRegionDev) == 96, "AffineRegionDev is 96 bytes");

constexpr double AFFINE_COORD_MAX = 524288.0;   // 2^19: the bound on |m0| (out_w - 1), |m3| (out_w - 1), |m1 y + m2|, |m4 y + m5|

struct AffineArgs {
    const AffineRegionDev* regions;
    uint32_t n_regions;
    uint32_t n_units;
    uint8_t* dst;           // the caller's buffer; every region's output lies inside [dst, dst + dst_bytes)
    uint64_t dst_bytes;
    uint32_t out_w, out_h;
    uint32_t C;             // channels of the output: 1, 3 or 4
    uint32_t gray;          // != 0: colour sources go through BGR2GRAY tap by tap (C = 1)
    uint32_t planar;        // != 0: n x C x out_h x out_w
    uint32_t rows, row_bytes;
};
int launch_affine(const AffineArgs& a, void* stream);

}  // namespace vj
