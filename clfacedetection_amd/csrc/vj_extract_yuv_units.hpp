// Records the kernels of vj_extract_yuv / vj_extract_affine_yuv (vj_extract_yuv.hip) share with the host code that
// builds them (vj_extract_yuv_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs, nothing else.  A record is
// vj_extract's (or vj_extract_affine's) with the frame's three planes in place of its one image; the work units and the taps are
// vj_extract's (vj_extract_units.hpp).
#pragma once
#include <stdint.h>

#include "vj_affine_units.hpp"
#include "vj_yuv_units.hpp"

namespace vj {

// The planes of the 4:2:0 frame a region is cut from.  Device addresses: the caller's device-resident planes, or the planes' places in
// the uploaded block of the slice's host frames.  c0: the pair plane (NV12 / NV21) or the U plane; c1: the V plane, I420 only.
struct YuvPlanesDev {
    const uint8_t* y;
    const uint8_t* c0;
    const uint8_t* c1;
    uint32_t y_stride, c_stride;   // bytes per row of the Y plane / of a chroma plane
    int32_t  fw, fh;               // the frame's size in luma pixels: even
    uint32_t layout;               // YUV_NV12 / YUV_NV21 / YUV_I420
    uint32_t unit_first;           // first work unit of the region
};
static_assert(sizeof(YuvPlanesDev) == 48, "YuvPlanesDev is 48 bytes");

// One region of a vj_extract_yuv call: ExtractRegionDev's crop, taps and mode, in luma pixels
struct ExtractYuvRegionDev {
    YuvPlanesDev f;
    uint64_t dst_off;       // byte offset of the region's output in the destination buffer
    int32_t  x0, y0;        // the crop's origin in the frame (margin included; may be negative)
    uint32_t cw, ch;        // the crop's size
    uint32_t xtab, ytab;    // first PyrTap of its columns / rows (EXTRACT_COPY and EXTRACT_AREA read none)
    uint32_t mode;          // EXTRACT_BILINEAR, EXTRACT_AREA, EXTRACT_COPY
    uint32_t reserved[3];
};
static_assert(sizeof(ExtractYuvRegionDev) == 96, "ExtractYuvRegionDev is 96 bytes");

// One region of a vj_extract_affine_yuv call: AffineRegionDev's matrix
struct AffineYuvRegionDev {
    YuvPlanesDev f;
    uint64_t dst_off;
    uint64_t reserved;
    double   m[6];         // src_x = m0 x + m1 y + m2, src_y = m3 x + m4 y + m5, in luma pixels
};
static_assert(sizeof(AffineYuvRegionDev) == 112, "AffineYuvRegionDev is 112 bytes");

struct ExtractYuvArgs {
    const void* regions;    // ExtractYuvRegionDev (extract_yuv_regions) or AffineYuvRegionDev (affine_yuv_regions)
    uint32_t n_regions;
    uint32_t n_units;
    const PyrTap* taps;     // extract_yuv_regions only
    uint8_t* dst;           // the caller's buffer; every region's output lies inside [dst, dst + dst_bytes)
    uint64_t dst_bytes;
    uint32_t out_w, out_h;
    uint32_t C;             // channels of the output: 1 (gray), 3 or 4
    uint32_t gray;          // != 0: every decoded tap goes through BGR2GRAY, then the blend (C = 1)
    uint32_t planar;        // != 0: n x C x out_h x out_w
    uint32_t swap_rb;       // VJ_YUV_RGB_ORDER: the decoded taps are R, G, B
    uint32_t rows, row_bytes;
};
int launch_extract_yuv(const ExtractYuvArgs& a, void* stream);
int launch_affine_yuv(const ExtractYuvArgs& a, void* stream);

}  // namespace vj
