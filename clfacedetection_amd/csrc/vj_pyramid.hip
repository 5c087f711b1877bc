// gfx950 kernel of CV_HAAR_SCALE_IMAGE's image pyramid (VJ_FLAG_CV_SCALE_IMAGE, tempcv.cpp:1257-1329): cvResize(img, &img1,
// CV_INTER_LINEAR) of the 8-bit gray frame to every level's size (:1301), all levels of all frames of a sub-batch in ONE launch —
// the late levels are a few hundred pixels each, a launch per level would make the call launch-bound.  The arithmetic is OpenCV
// 2.4.2 imgproc's 8-bit path as DESIGN.md §4.8 states it (third-party, parity unpinned): integer only,
//   horizontal  h(row, dx) = S[row][i0] * c0 + S[row][i1] * c1                    (11-bit weights, 2048 = 1.0)
//   vertical    dst = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
// and the 2 x 2 mean (sum + 2) >> 2 where the source is exactly twice the level.  The taps (source indices and weights of every
// destination column and row) come from the host, built once per plan (vj_cv.cpp: build_taps): the kernel does no float arithmetic.
// BGR / BGRA frames go through the ingest conversion (bgr2gray) tap by tap: the gray image is never written.
//
// One thread per destination pixel, a workgroup per PYR_UNIT_PX pixels of one level row; blockIdx.x is the unit within the frame
// (the level comes from a binary search of the level table's unit prefix: uniform, scalar loads), blockIdx.y the frame.  The
// kernel is bound by its byte stores and the four taps' loads, which neighbouring lanes share.
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"

namespace vj {

__device__ __forceinline__ int32_t pyr_px(const uint8_t* row, uint32_t x, uint32_t ch) {
    if (ch <= 1u) return (int32_t)row[x];
    const uint8_t* p = row + (size_t)x * ch;
    return (int32_t)bgr2gray(p[0], p[1], p[2]);
}

__global__ __launch_bounds__(PYR_UNIT_PX) void pyramid_levels(PyrArgs a) {
    kptr<PyrLevelDev> levels = as_k(a.levels);
    const uint32_t unit = blockIdx.x;
    uint32_t lo = 0, hi = a.n_levels;   // the last level whose first unit is <= unit
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (levels[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    const uint32_t lw = levels[lo].w, lh = levels[lo].h, ox = levels[lo].ox, oy = levels[lo].oy;
    const uint32_t units_per_row = (lw + PYR_UNIT_PX - 1u) / PYR_UNIT_PX;
    const uint32_t u = unit - levels[lo].unit_first;
    const uint32_t dy = u / units_per_row, dx = (u - dy * units_per_row) * PYR_UNIT_PX + threadIdx.x;
    // inside the level, and the level inside the canvas (the host lays it out so; a store never leaves the canvas)
    if (dy >= lh || dx >= lw || ox + dx >= a.canvas_w || oy + dy >= a.canvas_h) return;
    // (a PyrTap as two dwords: i0 | i1 << 16, c0 | c1 << 16; the row's tap is uniform: scalar loads)
    const uint2 wx = reinterpret_cast<const uint2*>(a.taps)[levels[lo].xtab + dx];
    kptr<uint32_t> taps_k = as_k(reinterpret_cast<const uint32_t*>(a.taps));
    const uint2 wy = make_uint2(taps_k[2u * (levels[lo].ytab + dy)], taps_k[2u * (levels[lo].ytab + dy) + 1u]);
    struct Tap { uint32_t i0, i1; int32_t c0, c1; };
    const Tap tx{wx.x & 0xffffu, wx.x >> 16, (int32_t)(int16_t)(wx.y & 0xffffu), (int32_t)(int16_t)(wx.y >> 16)};
    const Tap ty{wy.x & 0xffffu, wy.x >> 16, (int32_t)(int16_t)(wy.y & 0xffffu), (int32_t)(int16_t)(wy.y >> 16)};
    const uint32_t x0 = min(tx.i0, a.width - 1u), x1 = min(tx.i1, a.width - 1u);
    const uint32_t y0 = min(ty.i0, a.height - 1u), y1 = min(ty.i1, a.height - 1u);
    const bool area = levels[lo].area != 0u;
    for (uint32_t frame = blockIdx.y; frame < a.n_frames; frame += gridDim.y) {
        const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
        const uint8_t* r0 = img + (size_t)y0 * a.gray_stride;
        const uint8_t* r1 = img + (size_t)y1 * a.gray_stride;
        const int32_t s00 = pyr_px(r0, x0, a.channels), s01 = pyr_px(r0, x1, a.channels);
        const int32_t s10 = pyr_px(r1, x0, a.channels), s11 = pyr_px(r1, x1, a.channels);
        int32_t v;
        if (area) {
            v = (s00 + s01 + s10 + s11 + 2) >> 2;
        } else {
            const int32_t h0 = s00 * tx.c0 + s01 * tx.c1, h1 = s10 * tx.c0 + s11 * tx.c1;
            v = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
        a.canvas[(size_t)frame * a.canvas_frame_bytes + (size_t)(oy + dy) * a.canvas_pitch + ox + dx] = (uint8_t)v;
    }
}

int launch_pyramid(const PyrArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    dim3 g(a.n_units, std::min<uint32_t>(a.n_frames, 65535u)), b(PYR_UNIT_PX);
    hipLaunchKernelGGL(pyramid_levels, g, b, 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

// CV_HAAR_SCALE_IMAGE inside regions (vj_detect_opencv_rois, route 2): a resized crop is not a crop of the resized
// frame, so every region has level images of its own — all of them, for all regions of a canvas, in ONE launch.  The arithmetic is
// pyramid_levels'.  A level image names its frame and its crop; its taps index the CROP (they depend on the crop's and the level's
// lengths only, so level images share them): the kernel adds the crop's origin and clamps to the crop's last column and row — the
// frame's own would let a border tap read the neighbour pixel outside the region.
// A workgroup is a PYR_REGION_TW x PYR_REGION_TH block of one level image (they are mostly smaller than one row of pyramid_levels'
// units), a thread four destination pixels of a row: one dword store where all four lie inside the level image (its origin, the
// block and the pitch are multiples of 4), byte stores at its right edge.
__global__ __launch_bounds__(256) void pyramid_regions(PyrRegionArgs a) {
    kptr<PyrRegionLevelDev> levels = as_k(a.levels);
    const uint32_t unit = blockIdx.x;
    uint32_t lo = 0, hi = a.n_levels;   // the last level image whose first unit is <= unit
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (levels[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    const uint32_t lw = levels[lo].w, lh = levels[lo].h, ox = levels[lo].ox, oy = levels[lo].oy;
    const uint32_t cx = levels[lo].cx, cy = levels[lo].cy, cw = levels[lo].cw, chh = levels[lo].ch, frame = levels[lo].frame;
    const uint32_t blocks_per_row = (lw + PYR_REGION_TW - 1u) / PYR_REGION_TW;
    const uint32_t u = unit - levels[lo].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * PYR_REGION_TW + (threadIdx.x & 15u) * 4u, dy = by * PYR_REGION_TH + (threadIdx.x >> 4);
    // inside the level image, the level image inside the canvas, the crop inside its frame (the host lays them out and checks them
    // so; neither a store nor a load leaves its buffer)
    if (dy >= lh || dx >= lw || oy + dy >= a.canvas_h || ox + dx >= a.canvas_w) return;
    if (frame >= a.n_frames || cw == 0u || chh == 0u || cx + cw > a.width || cy + chh > a.height) return;
    struct Tap { uint32_t i0, i1; int32_t c0, c1; };
    auto tap_of = [&](uint32_t i) {
        const uint2 w = reinterpret_cast<const uint2*>(a.taps)[i];
        return Tap{w.x & 0xffffu, w.x >> 16, (int32_t)(int16_t)(w.y & 0xffffu), (int32_t)(int16_t)(w.y >> 16)};
    };
    const Tap ty = tap_of(levels[lo].ytab + dy);
    const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
    const uint8_t* r0 = img + (size_t)(cy + min(ty.i0, chh - 1u)) * a.gray_stride;
    const uint8_t* r1 = img + (size_t)(cy + min(ty.i1, chh - 1u)) * a.gray_stride;
    const bool area = levels[lo].area != 0u;
    const uint32_t n = min(4u, lw - dx);
    uint32_t packed = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const Tap tx = tap_of(levels[lo].xtab + min(dx + k, lw - 1u));   // (past the right edge: the last column again, not stored)
        const uint32_t x0 = cx + min(tx.i0, cw - 1u), x1 = cx + min(tx.i1, cw - 1u);
        const int32_t s00 = pyr_px(r0, x0, a.channels), s01 = pyr_px(r0, x1, a.channels);
        const int32_t s10 = pyr_px(r1, x0, a.channels), s11 = pyr_px(r1, x1, a.channels);
        int32_t v;
        if (area) {
            v = (s00 + s01 + s10 + s11 + 2) >> 2;
        } else {
            const int32_t h0 = s00 * tx.c0 + s01 * tx.c1, h1 = s10 * tx.c0 + s11 * tx.c1;
            v = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
        }
        packed |= ((uint32_t)v & 0xffu) << (8u * k);
    }
    uint8_t* dst = a.canvas + (size_t)(oy + dy) * a.canvas_pitch + ox + dx;
    if (n == 4u && ox + dx + 4u <= a.canvas_w && ((ox | a.canvas_pitch) & 3u) == 0u) {
        *reinterpret_cast<uint32_t*>(dst) = packed;
    } else {
        for (uint32_t k = 0; k < n; ++k)
            if (ox + dx + k < a.canvas_w) dst[k] = (uint8_t)(packed >> (8u * k));
    }
}

int launch_pyramid_regions(const PyrRegionArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_levels == 0u) return 0;
    dim3 g(a.n_units), b(256);
    hipLaunchKernelGGL(pyramid_regions, g, b, 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
