// Records the colour-conversion kernels (vj_yuv.hip) share with the host code that builds them (vj_yuv_host.cpp,
// which is compiled without HIP for the sanitizer runs): plain PODs and the geometry both sides derive from them, nothing else.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VJ_YUV_HD __host__ __device__
#else
#define VJ_YUV_HD
#endif

namespace vj {

enum : uint32_t { YUV_NV12 = 0, YUV_NV21 = 1, YUV_I420 = 2 };   // = VJ_YUV_NV12 / _NV21 / _I420

// One frame of a vj_yuv_to_bgr or vj_bgr_to_yuv call.  Device addresses: the caller's device-resident planes, or the frame's place in
// the uploaded block of the call's host frames.
//   decode  y, c0, c1: the source planes (c1: I420 only), rows y_stride / c_stride bytes apart; dst_off: the BGR image in the
//           caller's buffer, rows `pitch` = align4(width * channels) bytes apart
//   encode  y: the BGR / BGRA source, rows y_stride bytes apart, `channels` bytes per pixel; dst_off: the stacked output frame, whose
//           planes follow from width, height and the layout (yuv_plane_pitch, yuv_plane_off); pitch = align4(width)
// dst_off is a multiple of 256 and every pitch a multiple of 4: every plane and every row of the output is 4-byte aligned.
struct YuvFrameDev {
    const uint8_t* y;
    const uint8_t* c0;
    const uint8_t* c1;
    uint64_t dst_off;
    uint32_t y_stride, c_stride;
    uint32_t width, height;   // even, 2 .. 65534
    uint32_t pitch;
    uint32_t channels;        // encode: of this source (3 or 4); decode: the call's
    uint32_t unit_first;      // first work unit (a YUV_BLOCK_W x YUV_BLOCK_H block of the frame's pixels)
    uint32_t layout;          // YUV_NV12 / YUV_NV21 / YUV_I420: decode: of this source; encode: the call's
};
static_assert(sizeof(YuvFrameDev) == 64, "YuvFrameDev is 64 bytes");

// Pixels per lane and per workgroup: a lane owns YUV_LANE_W x 2 pixels (two aligned dwords of Y, one of NV12 chroma), a wave one row
// pair of 64 lanes at a time, the 4 waves of a workgroup row pairs k, k + 4, ... of the block.
constexpr uint32_t YUV_LANE_W = 4, YUV_WAVES = 4;
constexpr uint32_t YUV_BLOCK_W = 64u * YUV_LANE_W, YUV_BLOCK_H = 32;
VJ_YUV_HD inline uint64_t yuv_units(uint32_t w, uint32_t h) {
    return (uint64_t)((w + YUV_BLOCK_W - 1u) / YUV_BLOCK_W) * (uint64_t)((h + YUV_BLOCK_H - 1u) / YUV_BLOCK_H);
}

VJ_YUV_HD inline uint32_t yuv_align4(uint32_t v) { return (v + 3u) & ~3u; }
// Row bytes of a chroma plane: w for the pair plane, w / 2 for I420's
VJ_YUV_HD inline uint32_t yuv_chroma_row_bytes(uint32_t layout, uint32_t w) { return layout == YUV_I420 ? w / 2u : w; }
// The stacked output frame of the encoder: plane 0 = Y, 1 = pairs or U, 2 = V (I420 only)
VJ_YUV_HD inline uint32_t yuv_plane_pitch(uint32_t layout, uint32_t w, uint32_t plane) {
    return yuv_align4(plane == 0u ? w : yuv_chroma_row_bytes(layout, w));
}
VJ_YUV_HD inline uint64_t yuv_plane_off(uint32_t layout, uint32_t w, uint32_t h, uint32_t plane) {
    uint64_t off = 0;
    if (plane >= 1u) off += (uint64_t)yuv_plane_pitch(layout, w, 0u) * h;
    if (plane >= 2u) off += (uint64_t)yuv_plane_pitch(layout, w, 1u) * (h / 2u);
    return off;
}
VJ_YUV_HD inline uint64_t yuv_frame_bytes(uint32_t layout, uint32_t w, uint32_t h) {
    return yuv_plane_off(layout, w, h, 2u) + (layout == YUV_I420 ? (uint64_t)yuv_plane_pitch(layout, w, 2u) * (h / 2u) : 0u);
}

struct YuvArgs {
    const YuvFrameDev* frames;
    uint32_t n_frames;
    uint32_t n_units;
    uint8_t* dst;             // the caller's buffer; every frame's output lies inside [dst, dst + dst_bytes)
    uint64_t dst_bytes;
    uint32_t layout;          // YUV_NV12 / YUV_NV21 / YUV_I420
    uint32_t channels;        // decode: 3 or 4
    uint32_t swap_rb;         // VJ_YUV_RGB_ORDER
};
int launch_yuv_to_bgr(const YuvArgs& a, void* stream);
int launch_bgr_to_yuv(const YuvArgs& a, void* stream);

}  // namespace vj
