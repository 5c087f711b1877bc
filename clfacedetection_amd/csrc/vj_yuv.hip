// gfx950 kernels of vj_yuv_to_bgr / vj_bgr_to_yuv: a decoder's 4:2:0 frames (NV12, NV21, I420) to interleaved
// BGR / BGRA and back, OpenCV's 8-bit fixed-point BT.601 limited-range arithmetic, integers only (the definition: include/vj.h).
//   yuv_to_bgr<LAYOUT, CH>   nearest chroma; CH = 4: alpha 255
//   bgr_to_yuv<LAYOUT, CH>   Y of every pixel, U and V of the top-left pixel of each 2 x 2 block
// Both are pure streaming: what counts is bytes per instruction.  A workgroup is a YUV_BLOCK_W x YUV_BLOCK_H block of one frame (the
// frame from a binary search of the records' unit prefix: uniform, scalar loads — as prep_resize finds its frame), a wave one ROW PAIR
// of it at a time, a lane 4 x 2 pixels: two dwords of Y and one of NV12 chroma (two bytes of each I420 plane) against 3-dword (BGR) or
// 4-dword (BGRA) accesses per row on the other side, the wave's accesses covering consecutive bytes of a row.  Widths are even, so a
// lane holds 4 or 2 pixels; the 2-pixel lane at the end of a row whose width is not a multiple of 4 writes its row's pad bytes (as 0)
// in the same dwords.  Every output row is 4-byte aligned by layout.  A source row is read with dwords where its address is a
// multiple of 4 and byte by byte elsewhere: never an unaligned dword.
#include <hip/hip_runtime.h>
#include "vj_yuv_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {

// multi-dword accesses of rows that are 4-byte, not 16-byte, aligned (the caller's buffer is a multiple of 4)
typedef uint32_t yuv_u32x2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t yuv_u32x3 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t yuv_u32x4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int32_t YUV_HALF = 1 << 19;

// the last frame whose first unit is <= unit; uniform, scalar loads
__device__ __forceinline__ uint32_t yuv_frame_of(kptr<YuvFrameDev> frames, uint32_t n_frames, uint32_t unit) {
    uint32_t lo = 0, hi = n_frames;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (frames[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

// bytes p[0 .. n) packed little-endian, n = 2 or 4 (bytes beyond n: 0): one dword where all four are there and p is aligned
__device__ __forceinline__ uint32_t yuv_load4(const uint8_t* p, uint32_t n) {
    if (n == 4u && ((uintptr_t)p & 3u) == 0u) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8;
    if (n == 4u) v |= (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return v;
}

__device__ __forceinline__ uint32_t yuv_sat(int32_t t) { return (uint32_t)min(max(t, 0), 255); }

struct YuvChroma { int32_t b, g, r; };   // the terms two pixels of a row, and the two below them, share
__device__ __forceinline__ YuvChroma yuv_chroma(uint32_t U, uint32_t V) {
    const int32_t u = (int32_t)U - 128, v = (int32_t)V - 128;
    return YuvChroma{YUV_HALF + 2116026 * u, YUV_HALF - 852492 * v - 409993 * u, YUV_HALF + 1673527 * v};
}
// B | G << 8 | R << 16 | 255 << 24 (swap: R and B exchanged)
__device__ __forceinline__ uint32_t yuv_decode_px(uint32_t Y, const YuvChroma& c, bool swap) {
    const int32_t yy = max((int32_t)Y - 16, 0) * 1220542;
    const uint32_t b = yuv_sat((yy + c.b) >> 20), g = yuv_sat((yy + c.g) >> 20), r = yuv_sat((yy + c.r) >> 20);
    return (swap ? r : b) | g << 8 | (swap ? b : r) << 16 | 0xff000000u;
}

// the first n (2 or 4) of four decoded pixels to dst, a 4-byte aligned place in the row; CH = 3, n = 2: and the row's two pad bytes
template <uint32_t CH>
__device__ __forceinline__ void yuv_store_bgr(uint8_t* dst, const uint32_t p[4], uint32_t n) {
    if (CH == 4u) {
        if (n == 4u) *reinterpret_cast<yuv_u32x4*>(dst) = yuv_u32x4{p[0], p[1], p[2], p[3]};
        else *reinterpret_cast<yuv_u32x2*>(dst) = yuv_u32x2{p[0], p[1]};
    } else {   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
        const uint32_t q0 = p[0] & 0xffffffu, q1 = p[1] & 0xffffffu, q2 = p[2] & 0xffffffu, q3 = p[3] & 0xffffffu;
        if (n == 4u) *reinterpret_cast<yuv_u32x3*>(dst) = yuv_u32x3{q0 | q1 << 24, q1 >> 8 | q2 << 16, q2 >> 16 | q3 << 8};
        else *reinterpret_cast<yuv_u32x2*>(dst) = yuv_u32x2{q0 | q1 << 24, q1 >> 8};
    }
}

// n (2 or 4) pixels of a BGR / BGRA row at p as B | G << 8 | R << 16 (bits 24 .. 31: anything); pixels beyond n: 0
template <uint32_t CH>
__device__ __forceinline__ void yuv_load_bgr(const uint8_t* p, uint32_t n, uint32_t px[4]) {
    const bool aligned = ((uintptr_t)p & 3u) == 0u;
    px[2] = px[3] = 0u;
    if (CH == 4u) {
        if (aligned && n == 4u) {
            const yuv_u32x4 w = *reinterpret_cast<const yuv_u32x4*>(p);
            px[0] = w.x, px[1] = w.y, px[2] = w.z, px[3] = w.w;
        } else if (aligned) {
            const yuv_u32x2 w = *reinterpret_cast<const yuv_u32x2*>(p);
            px[0] = w.x, px[1] = w.y;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < n) px[k] = (uint32_t)p[4u * k] | (uint32_t)p[4u * k + 1u] << 8 | (uint32_t)p[4u * k + 2u] << 16;
        }
    } else {
        if (aligned && n == 4u) {   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            const yuv_u32x3 w = *reinterpret_cast<const yuv_u32x3*>(p);
            px[0] = w.x, px[1] = w.x >> 24 | w.y << 8, px[2] = w.y >> 16 | w.z << 16, px[3] = w.z >> 8;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k)
                if (k < n) px[k] = (uint32_t)p[3u * k] | (uint32_t)p[3u * k + 1u] << 8 | (uint32_t)p[3u * k + 2u] << 16;
        }
    }
}

__device__ __forceinline__ uint32_t yuv_luma(uint32_t px, bool swap) {
    const int32_t c0 = (int32_t)(px & 0xffu), g = (int32_t)((px >> 8) & 0xffu), c2 = (int32_t)((px >> 16) & 0xffu);
    const int32_t b = swap ? c2 : c0, r = swap ? c0 : c2;
    return (uint32_t)((269484 * r + 528482 * g + 102760 * b + YUV_HALF + (16 << 20)) >> 20);
}
// U | V << 8
__device__ __forceinline__ uint32_t yuv_uv(uint32_t px, bool swap) {
    const int32_t c0 = (int32_t)(px & 0xffu), g = (int32_t)((px >> 8) & 0xffu), c2 = (int32_t)((px >> 16) & 0xffu);
    const int32_t b = swap ? c2 : c0, r = swap ? c0 : c2;
    const int32_t u = (-155188 * r - 305135 * g + 460324 * b + YUV_HALF + (128 << 20)) >> 20;
    const int32_t v = (460324 * r - 385875 * g - 74448 * b + YUV_HALF + (128 << 20)) >> 20;
    return ((uint32_t)u & 0xffu) | ((uint32_t)v & 0xffu) << 8;
}

}  // namespace

// A launch converts the frames of the slice that have layout LAYOUT and skips the others (uniform).  Every load lies inside the
// frame's planes: columns x .. x + n - 1 < width of rows y, y + 1 < height, chroma bytes below the
// plane's row bytes of row y / 2.  Every store lies inside the frame's image and that inside the buffer (checked): x < width, so
// (x + n) * CH <= pitch, and the 2-pixel BGR lane ends exactly at the pitch.
template <uint32_t LAYOUT, uint32_t CH>
__global__ __launch_bounds__(256) void yuv_to_bgr(YuvArgs a) {
    kptr<YuvFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    if (unit >= a.n_units || a.n_frames == 0u) return;
    const uint32_t f = yuv_frame_of(frames, a.n_frames, unit);
    if (frames[f].layout != LAYOUT) return;
    const uint32_t w = frames[f].width, h = frames[f].height, pitch = frames[f].pitch;
    const uint64_t off = frames[f].dst_off;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blocks_per_row = (w + YUV_BLOCK_W - 1u) / YUV_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t x = bx * YUV_BLOCK_W + lane * YUV_LANE_W;
    const uint32_t y1 = min((by + 1u) * YUV_BLOCK_H, h);
    // the image inside the buffer (the host lays it out so; a store never leaves the buffer)
    const bool inside = ((w | h) & 1u) == 0u && (pitch & 3u) == 0u && (off & 3u) == 0u && pitch >= w * CH && off + (uint64_t)pitch * h <= a.dst_bytes;
    if (!inside || x >= w) return;
    const uint32_t n = min(YUV_LANE_W, w - x);   // 4, or 2 at the end of a row
    const size_t ys = frames[f].y_stride, cs = frames[f].c_stride;
    const uint8_t* py = frames[f].y + x;
    const uint8_t* pc0 = frames[f].c0 + (LAYOUT == YUV_I420 ? x >> 1 : x);
    const uint8_t* pc1 = LAYOUT == YUV_I420 ? frames[f].c1 + (x >> 1) : nullptr;
    uint8_t* dst = a.dst + off + (size_t)x * CH;
    const bool swap = a.swap_rb != 0u;
    for (uint32_t y = by * YUV_BLOCK_H + 2u * wave; y < y1; y += 2u * YUV_WAVES) {   // (y is even and so is h: row y + 1 exists)
        const uint32_t ya = yuv_load4(py + (size_t)y * ys, n), yb = yuv_load4(py + (size_t)(y + 1u) * ys, n);
        uint32_t u0, v0, u1 = 128u, v1 = 128u;
        if (LAYOUT == YUV_I420) {
            const uint8_t* ru = pc0 + (size_t)(y >> 1) * cs;
            const uint8_t* rv = pc1 + (size_t)(y >> 1) * cs;
            u0 = ru[0], v0 = rv[0];
            if (n == 4u) u1 = ru[1], v1 = rv[1];
        } else {
            const uint32_t c = yuv_load4(pc0 + (size_t)(y >> 1) * cs, n);
            const uint32_t e0 = c & 0xffu, o0 = (c >> 8) & 0xffu, e1 = (c >> 16) & 0xffu, o1 = c >> 24;
            u0 = LAYOUT == YUV_NV12 ? e0 : o0, v0 = LAYOUT == YUV_NV12 ? o0 : e0;
            if (n == 4u) u1 = LAYOUT == YUV_NV12 ? e1 : o1, v1 = LAYOUT == YUV_NV12 ? o1 : e1;
        }
        const YuvChroma ca = yuv_chroma(u0, v0), cb = yuv_chroma(u1, v1);
        uint32_t r0[4], r1[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            r0[k] = yuv_decode_px((ya >> (8u * k)) & 0xffu, k < 2u ? ca : cb, swap);
            r1[k] = yuv_decode_px((yb >> (8u * k)) & 0xffu, k < 2u ? ca : cb, swap);
        }
        yuv_store_bgr<CH>(dst + (size_t)y * pitch, r0, n);
        yuv_store_bgr<CH>(dst + (size_t)(y + 1u) * pitch, r1, n);
    }
}

// A launch converts the frames of the slice that have CH channels and skips the others (uniform).  Every load lies inside the
// source: bytes [x * CH, (x + n) * CH) of rows y, y + 1.  Every store lies inside the stacked output frame and that inside the
// buffer (checked): the Y dword ends at x + 4 <= pitch; the pair dword likewise; I420: bytes [x / 2, x / 2 + 2) of a chroma row
// and, from the row's last lane, the two pad bytes before the pitch where there are any.
template <uint32_t LAYOUT, uint32_t CH>
__global__ __launch_bounds__(256) void bgr_to_yuv(YuvArgs a) {
    kptr<YuvFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    if (unit >= a.n_units || a.n_frames == 0u) return;
    const uint32_t f = yuv_frame_of(frames, a.n_frames, unit);
    if (frames[f].channels != CH) return;
    const uint32_t w = frames[f].width, h = frames[f].height, pitch = frames[f].pitch;
    const uint64_t off = frames[f].dst_off;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blocks_per_row = (w + YUV_BLOCK_W - 1u) / YUV_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t x = bx * YUV_BLOCK_W + lane * YUV_LANE_W;
    const uint32_t y1 = min((by + 1u) * YUV_BLOCK_H, h);
    const bool inside = ((w | h) & 1u) == 0u && pitch == yuv_align4(w) && (off & 3u) == 0u && off + yuv_frame_bytes(LAYOUT, w, h) <= a.dst_bytes;
    if (!inside || x >= w) return;
    const uint32_t n = min(YUV_LANE_W, w - x);
    const size_t ss = frames[f].y_stride;
    const uint8_t* src = frames[f].y + (size_t)x * CH;
    const uint32_t cp = yuv_plane_pitch(LAYOUT, w, 1u);
    uint8_t* dy = a.dst + off + x;
    uint8_t* dc0 = a.dst + off + yuv_plane_off(LAYOUT, w, h, 1u) + (LAYOUT == YUV_I420 ? x >> 1 : x);
    uint8_t* dc1 = a.dst + off + yuv_plane_off(LAYOUT, w, h, 2u) + (x >> 1);   // (I420 only)
    const bool swap = a.swap_rb != 0u;
    const bool row_end = x + YUV_LANE_W >= w && (x >> 1) + 2u < cp;            // I420: this lane zeroes the chroma rows' last two pad bytes
    for (uint32_t y = by * YUV_BLOCK_H + 2u * wave; y < y1; y += 2u * YUV_WAVES) {
        uint32_t r0[4], r1[4];
        yuv_load_bgr<CH>(src + (size_t)y * ss, n, r0);
        yuv_load_bgr<CH>(src + (size_t)(y + 1u) * ss, n, r1);
        uint32_t ya = yuv_luma(r0[0], swap) | yuv_luma(r0[1], swap) << 8, yb = yuv_luma(r1[0], swap) | yuv_luma(r1[1], swap) << 8;
        uint32_t uv0 = yuv_uv(r0[0], swap), uv1 = 0u;
        if (n == 4u) {
            ya |= yuv_luma(r0[2], swap) << 16 | yuv_luma(r0[3], swap) << 24;
            yb |= yuv_luma(r1[2], swap) << 16 | yuv_luma(r1[3], swap) << 24;
            uv1 = yuv_uv(r0[2], swap);
        }
        *reinterpret_cast<uint32_t*>(dy + (size_t)y * pitch) = ya;              // (n = 2: with the row's two pad bytes)
        *reinterpret_cast<uint32_t*>(dy + (size_t)(y + 1u) * pitch) = yb;
        const size_t crow = (size_t)(y >> 1) * cp;
        if (LAYOUT == YUV_I420) {
            *reinterpret_cast<uint16_t*>(dc0 + crow) = (uint16_t)((uv0 & 0xffu) | (uv1 & 0xffu) << 8);
            *reinterpret_cast<uint16_t*>(dc1 + crow) = (uint16_t)((uv0 >> 8) | (uv1 >> 8) << 8);
            if (row_end) {
                *reinterpret_cast<uint16_t*>(dc0 + crow + 2u) = (uint16_t)0;
                *reinterpret_cast<uint16_t*>(dc1 + crow + 2u) = (uint16_t)0;
            }
        } else {
            if (LAYOUT == YUV_NV21) {
                uv0 = (uv0 >> 8) | (uv0 & 0xffu) << 8;
                uv1 = (uv1 >> 8) | (uv1 & 0xffu) << 8;
            }
            *reinterpret_cast<uint32_t*>(dc0 + crow) = uv0 | uv1 << 16;
        }
    }
}

namespace {
template <uint32_t CH>
void launch_decode(const YuvArgs& a, hipStream_t st) {
    if (a.layout == YUV_NV12) hipLaunchKernelGGL((yuv_to_bgr<YUV_NV12, CH>), dim3(a.n_units), dim3(256), 0, st, a);
    else if (a.layout == YUV_NV21) hipLaunchKernelGGL((yuv_to_bgr<YUV_NV21, CH>), dim3(a.n_units), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((yuv_to_bgr<YUV_I420, CH>), dim3(a.n_units), dim3(256), 0, st, a);
}
template <uint32_t CH>
void launch_encode(const YuvArgs& a, hipStream_t st) {
    if (a.layout == YUV_NV12) hipLaunchKernelGGL((bgr_to_yuv<YUV_NV12, CH>), dim3(a.n_units), dim3(256), 0, st, a);
    else if (a.layout == YUV_NV21) hipLaunchKernelGGL((bgr_to_yuv<YUV_NV21, CH>), dim3(a.n_units), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((bgr_to_yuv<YUV_I420, CH>), dim3(a.n_units), dim3(256), 0, st, a);
}
}  // namespace

// a.layout: the frames of the launch that have it are converted (the driver launches once per layout a slice holds)
int launch_yuv_to_bgr(const YuvArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    if (a.layout > YUV_I420 || (a.channels != 3u && a.channels != 4u)) return (int)hipErrorInvalidValue;
    if (a.channels == 3u) launch_decode<3u>(a, (hipStream_t)stream_);
    else launch_decode<4u>(a, (hipStream_t)stream_);
    return (int)hipGetLastError();
}

// a.channels: 3 or 4 — the sources of the launch that have as many are converted
int launch_bgr_to_yuv(const YuvArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    if (a.layout > YUV_I420 || (a.channels != 3u && a.channels != 4u)) return (int)hipErrorInvalidValue;
    if (a.channels == 3u) launch_encode<3u>(a, (hipStream_t)stream_);
    else launch_encode<4u>(a, (hipStream_t)stream_);
    return (int)hipGetLastError();
}

}  // namespace vj
