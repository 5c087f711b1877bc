// Small device-side helpers shared by the gfx950 kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vj {

// Read-only, wave-uniform data goes through address space 4 so that the compiler may
// use s_load (scalar cache) even though the kernel also stores to global memory.
template <typename T>
using kptr = const T __attribute__((address_space(4)))*;
template <typename T>
__device__ __forceinline__ kptr<T> as_k(const T* p) {
    return (kptr<T>)(uintptr_t)p;
}

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// Number of set bits of `mask` below this lane.
__device__ __forceinline__ uint32_t mbcnt(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Image gathers go through buffer loads: the 128-bit resource descriptor and the
// scalar offset (a rectangle corner, uniform across the wave) live in SGPRs and the
// lane contributes only its 32-bit window offset, so a gather costs no VALU address
// arithmetic at all:  buffer_load_dword v, v_off, s[rsrc], s_corner offen.
// Out-of-range offsets return 0 instead of faulting.
using rsrc_t = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ uint32_t ld_u32(rsrc_t r, uint32_t lane_off, uint32_t uniform_off) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, lane_off, uniform_off, 0);
}
__device__ __forceinline__ uint64_t ld_u64(rsrc_t r, uint32_t lane_off, uint32_t uniform_off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, lane_off, uniform_off, 0);
    return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
}

__device__ __forceinline__ uint32_t load_px4(const uint8_t* row, uint32_t x, uint32_t width) {
    // four pixels x..x+3 packed little-endian; pixels beyond the row read as 0
    const uint8_t* p = row + x;
    if (x + 4 <= width && ((uintptr_t)p & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
    uint32_t v = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (x + c < width) v |= (uint32_t)p[c] << (8 * c);
    return v;
}

// Image ingest: 3-channel BGR / 4-channel BGRA frames are converted on the fly with OpenCV's 8-bit
// fixed-point BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14 (OpenCV 2.4.2 imgproc, the cvCvtColor the
// reference calls at clif.cpp:328 — third-party arithmetic), fused into both pixel reads
// of the integral so that no gray copy is written.
__device__ __forceinline__ uint32_t bgr2gray(uint32_t b, uint32_t g, uint32_t r) {
    return (b * 1868u + g * 9617u + r * 4899u + 8192u) >> 14;
}
__device__ __forceinline__ uint32_t load_gray4(const uint8_t* row, uint32_t x, uint32_t width, uint32_t ch) {
    if (ch <= 1u) return load_px4(row, x, width);
    const uint8_t* p = row + (size_t)x * ch;
    uint32_t v = 0;
    if (x + 4 <= width && ((uintptr_t)p & 3u) == 0) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
        if (ch == 3u) {   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
            v = bgr2gray(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu) |
                bgr2gray(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu) << 8 |
                bgr2gray((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu) << 16 |
                bgr2gray((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24) << 24;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v |= bgr2gray(w[c] & 0xffu, (w[c] >> 8) & 0xffu, (w[c] >> 16) & 0xffu) << (8 * c);
        }
        return v;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (x + c < width) v |= bgr2gray(p[c * ch], p[c * ch + 1u], p[c * ch + 2u]) << (8 * c);
    return v;
}

// VJ_FLAG_EQUALIZE_HIST: four packed pixels through a frame's look-up table in LDS (vj_equalize.hip, vj_atlas.hip).  Pixels beyond
// the row come as 0 from load_gray4 and stay 0: lut[0] is 0 in every table equalize_lut writes.
__device__ __forceinline__ uint32_t lut_gray4(const uint8_t* lut, uint32_t v) {
    return (uint32_t)lut[v & 0xffu] | (uint32_t)lut[(v >> 8) & 0xffu] << 8 | (uint32_t)lut[(v >> 16) & 0xffu] << 16 | (uint32_t)lut[v >> 24] << 24;
}

// CV_HAAR_DO_CANNY_PRUNING's test (tempcv.cpp:1147-1158): the edge map's sum s and the frame's own sum sq (pq points at `sum`)
// over the pruning rectangle, four-corner differences in int; pruned iff s < 100 || sq < 20
__device__ __forceinline__ bool cv_pruned(rsrc_t eimg, rsrc_t img, uint32_t off, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3) {
    const int32_t s = (int32_t)(ld_u32(eimg, off, e0) - ld_u32(eimg, off, e1) - ld_u32(eimg, off, e2) + ld_u32(eimg, off, e3));
    const int32_t sq = (int32_t)(ld_u32(img, off, e0) - ld_u32(img, off, e1) - ld_u32(img, off, e2) + ld_u32(img, off, e3));
    return s < 100 || sq < 20;
}

// 64-byte node record as the scalar unit loads it (one s_load_dwordx16).
typedef uint32_t NodeRecDev __attribute__((ext_vector_type(16)));

}  // namespace vj
