// gfx950 kernel of the mixed-size entry points (vj_detect_mixed, vj_detect_opencv_mixed, vj_pack_frames): the gray
// images of frames of any sizes, strides and channel counts, each written to its slot of ONE 8-bit atlas, all frames of the atlas in
// ONE launch — the frames are a few ten thousand pixels each, a launch per frame would make the call launch-bound.  The atlas is
// then integrated as one frame and every frame runs as a region of it.
//
// A workgroup is an ATLAS_BLOCK_W x ATLAS_BLOCK_H block of one frame (vj_atlas_units.hpp says why that shape), a wave one of its
// rows, a thread four pixels of the row: load_gray4 — the ingest conversion of the integral kernels, so BGR / BGRA frames give the
// bytes vj_grayscale gives — and one dword store.  blockIdx.x is the unit within the atlas; the frame comes from a binary search of
// the frame table's unit prefix (uniform: scalar loads), as pyramid_regions finds its level image.
//   reads   load_gray4 takes whole dwords only where the four pixels lie inside the row AND the address is 4-byte aligned; odd
//           pointers, odd strides and a row's last partial dword go byte by byte, and no byte at or beyond w * channels of a row is
//           touched (a source may end with its last row).
//   stores  always one aligned dword: slot origins, the atlas pitch and a thread's column are multiples of 4, and a slot is
//           align4(w) wide, so a row's last dword — its pixels beyond w are written as 0 — stays inside the slot.
// No LDS, no scratch; bound by the byte traffic.
//
// EQ (VJ_FLAG_EQUALIZE_HIST): the second instantiation sends the four pixels through the frame's look-up table
// (equalize_lut, vj_equalize.hip) before the store — the table staged in LDS, one byte per thread, one barrier that every thread
// reaches before the first return.  atlas_pack<false> is the kernel as it was, instruction for instruction.
#include <hip/hip_runtime.h>
#include "vj_atlas_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

template <bool EQ>
__global__ __launch_bounds__(256) void atlas_pack(AtlasPackArgs a) {
    __shared__ uint8_t lut[256];   // (EQ only: never touched, and not allocated, otherwise)
    kptr<AtlasFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    uint32_t lo = 0, hi = a.n_frames;   // the last frame whose first unit is <= unit
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (frames[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    if constexpr (EQ) {
        lut[threadIdx.x] = a.lut[(size_t)lo * 256u + threadIdx.x];
        __syncthreads();
    }
    const uint32_t w = frames[lo].w, h = frames[lo].h, ox = frames[lo].ox, oy = frames[lo].oy;
    const uint32_t blocks_per_row = (w + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W;
    const uint32_t u = unit - frames[lo].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * ATLAS_BLOCK_W + (threadIdx.x & 63u) * 4u, dy = by * ATLAS_BLOCK_H + (threadIdx.x >> 6);
    // inside the frame, and the dword inside the atlas (the host lays the slots out and checks them so; a store never leaves it)
    if (dy >= h || dx >= w || ((ox | a.atlas_pitch) & 3u) != 0u) return;
    if (ox + dx + 4u > a.atlas_pitch || ox + dx >= a.atlas_w || oy + dy >= a.atlas_h) return;
    const uint8_t* row = frames[lo].src + (size_t)dy * frames[lo].stride;
    uint32_t v = load_gray4(row, dx, w, frames[lo].channels);
    if constexpr (EQ) v = lut_gray4(lut, v);
    *reinterpret_cast<uint32_t*>(a.atlas + (size_t)(oy + dy) * a.atlas_pitch + ox + dx) = v;
}

int launch_atlas_pack(const AtlasPackArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    dim3 g(a.n_units), b(256);
    if (a.lut) hipLaunchKernelGGL(atlas_pack<true>, g, b, 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL(atlas_pack<false>, g, b, 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
