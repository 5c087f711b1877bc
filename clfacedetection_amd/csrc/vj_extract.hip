// gfx950 kernel of vj_extract: every region of a call — a crop of one of its frames, replicated beyond the frame's
// border — resized to one fixed size, per channel, device in, device out:
//   extract_regions    out[k] = cv::resize(crop_k, (out_w, out_h), INTER_LINEAR), interleaved or planar, or gray through BGR2GRAY
// The arithmetic is pyramid_levels' / prep_resize's (vj_pyramid.hip, vj_prep.hip), integer only: horizontal
// h = S[i0] * c0 + S[i1] * c1 with 11-bit weights, vertical (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, the
// 2 x 2 mean (sum + 2) >> 2 where the crop is exactly twice the output, a copy where it has the output's size.  The taps come from
// the host (build_taps) and index the CROP, so they clamp at the crop's edges; tap + crop origin is then clamped to the frame.
//
// A workgroup is a block of one region's output rows (the region from a binary search of the records' unit prefix: uniform, scalar
// loads — as prep_resize finds its frame), a wave one row at a time, a lane one four-byte SLOT of the row: rows are dense, so a
// row's first byte lies at any address, and slot s holds the bytes [4 s - (A & 3), 4 s - (A & 3) + 4) of a row at address A.  A slot
// wholly inside the row is ONE aligned dword store; the ragged slots at a row's head and tail are stored byte by byte.
// -DEXTRACT_BYTE_STORES (tests/measure_extract.py: what the dword store buys): every slot byte by byte.
#include <hip/hip_runtime.h>
#include "vj_extract_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {
constexpr uint32_t EXTRACT_WAVES = 4;   // waves per workgroup

// the last region whose first unit is <= unit; uniform, scalar loads
__device__ __forceinline__ uint32_t extract_region_of(kptr<ExtractRegionDev> regs, uint32_t n, uint32_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (regs[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t hi) { return min(max(v, 0), hi); }

// channel c of pixel x of a frame row (x inside the frame); conv: the pixel's gray value
__device__ __forceinline__ uint32_t extract_px(const uint8_t* row, uint32_t x, uint32_t sch, uint32_t c, bool conv) {
    const uint8_t* p = row + (size_t)x * sch;
    if (conv) return bgr2gray(p[0], p[1], p[2]);
    return (uint32_t)p[c];
}
}  // namespace

// Every load lies inside its frame: a source index is min(max(origin + tap, 0), size - 1), or — the wide loads — inside a crop that
// lies inside the frame.  Every store lies inside the region's rows * row_bytes bytes and those inside the buffer (checked below).
__global__ __launch_bounds__(256) void extract_regions(ExtractArgs a) {
    kptr<ExtractRegionDev> regs = as_k(a.regions);
    const uint32_t unit = blockIdx.x;
    const uint32_t k = extract_region_of(regs, a.n_regions, unit);
    const uint32_t B = a.row_bytes, R = a.rows, C = a.C;
    const uint64_t off = regs[k].dst_off;
    if (R == 0u || B == 0u || off + (uint64_t)R * B > a.dst_bytes) return;   // (the host lays the regions out inside the buffer)
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blocks_per_row = ((B + 6u) / 4u + EXTRACT_BLOCK_SLOTS - 1u) / EXTRACT_BLOCK_SLOTS;
    const uint32_t u = unit - regs[k].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t r1 = min((by + 1u) * EXTRACT_BLOCK_H, R);

    const uint8_t* src = regs[k].src;
    const size_t stride = regs[k].stride;
    const uint32_t sch = regs[k].channels, mode = regs[k].mode, cw = regs[k].cw, chh = regs[k].ch;
    const int32_t fw = regs[k].fw, fh = regs[k].fh, x0 = regs[k].x0, y0 = regs[k].y0;
    const bool conv = a.gray != 0u && sch > 1u;
    // wide loads: the crop wholly inside the frame, and the output's bytes are the source's (copy) or a gray source (mean)
    const bool crop_inside = x0 >= 0 && y0 >= 0 && (int64_t)x0 + cw <= (int64_t)fw && (int64_t)y0 + chh <= (int64_t)fh;
    const bool wide_copy = crop_inside && mode == EXTRACT_COPY && !conv && (a.planar == 0u || sch == 1u) && sch == C;
    const bool wide_area = crop_inside && mode == EXTRACT_AREA && sch == 1u;
    kptr<uint32_t> taps_k = as_k(reinterpret_cast<const uint32_t*>(a.taps));

    for (uint32_t r = by * EXTRACT_BLOCK_H + wave; r < r1; r += EXTRACT_WAVES) {   // (uniform: every lane of the wave walks the rows)
        uint8_t* drow = a.dst + off + (size_t)r * B;
        const uint32_t m = (uint32_t)((uintptr_t)drow & 3u);
        const int32_t b0 = (int32_t)((bx * EXTRACT_BLOCK_SLOTS + lane) * 4u) - (int32_t)m;
        const int32_t lo = max(b0, 0), hi = min(b0 + 4, (int32_t)B);
        if (lo >= hi) continue;
        // the row's channel plane and output row, and its two source rows (uniform)
        uint32_t cpl = 0, y = r;
        if (a.planar != 0u) {
            cpl = r / a.out_h;
            y = r - cpl * a.out_h;
        }
        int32_t yi0, yi1, wb0 = 0, wb1 = 0;
        if (mode == EXTRACT_COPY) {
            yi0 = yi1 = (int32_t)y;
        } else if (mode == EXTRACT_AREA) {
            yi0 = 2 * (int32_t)y;
            yi1 = yi0 + 1;
        } else {
            const uint32_t yt = regs[k].ytab + y;
            const uint32_t wy0 = taps_k[2u * yt], wy1 = taps_k[2u * yt + 1u];   // the row's tap: scalar loads
            yi0 = (int32_t)(wy0 & 0xffffu);
            yi1 = (int32_t)(wy0 >> 16);
            wb0 = (int32_t)(int16_t)(wy1 & 0xffffu);
            wb1 = (int32_t)(int16_t)(wy1 >> 16);
        }
        const uint8_t* r0 = src + (size_t)clampi(y0 + yi0, fh - 1) * stride;
        const uint8_t* r1p = src + (size_t)clampi(y0 + yi1, fh - 1) * stride;

        uint32_t packed = 0;
        bool done = false;
        if (hi - lo == 4) {
            if (wide_copy) {          // output bytes b0 .. b0 + 3 are the crop row's bytes b0 .. b0 + 3: b0 + 4 <= B = cw * sch
                const uint8_t* p = r0 + (size_t)x0 * sch + (uint32_t)b0;
                if (((uintptr_t)p & 3u) == 0u) {
                    packed = *reinterpret_cast<const uint32_t*>(p);
                    done = true;
                }
            } else if (wide_area) {   // gray: output bytes b0 .. b0 + 3 from crop columns 2 b0 .. 2 b0 + 7 of two rows: 2 b0 + 8 <= cw
                const uint8_t* p0 = r0 + (size_t)x0 + 2u * (uint32_t)b0;
                const uint8_t* p1 = r1p + (size_t)x0 + 2u * (uint32_t)b0;
                if ((((uintptr_t)p0 | (uintptr_t)p1) & 3u) == 0u) {
                    const uint32_t a0 = reinterpret_cast<const uint32_t*>(p0)[0], a1 = reinterpret_cast<const uint32_t*>(p0)[1];
                    const uint32_t c0 = reinterpret_cast<const uint32_t*>(p1)[0], c1 = reinterpret_cast<const uint32_t*>(p1)[1];
                    // pairs of bytes summed side by side: (even + odd) of both rows in 16-bit halves
                    const uint32_t s0 = (a0 & 0x00ff00ffu) + ((a0 >> 8) & 0x00ff00ffu) + (c0 & 0x00ff00ffu) + ((c0 >> 8) & 0x00ff00ffu) + 0x00020002u;
                    const uint32_t s1 = (a1 & 0x00ff00ffu) + ((a1 >> 8) & 0x00ff00ffu) + (c1 & 0x00ff00ffu) + ((c1 >> 8) & 0x00ff00ffu) + 0x00020002u;
                    packed = ((s0 >> 2) & 0xffu) | (((s0 >> 18) & 0xffu) << 8) | (((s1 >> 2) & 0xffu) << 16) | (((s1 >> 18) & 0xffu) << 24);
                    done = true;
                }
            }
        }
        if (!done) {
#pragma unroll
            for (int32_t q = 0; q < 4; ++q) {
                const int32_t b = b0 + q;
                if (b < lo || b >= hi) continue;
                uint32_t x = (uint32_t)b, c = cpl;
                if (a.planar == 0u && C > 1u) {
                    x = C == 3u ? (uint32_t)b / 3u : (uint32_t)b >> 2;
                    c = (uint32_t)b - x * C;
                }
                uint32_t v;
                if (mode == EXTRACT_COPY) {
                    v = extract_px(r0, (uint32_t)clampi(x0 + (int32_t)x, fw - 1), sch, c, conv);
                } else if (mode == EXTRACT_AREA) {
                    const uint32_t xs0 = (uint32_t)clampi(x0 + 2 * (int32_t)x, fw - 1), xs1 = (uint32_t)clampi(x0 + 2 * (int32_t)x + 1, fw - 1);
                    v = (extract_px(r0, xs0, sch, c, conv) + extract_px(r0, xs1, sch, c, conv) + extract_px(r1p, xs0, sch, c, conv) +
                         extract_px(r1p, xs1, sch, c, conv) + 2u) >> 2;
                } else {
                    const uint2 t = *reinterpret_cast<const uint2*>(a.taps + regs[k].xtab + x);   // the column's tap: a vector load
                    const uint32_t xs0 = (uint32_t)clampi(x0 + (int32_t)(t.x & 0xffffu), fw - 1), xs1 = (uint32_t)clampi(x0 + (int32_t)(t.x >> 16), fw - 1);
                    const int32_t c0 = (int32_t)(int16_t)(t.y & 0xffffu), c1 = (int32_t)(int16_t)(t.y >> 16);
                    const int32_t s00 = (int32_t)extract_px(r0, xs0, sch, c, conv), s01 = (int32_t)extract_px(r0, xs1, sch, c, conv);
                    const int32_t s10 = (int32_t)extract_px(r1p, xs0, sch, c, conv), s11 = (int32_t)extract_px(r1p, xs1, sch, c, conv);
                    const int32_t h0 = s00 * c0 + s01 * c1, h1 = s10 * c0 + s11 * c1;
                    v = (uint32_t)((((wb0 * (h0 >> 4)) >> 16) + ((wb1 * (h1 >> 4)) >> 16) + 2) >> 2);
                }
                packed |= (v & 0xffu) << (8 * q);
            }
        }
#ifndef EXTRACT_BYTE_STORES
        if (hi - lo == 4) {
            *reinterpret_cast<uint32_t*>(drow + b0) = packed;   // (drow + b0) & 3 == 0: b0 = 4 slot - (drow & 3)
            continue;
        }
#endif
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t b = b0 + q;
            if (b >= lo && b < hi) drow[b] = (uint8_t)(packed >> (8 * q));
        }
    }
}

int launch_extract(const ExtractArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_regions == 0u) return 0;
    hipLaunchKernelGGL(extract_regions, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
