// gfx950 kernel of vj_extract_affine: every region of a call — one affine map from the output's pixels into one of
// the call's frames, the frame's border replicated — sampled bilinearly to one fixed size, per channel, device in, device out:
//   affine_regions    out[k][y][x] = the blend of the 2 x 2 source pixels at m_k (x, y), interleaved or planar, or gray through BGR2GRAY
// The arithmetic is integer but for the position terms: ax[x] = rne((m0 x) 1024), bx[x] = rne((m3 x) 1024) per lane and
// X0[y] = rne((m1 y + m2) 1024) + 16, Y0[y] = rne((m4 y + m5) 1024) + 16 once per row, in f64 ON THE DEVICE (IEEE multiply and add,
// no contraction: -ffp-contract=off; __double2int_rn rounds half to even) — the host uploads the six matrix entries and no table.
// X = (X0 + ax) >> 5 holds the source column in its bits 5.. and the 1/32-pixel fraction in its low five; four 15-bit weights that
// sum to 32768; out = (sum + 16384) >> 15.
//
// The decomposition is extract_regions' (vj_extract.hip): a workgroup is a block of one region's output rows (the region from a
// binary search of the records' unit prefix: uniform, scalar loads), a wave one row at a time, a lane one four-byte SLOT of the row:
// slot s holds the bytes [4 s - (A & 3), 4 s - (A & 3) + 4) of a row at address A.  A slot wholly inside the row is ONE aligned dword
// store; the ragged slots at a row's head and tail are stored byte by byte.  A lane computes a pixel's position once for the bytes
// of its slot that belong to that pixel; every byte loads its own four taps (one channel each, three for a gray conversion).
#include <hip/hip_runtime.h>
#include "vj_affine_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {
constexpr uint32_t AFFINE_WAVES = 4;   // waves per workgroup

// the last region whose first unit is <= unit; uniform, scalar loads
__device__ __forceinline__ uint32_t affine_region_of(kptr<AffineRegionDev> regs, uint32_t n, uint32_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (regs[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int32_t affine_clamp(int32_t v, int32_t hi) { return min(max(v, 0), hi); }

// channel c of pixel x of a frame row (x inside the frame); conv: the pixel's gray value
__device__ __forceinline__ uint32_t affine_px(const uint8_t* row, uint32_t x, uint32_t sch, uint32_t c, bool conv) {
    const uint8_t* p = row + (size_t)x * sch;
    if (conv) return bgr2gray(p[0], p[1], p[2]);
    return (uint32_t)p[c];
}
}  // namespace

// Every load lies inside its frame: a source index is min(max(v, 0), size - 1) and a channel index below the source's channel count
// (c < C = channels without the gray flag, 0 with it).  Every store lies inside the region's rows * row_bytes bytes and those inside
// the buffer (checked below).  The host's limits (|terms| <= 2^19 pixels) keep every rne inside int32 and X0 + ax below 2^30 + 16.
__global__ __launch_bounds__(256) void affine_regions(AffineArgs a) {
    kptr<AffineRegionDev> regs = as_k(a.regions);
    const uint32_t unit = blockIdx.x;
    const uint32_t k = affine_region_of(regs, a.n_regions, unit);
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
    const uint32_t sch = regs[k].channels;
    const int32_t fw = regs[k].fw, fh = regs[k].fh;
    const double m0 = regs[k].m[0], m1 = regs[k].m[1], m2 = regs[k].m[2], m3 = regs[k].m[3], m4 = regs[k].m[4], m5 = regs[k].m[5];
    const bool conv = a.gray != 0u && sch > 1u;

    for (uint32_t r = by * EXTRACT_BLOCK_H + wave; r < r1; r += AFFINE_WAVES) {   // (uniform: every lane of the wave walks the rows)
        uint8_t* drow = a.dst + off + (size_t)r * B;
        const uint32_t mis = (uint32_t)((uintptr_t)drow & 3u);
        const int32_t b0 = (int32_t)((bx * EXTRACT_BLOCK_SLOTS + lane) * 4u) - (int32_t)mis;
        const int32_t lo = max(b0, 0), hi = min(b0 + 4, (int32_t)B);
        if (lo >= hi) continue;
        // the row's channel plane and output row, and its two row terms (uniform)
        uint32_t cpl = 0, y = r;
        if (a.planar != 0u) {
            cpl = r / a.out_h;
            y = r - cpl * a.out_h;
        }
        const double yd = (double)y;
        const int32_t X0 = __double2int_rn((m1 * yd + m2) * 1024.0) + 16;
        const int32_t Y0 = __double2int_rn((m4 * yd + m5) * 1024.0) + 16;

        uint32_t packed = 0, x_at = 0xffffffffu;
        uint32_t w00 = 0, w01 = 0, w10 = 0, w11 = 0, xs0 = 0, xs1 = 0;
        const uint8_t* row0 = src;
        const uint8_t* row1 = src;
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t b = b0 + q;
            if (b < lo || b >= hi) continue;
            uint32_t x = (uint32_t)b, c = cpl;
            if (a.planar == 0u && C > 1u) {
                x = C == 3u ? (uint32_t)b / 3u : (uint32_t)b >> 2;
                c = (uint32_t)b - x * C;
            }
            if (x != x_at) {   // the pixel's position, weights and clamped taps: once for the bytes of one pixel
                x_at = x;
                const double xd = (double)x;
                const int32_t X = (X0 + __double2int_rn((m0 * xd) * 1024.0)) >> 5;
                const int32_t Y = (Y0 + __double2int_rn((m3 * xd) * 1024.0)) >> 5;
                const int32_t sx = X >> 5, sy = Y >> 5;
                const uint32_t fx = (uint32_t)(X & 31), fy = (uint32_t)(Y & 31);
                w00 = (32u - fx) * (32u - fy) * 32u;
                w01 = fx * (32u - fy) * 32u;
                w10 = (32u - fx) * fy * 32u;
                w11 = fx * fy * 32u;
                xs0 = (uint32_t)affine_clamp(sx, fw - 1);
                xs1 = (uint32_t)affine_clamp(sx + 1, fw - 1);
                row0 = src + (size_t)affine_clamp(sy, fh - 1) * stride;
                row1 = src + (size_t)affine_clamp(sy + 1, fh - 1) * stride;
            }
            const uint32_t p00 = affine_px(row0, xs0, sch, c, conv), p01 = affine_px(row0, xs1, sch, c, conv);
            const uint32_t p10 = affine_px(row1, xs0, sch, c, conv), p11 = affine_px(row1, xs1, sch, c, conv);
            const uint32_t v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + 16384u) >> 15;
            packed |= (v & 0xffu) << (8 * q);
        }
        if (hi - lo == 4) {
            *reinterpret_cast<uint32_t*>(drow + b0) = packed;   // (drow + b0) & 3 == 0: b0 = 4 slot - (drow & 3)
            continue;
        }
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t b = b0 + q;
            if (b >= lo && b < hi) drow[b] = (uint8_t)(packed >> (8 * q));
        }
    }
}

int launch_affine(const AffineArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_regions == 0u) return 0;
    hipLaunchKernelGGL(affine_regions, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
