// gfx950 kernels of vj_extract_yuv / vj_extract_affine_yuv: regions of NV12 / NV21 / I420 frames resized, or warped,
// to one fixed size as BGR / BGRA / RGB / RGBA or gray, device in, device out — what extract_regions (vj_extract.hip) and
// affine_regions (vj_affine.hip) write when their frames are what yuv_to_bgr (vj_yuv.hip) made of these, without that image:
//   extract_yuv_regions   out[k] = cv::resize(decode(crop_k), (out_w, out_h), INTER_LINEAR)
//   affine_yuv_regions    out[k][y][x] = the blend of the 2 x 2 decoded pixels at m_k (x, y)
// DECODE FIRST, per tap: a tap at the clamped luma pixel (cx, cy) is §4.21's decode of Y[cy][cx] and the chroma sample
// (cx >> 1, cy >> 1), saturated to bytes (alpha 255 with four channels; BGR2GRAY of the three bytes with the gray flag); the resize
// arithmetic of §4.17 or the blend of §4.19 then runs per channel on those bytes.  All clamps — the taps' at the crop's edges (in
// the host's tables), then the frame's — act on the luma coordinate; the chroma index follows from the clamped one.
//
// The decomposition is extract_regions': a workgroup is a block of one region's output rows (the region from a binary search of the
// records' unit prefix: uniform, scalar loads), a wave one row at a time, a lane one four-byte SLOT of the row: slot s holds the bytes
// [4 s - (A & 3), 4 s - (A & 3) + 4) of a row at address A.  A slot wholly inside the row is ONE aligned dword store; the ragged slots
// at a row's head and tail are stored byte by byte.  The work of a lane is PER PIXEL: for each pixel its slot touches (one or two of
// an interleaved row, four of a gray or planar one) the positions, taps and clamps are computed once, the taps are loaded as Y and a
// chroma pair, the chroma terms are computed once per DISTINCT chroma sample among them (taps x, x + 1 share theirs when x is even,
// rows likewise), every tap is decoded once to its three bytes, and then the channels the slot needs of that pixel are blended.
// A pair-plane sample is one 2-byte load where its address is even and two byte loads elsewhere: no load is wider than its alignment.
#include <hip/hip_runtime.h>
#include "vj_extract_yuv_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {
constexpr uint32_t EXTRACT_YUV_WAVES = 4;   // waves per workgroup
constexpr int32_t YUV_HALF = 1 << 19;

// the last region whose first unit is <= unit; uniform, scalar loads
template <typename Rec>
__device__ __forceinline__ uint32_t yuv_region_of(kptr<Rec> regs, uint32_t n, uint32_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (regs[mid].f.unit_first <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int32_t clampi(int32_t v, int32_t hi) { return min(max(v, 0), hi); }
__device__ __forceinline__ uint32_t sat8(int32_t t) { return (uint32_t)min(max(t, 0), 255); }

// a frame's planes and the BGR side of the call (uniform)
struct YuvSrc {
    const uint8_t* y;
    const uint8_t* c0;
    const uint8_t* c1;
    size_t ys, cs;
    uint32_t layout;
    int32_t fw, fh;
    bool swap, gray;
};
template <typename Rec>
__device__ __forceinline__ YuvSrc yuv_src(kptr<Rec> regs, uint32_t k, const ExtractYuvArgs& a) {
    return YuvSrc{regs[k].f.y, regs[k].f.c0, regs[k].f.c1, regs[k].f.y_stride, regs[k].f.c_stride, regs[k].f.layout, regs[k].f.fw, regs[k].f.fh,
                  a.swap_rb != 0u, a.gray != 0u};
}

// the terms the pixels of one chroma sample share (§4.21): the sample (cx, cy), cx < fw / 2, cy < fh / 2
struct ChromaTerms { int32_t b, g, r; };
__device__ __forceinline__ ChromaTerms chroma_at(const YuvSrc& s, uint32_t cx, uint32_t cy) {
    uint32_t U, V;
    if (s.layout == YUV_I420) {
        const size_t at = (size_t)cy * s.cs + cx;
        U = s.c0[at], V = s.c1[at];
    } else {
        const uint8_t* p = s.c0 + (size_t)cy * s.cs + 2u * (size_t)cx;
        uint32_t e, o;
        if (((uintptr_t)p & 1u) == 0u) {   // the pair in one 2-byte load
            const uint32_t w = *reinterpret_cast<const uint16_t*>(p);
            e = w & 0xffu, o = w >> 8;
        } else {
            e = p[0], o = p[1];
        }
        U = s.layout == YUV_NV12 ? e : o, V = s.layout == YUV_NV12 ? o : e;
    }
    const int32_t u = (int32_t)U - 128, v = (int32_t)V - 128;
    return ChromaTerms{YUV_HALF + 2116026 * u, YUV_HALF - 852492 * v - 409993 * u, YUV_HALF + 1673527 * v};
}

// The tap at luma pixel (x, y) inside the frame, decoded: its bytes in the output's channel order with alpha 255 in bits 24 .. 31,
// or — the gray flag — the BGR2GRAY of those three bytes in bits 0 .. 7
__device__ __forceinline__ uint32_t decode_tap(const YuvSrc& s, uint32_t x, uint32_t y, const ChromaTerms& c) {
    const int32_t yy = max((int32_t)s.y[(size_t)y * s.ys + x] - 16, 0) * 1220542;
    const uint32_t b = sat8((yy + c.b) >> 20), g = sat8((yy + c.g) >> 20), r = sat8((yy + c.r) >> 20);
    const uint32_t p0 = s.swap ? r : b, p2 = s.swap ? b : r;
    if (s.gray) return bgr2gray(p0, g, p2);
    return p0 | g << 8 | p2 << 16 | 0xff000000u;
}

// The four taps (x0 | x1, y0 | y1), all inside the frame: one chroma load and one set of terms per distinct sample among them
struct Taps4 { uint32_t t00, t01, t10, t11; };
__device__ __forceinline__ Taps4 decode_taps(const YuvSrc& s, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {
    const uint32_t cx0 = x0 >> 1, cx1 = x1 >> 1, cy0 = y0 >> 1, cy1 = y1 >> 1;
    const ChromaTerms c00 = chroma_at(s, cx0, cy0);
    ChromaTerms c01 = c00;
    if (cx1 != cx0) c01 = chroma_at(s, cx1, cy0);
    ChromaTerms c10 = c00, c11 = c01;
    if (cy1 != cy0) {
        c10 = chroma_at(s, cx0, cy1);
        c11 = c10;
        if (cx1 != cx0) c11 = chroma_at(s, cx1, cy1);
    }
    return Taps4{decode_tap(s, x0, y0, c00), decode_tap(s, x1, y0, c01), decode_tap(s, x0, y1, c10), decode_tap(s, x1, y1, c11)};
}

__device__ __forceinline__ int32_t chan(uint32_t t, uint32_t c) { return (int32_t)((t >> (8u * c)) & 0xffu); }

// pixel x and channel c of byte b of an output row
__device__ __forceinline__ void byte_of_row(const ExtractYuvArgs& a, uint32_t b, uint32_t cpl, uint32_t* x, uint32_t* c) {
    *x = b, *c = cpl;
    if (a.planar == 0u && a.C > 1u) {
        *x = a.C == 3u ? b / 3u : b >> 2;
        *c = b - *x * a.C;
    }
}

// a slot's bytes [lo, hi) of row `drow`, packed from bit 8 (b - b0): a whole slot as one dword — (drow + b0) & 3 == 0 by construction
__device__ __forceinline__ void store_slot(uint8_t* drow, int32_t b0, int32_t lo, int32_t hi, uint32_t packed) {
    if (hi - lo == 4) {
        *reinterpret_cast<uint32_t*>(drow + b0) = packed;
        return;
    }
#pragma unroll
    for (int32_t q = 0; q < 4; ++q) {
        const int32_t b = b0 + q;
        if (b >= lo && b < hi) drow[b] = (uint8_t)(packed >> (8 * q));
    }
}
}  // namespace

// Every load lies inside its plane: a luma index is min(max(origin + tap, 0), size - 1), a chroma index that shifted right by one —
// below size / 2, the sizes being even.  Every store lies inside the region's rows * row_bytes bytes and those inside the buffer
// (checked below).
__global__ __launch_bounds__(256) void extract_yuv_regions(ExtractYuvArgs a) {
    kptr<ExtractYuvRegionDev> regs = as_k(reinterpret_cast<const ExtractYuvRegionDev*>(a.regions));
    const uint32_t unit = blockIdx.x;
    if (unit >= a.n_units || a.n_regions == 0u) return;
    const uint32_t k = yuv_region_of(regs, a.n_regions, unit);
    const uint32_t B = a.row_bytes, R = a.rows;
    const uint64_t off = regs[k].dst_off;
    if (R == 0u || B == 0u || off + (uint64_t)R * B > a.dst_bytes) return;   // (the host lays the regions out inside the buffer)
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blocks_per_row = ((B + 6u) / 4u + EXTRACT_BLOCK_SLOTS - 1u) / EXTRACT_BLOCK_SLOTS;
    const uint32_t u = unit - regs[k].f.unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t r1 = min((by + 1u) * EXTRACT_BLOCK_H, R);

    const YuvSrc s = yuv_src(regs, k, a);
    const uint32_t mode = regs[k].mode;
    const int32_t x0 = regs[k].x0, y0 = regs[k].y0;
    if (s.fw < 2 || s.fh < 2) return;
    kptr<uint32_t> taps_k = as_k(reinterpret_cast<const uint32_t*>(a.taps));

    for (uint32_t r = by * EXTRACT_BLOCK_H + wave; r < r1; r += EXTRACT_YUV_WAVES) {   // (uniform: every lane of the wave walks the rows)
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
        const uint32_t ys0 = (uint32_t)clampi(y0 + yi0, s.fh - 1), ys1 = (uint32_t)clampi(y0 + yi1, s.fh - 1);

        uint32_t packed = 0, x_at = 0xffffffffu;
        Taps4 t = {0u, 0u, 0u, 0u};
        int32_t c0 = 0, c1 = 0;
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t b = b0 + q;
            if (b < lo || b >= hi) continue;
            uint32_t x, c;
            byte_of_row(a, (uint32_t)b, cpl, &x, &c);
            if (x != x_at) {   // the pixel's positions, clamps and decoded taps: once for the bytes of one pixel
                x_at = x;
                if (mode == EXTRACT_COPY) {
                    const uint32_t xs = (uint32_t)clampi(x0 + (int32_t)x, s.fw - 1);
                    t.t00 = decode_tap(s, xs, ys0, chroma_at(s, xs >> 1, ys0 >> 1));
                } else {
                    int32_t xi0 = 2 * (int32_t)x, xi1 = xi0 + 1;
                    if (mode == EXTRACT_BILINEAR) {
                        const uint2 tp = *reinterpret_cast<const uint2*>(a.taps + regs[k].xtab + x);   // the column's tap: a vector load
                        xi0 = (int32_t)(tp.x & 0xffffu);
                        xi1 = (int32_t)(tp.x >> 16);
                        c0 = (int32_t)(int16_t)(tp.y & 0xffffu);
                        c1 = (int32_t)(int16_t)(tp.y >> 16);
                    }
                    t = decode_taps(s, (uint32_t)clampi(x0 + xi0, s.fw - 1), (uint32_t)clampi(x0 + xi1, s.fw - 1), ys0, ys1);
                }
            }
            if (s.gray) c = 0u;   // (C = 1: the taps hold their gray value)
            uint32_t v;
            if (mode == EXTRACT_COPY) {
                v = (uint32_t)chan(t.t00, c);
            } else if (mode == EXTRACT_AREA) {
                v = (uint32_t)(chan(t.t00, c) + chan(t.t01, c) + chan(t.t10, c) + chan(t.t11, c) + 2) >> 2;
            } else {
                const int32_t h0 = chan(t.t00, c) * c0 + chan(t.t01, c) * c1, h1 = chan(t.t10, c) * c0 + chan(t.t11, c) * c1;
                v = (uint32_t)((((wb0 * (h0 >> 4)) >> 16) + ((wb1 * (h1 >> 4)) >> 16) + 2) >> 2);
            }
            packed |= (v & 0xffu) << (8 * q);
        }
        store_slot(drow, b0, lo, hi, packed);
    }
}

// Loads and stores: as above.  The host's limits (|terms| <= 2^19 pixels) keep every rne inside int32 and X0 + ax below 2^30 + 16.
__global__ __launch_bounds__(256) void affine_yuv_regions(ExtractYuvArgs a) {
    kptr<AffineYuvRegionDev> regs = as_k(reinterpret_cast<const AffineYuvRegionDev*>(a.regions));
    const uint32_t unit = blockIdx.x;
    if (unit >= a.n_units || a.n_regions == 0u) return;
    const uint32_t k = yuv_region_of(regs, a.n_regions, unit);
    const uint32_t B = a.row_bytes, R = a.rows;
    const uint64_t off = regs[k].dst_off;
    if (R == 0u || B == 0u || off + (uint64_t)R * B > a.dst_bytes) return;   // (the host lays the regions out inside the buffer)
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t blocks_per_row = ((B + 6u) / 4u + EXTRACT_BLOCK_SLOTS - 1u) / EXTRACT_BLOCK_SLOTS;
    const uint32_t u = unit - regs[k].f.unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t r1 = min((by + 1u) * EXTRACT_BLOCK_H, R);

    const YuvSrc s = yuv_src(regs, k, a);
    if (s.fw < 2 || s.fh < 2) return;
    const double m0 = regs[k].m[0], m1 = regs[k].m[1], m2 = regs[k].m[2], m3 = regs[k].m[3], m4 = regs[k].m[4], m5 = regs[k].m[5];

    for (uint32_t r = by * EXTRACT_BLOCK_H + wave; r < r1; r += EXTRACT_YUV_WAVES) {   // (uniform: every lane of the wave walks the rows)
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
        uint32_t w00 = 0, w01 = 0, w10 = 0, w11 = 0;
        Taps4 t = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int32_t q = 0; q < 4; ++q) {
            const int32_t b = b0 + q;
            if (b < lo || b >= hi) continue;
            uint32_t x, c;
            byte_of_row(a, (uint32_t)b, cpl, &x, &c);
            if (x != x_at) {   // the pixel's position, weights, clamped and decoded taps: once for the bytes of one pixel
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
                t = decode_taps(s, (uint32_t)clampi(sx, s.fw - 1), (uint32_t)clampi(sx + 1, s.fw - 1), (uint32_t)clampi(sy, s.fh - 1),
                                (uint32_t)clampi(sy + 1, s.fh - 1));
            }
            if (s.gray) c = 0u;   // (C = 1: the taps hold their gray value)
            const uint32_t v = ((uint32_t)chan(t.t00, c) * w00 + (uint32_t)chan(t.t01, c) * w01 + (uint32_t)chan(t.t10, c) * w10 +
                                (uint32_t)chan(t.t11, c) * w11 + 16384u) >> 15;
            packed |= (v & 0xffu) << (8 * q);
        }
        store_slot(drow, b0, lo, hi, packed);
    }
}

int launch_extract_yuv(const ExtractYuvArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_regions == 0u) return 0;
    if ((a.C != 1u && a.C != 3u && a.C != 4u) || (a.gray != 0u) != (a.C == 1u)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(extract_yuv_regions, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_affine_yuv(const ExtractYuvArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_regions == 0u) return 0;
    if ((a.C != 1u && a.C != 3u && a.C != 4u) || (a.gray != 0u) != (a.C == 1u)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(affine_yuv_regions, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
