// gfx950 kernels of vj_paint: the pixels inside, or around, the rectangles of a call changed IN PLACE — filled,
// outlined, pixelated or box-blurred, inside the rectangle or the ellipse inscribed in it.  All arithmetic is on integers.
//
// What makes in-place work safe: NO LAUNCH BOTH READS A FRAME AND WRITES ONE.  Phase 1 reads frames and writes scratch
//   paint_colsum   BLUR: per byte column of K the vertical kk-row sums, rows clamped to K, as 16-bit values (255 * 255 fits)
//   paint_cells    PIXELATE: the rounded mean of every cell, per channel, one byte each
// phase 2 reads scratch and writes frames
//   paint_apply    every mode: the value of every painted byte, stored iff its pixel is in the region's painted set and in no LATER
//                  region's of the same frame (the host's overlap list: usually empty)
// and stream order separates them.  paint_apply decomposes as extract_regions does: a workgroup is a block of K rows x four-byte
// slots of one region (the region from a binary search of the records' unit prefix: uniform, scalar loads), a wave one row at a
// time, a lane one slot of the FRAME row: slot s of a K row at address A holds its bytes [4 s - (A & 3), 4 s - (A & 3) + 4).  A slot
// whose four bytes are all in the row, painted and owned is ONE aligned dword store; every other slot is stored byte by byte, owned
// bytes only — a read-modify-write of a dword that holds a byte the region does not own would race with the workgroup that owns it.
#include <hip/hip_runtime.h>
#include "vj_paint_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {

// the last region whose first unit (apply or phase 1) is <= unit; uniform, scalar loads
template <bool PRE>
__device__ __forceinline__ uint32_t paint_region_of(kptr<PaintRegionDev> regs, uint32_t n, uint32_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((PRE ? regs[mid].pre_first : regs[mid].unit_first) <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The staged prefix sums of one wave's row segment: at most ceil(256 / C) + 1 pixels of the block plus 2 * 127 of the halo, times C
// channels: 510 (C = 1), 1023 (C = 3), 1276 (C = 4) values.
constexpr uint32_t PAINT_PREFIX_MAX = 1280;

}  // namespace

// Every load lies inside K, which lies inside the frame; every store lies inside the scratch range the host gave the region, and
// that inside the scratch (checked).
__global__ __launch_bounds__(256) void paint_colsum(PaintArgs a) {
    kptr<PaintRegionDev> regs = as_k(a.regions);
    const uint32_t unit = blockIdx.x;
    const uint32_t k = paint_region_of<true>(regs, a.n_regions, unit);
    const PaintGeom g = paint_geom(regs + k);
    const uint32_t C = regs[k].channels;
    const int32_t kw = g.cx1 - g.cx0, kh = g.cy1 - g.cy0;
    if (kw <= 0 || kh <= 0 || g.cx0 < 0 || g.cy0 < 0 || g.cx1 > regs[k].fw || g.cy1 > regs[k].fh || g.cy0 < regs[k].row0) return;
    const uint32_t B = (uint32_t)kw * C;
    const uint32_t cb = paint_col_blocks(B);
    const uint32_t u = unit - regs[k].pre_first;
    const uint32_t band = u / cb, bx = u - band * cb;
    const uint32_t col = bx * PAINT_BAND_COLS + threadIdx.x;
    const int32_t y0 = (int32_t)(band * PAINT_BAND_H), y1 = min(y0 + (int32_t)PAINT_BAND_H, kh);
    if (col >= B || y0 >= kh) return;
    const int32_t r = g.size >> 1;
    const size_t stride = regs[k].stride;
    const uint8_t* base = regs[k].frame + (size_t)(g.cy0 - regs[k].row0) * stride + (size_t)g.cx0 * C + col;   // K's row 0, this byte column
    const uint64_t off = regs[k].scratch_off;
    if (off + 2ull * (uint64_t)kh * B > a.scratch_bytes) return;   // (the host lays the ranges out inside the scratch)
    uint16_t* out = reinterpret_cast<uint16_t*>(a.scratch + off) + col;
    // the band's first window, then slide: add the row entering, subtract the row leaving
    uint32_t sum = 0;
    for (int32_t dy = -r; dy <= r; ++dy) sum += base[(size_t)min(max(y0 + dy, 0), kh - 1) * stride];
    out[(size_t)y0 * B] = (uint16_t)sum;
    for (int32_t y = y0 + 1; y < y1; ++y) {
        sum += base[(size_t)min(y + r, kh - 1) * stride];
        sum -= base[(size_t)max(y - 1 - r, 0) * stride];
        out[(size_t)y * B] = (uint16_t)sum;
    }
}

// A cell is shared by `lanes` lanes of a wave (a power of two: the record's), which walk its bytes and reduce per channel.
__global__ __launch_bounds__(256) void paint_cells(PaintArgs a) {
    kptr<PaintRegionDev> regs = as_k(a.regions);
    const uint32_t unit = blockIdx.x;
    const uint32_t k = paint_region_of<true>(regs, a.n_regions, unit);
    const PaintGeom g = paint_geom(regs + k);
    const uint32_t C = regs[k].channels, L = regs[k].lanes;
    const int32_t kw = g.cx1 - g.cx0, kh = g.cy1 - g.cy0;
    if (kw <= 0 || kh <= 0 || g.size <= 0 || L == 0u || L > 64u || (L & (L - 1u)) != 0u || L < C) return;
    if (g.cx0 < 0 || g.cy0 < 0 || g.cx1 > regs[k].fw || g.cy1 > regs[k].fh || g.cy0 < regs[k].row0) return;
    const uint32_t s = (uint32_t)g.size;
    const uint32_t nx = paint_cells_x((uint32_t)kw, s), ny = paint_cells_x((uint32_t)kh, s);
    const uint64_t ncells = (uint64_t)nx * ny;
    const uint64_t off = regs[k].scratch_off;
    if (off + ncells * C > a.scratch_bytes) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_wave = 64u / L;
    const uint64_t cell = (uint64_t)(unit - regs[k].pre_first) * (PAINT_WAVES * per_wave) + wave * per_wave + lane / L;
    const uint32_t sub = lane & (L - 1u);
    const bool valid = cell < ncells;
    uint32_t x0 = 0, y0 = 0, cw = 0, chh = 0;
    if (valid) {
        const uint32_t j = (uint32_t)(cell / nx), i = (uint32_t)(cell - (uint64_t)j * nx);
        x0 = i * s, y0 = j * s;
        cw = min(s, (uint32_t)kw - x0), chh = min(s, (uint32_t)kh - y0);
    }
    const size_t stride = regs[k].stride;
    const uint8_t* base = regs[k].frame + (size_t)((uint32_t)(g.cy0 - regs[k].row0) + y0) * stride + ((size_t)g.cx0 + x0) * C;
    const uint32_t cwb = cw * C, n_el = cwb * chh;   // (<= 4096 * 4096 * 4: 26 bits)
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (uint32_t e = sub; e < n_el; e += L) {
        const uint32_t row = e / cwb, cb = e - row * cwb;
        const uint32_t c = C == 1u ? 0u : C == 3u ? cb % 3u : cb & 3u;
        const uint32_t v = base[(size_t)row * stride + cb];
        s0 += c == 0u ? v : 0u;
        s1 += c == 1u ? v : 0u;
        s2 += c == 2u ? v : 0u;
        s3 += c == 3u ? v : 0u;
    }
    for (uint32_t d = L >> 1; d != 0u; d >>= 1) {   // (uniform: L is the region's)
        s0 += __shfl_xor(s0, d, 64);
        s1 += __shfl_xor(s1, d, 64);
        s2 += __shfl_xor(s2, d, 64);
        s3 += __shfl_xor(s3, d, 64);
    }
    if (valid && sub < C) {
        const uint32_t n = cw * chh;
        const uint32_t sum = sub == 0u ? s0 : sub == 1u ? s1 : sub == 2u ? s2 : s3;   // <= 4096^2 * 255 + 4096^2 / 2 < 2^32
        a.scratch[off + cell * C + sub] = (uint8_t)((sum + n / 2u) / n);
    }
}

// Every store lies inside K's span of a frame row (checked against the frame's size too); every scratch read lies inside the
// region's range and that inside the scratch (checked).
__global__ __launch_bounds__(256) void paint_apply(PaintArgs a) {
    __shared__ uint32_t prefix[PAINT_WAVES][PAINT_PREFIX_MAX];
    kptr<PaintRegionDev> regs = as_k(a.regions);
    kptr<uint32_t> ovl = as_k(a.overlaps);
    const uint32_t unit = blockIdx.x;
    const uint32_t k = paint_region_of<false>(regs, a.n_regions, unit);
    const PaintGeom g = paint_geom(regs + k);
    const uint32_t C = regs[k].channels, mode = a.mode;
    const bool ellipse = a.ellipse != 0u;
    const int32_t kw = g.cx1 - g.cx0, kh = g.cy1 - g.cy0;
    if (kw <= 0 || kh <= 0 || g.cx0 < 0 || g.cy0 < 0 || g.cx1 > regs[k].fw || g.cy1 > regs[k].fh || g.cy0 < regs[k].row0) return;   // (uniform)
    const uint32_t B = (uint32_t)kw * C;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t bpr = paint_row_blocks(B);
    const uint32_t u = unit - regs[k].unit_first;
    const uint32_t by = u / bpr, bx = u - by * bpr;
    const size_t stride = regs[k].stride;
    uint8_t* k0 = regs[k].frame + (size_t)(g.cy0 - regs[k].row0) * stride + (size_t)g.cx0 * C;   // K's first byte
    const uint64_t off = regs[k].scratch_off;
    const uint32_t n_ovl = regs[k].ovl_count, ovl_first = regs[k].ovl_first;
    const bool ovl_ok = (uint64_t)ovl_first + n_ovl <= a.n_overlaps;
    // what phase 1 left must lie inside the scratch (uniform)
    const uint32_t s = (uint32_t)max(g.size, 1);
    const uint32_t nx = paint_cells_x((uint32_t)kw, s);
    const bool scratch_ok = off + paint_scratch_bytes(mode, (uint32_t)kw, (uint32_t)kh, C, s) <= a.scratch_bytes;
    if ((mode == PAINT_BLUR || mode == PAINT_PIXELATE) && !scratch_ok) return;
    const int32_t rad = g.size >> 1;
    const uint32_t kk2 = (uint32_t)g.size * (uint32_t)g.size;

    for (uint32_t it = 0; it < PAINT_BLOCK_H / PAINT_WAVES; ++it) {   // (the same trip count for every wave: the barriers below)
        const uint32_t r = by * PAINT_BLOCK_H + it * PAINT_WAVES + wave;
        const bool row_ok = r < (uint32_t)kh;
        uint8_t* drow = k0 + (size_t)(row_ok ? r : 0u) * stride;
        const uint32_t m = (uint32_t)((uintptr_t)drow & 3u);
        const int32_t b0 = (int32_t)((bx * PAINT_BLOCK_SLOTS + lane) * 4u) - (int32_t)m;
        const int32_t lo = max(b0, 0), hi = min(b0 + 4, (int32_t)B);
        const int32_t py = g.cy0 + (int32_t)r;

        int32_t q_lo = 0;
        if (mode == PAINT_BLUR) {
            // the wave's bytes [wb0, wb1) of the row -> its pixels [p_lo, p_hi] -> the column sums it needs, [q_lo, q_hi], as
            // inclusive prefix sums per channel in LDS: a lane sums a run of pixels, the runs' totals are scanned across the wave
            const int32_t wb0 = max((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m, 0);
            const int32_t wb1 = min((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m + (int32_t)(PAINT_BLOCK_SLOTS * 4u), (int32_t)B);
            if (row_ok && wb0 < wb1) {
                const int32_t p_lo = wb0 / (int32_t)C, p_hi = (wb1 - 1) / (int32_t)C;
                q_lo = max(p_lo - rad, 0);
                const int32_t q_hi = min(p_hi + rad, kw - 1);
                const int32_t len = q_hi - q_lo + 1;
                if ((uint32_t)len * C <= PAINT_PREFIX_MAX) {   // (always: see PAINT_PREFIX_MAX)
                    const int32_t run = (len + 63) / 64;
                    const int32_t i0 = min((int32_t)lane * run, len), i1 = min(i0 + run, len);
                    const uint16_t* cs = reinterpret_cast<const uint16_t*>(a.scratch + off) + (size_t)r * B;
                    uint32_t t0 = 0, t1 = 0, t2 = 0, t3 = 0;
                    for (int32_t i = i0; i < i1; ++i) {
                        const uint32_t e = (uint32_t)(q_lo + i) * C, o = (uint32_t)i * C;
                        t0 += cs[e];
                        prefix[wave][o] = t0;
                        if (C > 1u) {
                            t1 += cs[e + 1u];
                            t2 += cs[e + 2u];
                            prefix[wave][o + 1u] = t1;
                            prefix[wave][o + 2u] = t2;
                        }
                        if (C > 3u) {
                            t3 += cs[e + 3u];
                            prefix[wave][o + 3u] = t3;
                        }
                    }
                    uint32_t x0 = t0, x1 = t1, x2 = t2, x3 = t3;   // inclusive scan of the runs' totals
                    for (uint32_t d = 1; d < 64u; d <<= 1) {
                        const uint32_t y0 = __shfl_up(x0, d, 64), y1 = __shfl_up(x1, d, 64), y2 = __shfl_up(x2, d, 64), y3 = __shfl_up(x3, d, 64);
                        if (lane >= d) x0 += y0, x1 += y1, x2 += y2, x3 += y3;
                    }
                    x0 -= t0, x1 -= t1, x2 -= t2, x3 -= t3;        // exclusive: what the lanes before this one hold
                    for (int32_t i = i0; i < i1; ++i) {
                        const uint32_t o = (uint32_t)i * C;
                        prefix[wave][o] += x0;
                        if (C > 1u) prefix[wave][o + 1u] += x1, prefix[wave][o + 2u] += x2;
                        if (C > 3u) prefix[wave][o + 3u] += x3;
                    }
                }
            }
            __syncthreads();
        }

        if (row_ok && lo < hi) {
            uint32_t packed = 0, own = 0;   // own: bit q set iff byte q is in the row, painted and owned
            int32_t last_p = -1;
            bool last_own = false;
#pragma unroll
            for (int32_t q = 0; q < 4; ++q) {
                const int32_t b = b0 + q;
                if (b < lo || b >= hi) continue;
                const int32_t p = C == 1u ? b : C == 3u ? b / 3 : b >> 2;   // pixel of K's row, and its channel
                const uint32_t c = (uint32_t)b - (uint32_t)p * C;
                const int32_t px = g.cx0 + p;
                if (p != last_p) {
                    last_p = p;
                    last_own = paint_in_set(g, px, py, mode, ellipse);
                    if (last_own && ovl_ok)
                        for (uint32_t o = 0; o < n_ovl; ++o) {   // (uniform trip count, scalar loads of the later record)
                            const PaintGeom h = paint_geom(regs + min(ovl[ovl_first + o], a.n_regions - 1u));
                            if (paint_in_set(h, px, py, mode, ellipse)) {
                                last_own = false;
                                break;
                            }
                        }
                }
                if (!last_own) continue;
                uint32_t v;
                if (mode == PAINT_BLUR) {
                    // sum over clamp(p + dx, 0, kw - 1), dx = -rad .. rad: the prefix difference plus the replicated ends
                    const int32_t ta = p - rad, tb = p + rad;
                    const int32_t ia = max(ta, 0) - q_lo, ib = min(tb, kw - 1) - q_lo;
                    const uint32_t* P = prefix[wave];
                    uint32_t sum = P[(uint32_t)ib * C + c] - (ia > 0 ? P[(uint32_t)(ia - 1) * C + c] : 0u);
                    if (ta < 0) sum += (uint32_t)(-ta) * P[c];   // (then q_lo = 0: P[c] is column sum 0)
                    if (tb > kw - 1) {                           // (then the staged run ends at kw - 1)
                        const int32_t il = kw - 1 - q_lo;
                        sum += (uint32_t)(tb - (kw - 1)) * (P[(uint32_t)il * C + c] - (il > 0 ? P[(uint32_t)(il - 1) * C + c] : 0u));
                    }
                    v = (sum + kk2 / 2u) / kk2;
                } else if (mode == PAINT_PIXELATE) {
                    const uint32_t cell = (r / s) * nx + (uint32_t)p / s;
                    v = a.scratch[off + (uint64_t)cell * C + c];
                } else {
                    v = (a.color >> (8u * c)) & 0xffu;
                }
                packed |= (v & 0xffu) << (8 * q);
                own |= 1u << q;
            }
            // (K lies inside the frame — checked above —, so bytes [lo, hi) of K's row lie inside the frame's row)
            if (own == 0xfu) {
                *reinterpret_cast<uint32_t*>(drow + b0) = packed;   // (drow + b0) & 3 == 0: b0 = 4 slot - (drow & 3)
            } else {
#pragma unroll
                for (int32_t q = 0; q < 4; ++q)
                    if ((own >> q) & 1u) drow[b0 + q] = (uint8_t)(packed >> (8 * q));
            }
        }
        if (mode == PAINT_BLUR) __syncthreads();   // the next row overwrites the prefix sums
    }
}

int launch_paint(const PaintArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_regions == 0u) return 0;
    hipStream_t st = (hipStream_t)stream_;
    if (a.n_pre_units != 0u) {
        if (a.mode == PAINT_BLUR) hipLaunchKernelGGL(paint_colsum, dim3(a.n_pre_units), dim3(256), 0, st, a);
        else if (a.mode == PAINT_PIXELATE) hipLaunchKernelGGL(paint_cells, dim3(a.n_pre_units), dim3(256), 0, st, a);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(paint_apply, dim3(a.n_units), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace vj
