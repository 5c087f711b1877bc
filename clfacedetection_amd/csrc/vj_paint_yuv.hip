// gfx950 kernels of vj_paint_yuv: the rectangles of a call painted into 4:2:0 frames IN PLACE, plane by plane.  A
// record is one (region, plane); a plane is an image of 1 or 2 interleaved components (Y, I420's U and V; the pair plane of NV12 /
// NV21), so a pixel is 1 or 2 bytes and nothing here divides by a channel count.  The Y records and the chroma records of a slice
// share the grids of ONE phase-1 launch and ONE phase-2 launch, and as in vj_paint.hip NO LAUNCH BOTH READS A PLANE AND WRITES ONE:
//   paint_yuv_colsum   BLUR: per byte column of the record's rectangle the vertical kk-row sums, rows clamped to it, 16-bit values
//   paint_yuv_cells    PIXELATE: the rounded mean of every cell, per component, one byte each
//   paint_yuv_apply    every mode: the value of every painted byte, stored iff its sample is in the region's painted set — P_k on
//                      the Y plane, "any of the four luma pixels in P_k" on chroma — and in no LATER region's of the same plane.
// paint_yuv_apply decomposes as paint_apply does (a workgroup a block of rows x four-byte slots of one record, a wave one row at a
// time, a lane one slot of the PLANE row).  What it does differently: for rectangles the painted set of a row is at most two
// intervals of samples, found ONCE per row and per later region from wave-uniform values (the 64-bit arithmetic is there), and a
// lane tests its samples with 32-bit compares; only the ellipse evaluates the shape per sample.  A pair plane may lie at any address
// mod 4: a slot whose four bytes are all in the row, painted and owned is ONE aligned dword store, every other slot is stored byte
// by byte, owned bytes only — never an unaligned dword, never a read-modify-write of a byte another workgroup owns.
#include <hip/hip_runtime.h>
#include "vj_paint_yuv_units.hpp"
#include "vj_devutil.hpp"

namespace vj {

namespace {

// the last record whose first unit (apply or phase 1) is <= unit; uniform, scalar loads
template <bool PRE>
__device__ __forceinline__ uint32_t paint_yuv_rec_of(kptr<PaintYuvRec> recs, uint32_t n, uint32_t unit) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((PRE ? recs[mid].pre_first : recs[mid].unit_first) <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The record's rectangle, checked (uniform): not empty, inside the plane, inside the rows `plane` holds, 1 or 2 components
struct PaintYuvRect { int32_t x0, y0, w, h; uint32_t C; bool ok; };
__device__ __forceinline__ PaintYuvRect paint_yuv_rect(kptr<PaintYuvRec> r) {
    PaintYuvRect q;
    q.x0 = r->kx0, q.y0 = r->ky0, q.w = r->kx1 - r->kx0, q.h = r->ky1 - r->ky0;
    q.C = r->comps;
    q.ok = q.w > 0 && q.h > 0 && q.x0 >= 0 && q.y0 >= 0 && r->kx1 <= r->pw && r->ky1 <= r->ph && q.y0 >= r->row0 && r->row0 >= 0 &&
           (q.C == 1u || q.C == 2u) && (uint64_t)(uint32_t)r->pw * q.C <= r->stride;
    return q;
}

}  // namespace

// Every load lies inside the record's rectangle, which lies inside the plane (checked); every store lies inside the scratch range
// the host gave the record, and that inside the scratch (checked).
__global__ __launch_bounds__(256) void paint_yuv_colsum(PaintYuvArgs a) {
    kptr<PaintYuvRec> recs = as_k(a.recs);
    const uint32_t unit = blockIdx.x;
    if (a.n_recs == 0u) return;
    const uint32_t k = paint_yuv_rec_of<true>(recs, a.n_recs, unit);
    const PaintYuvRect q = paint_yuv_rect(recs + k);
    const int32_t kk = recs[k].psize;
    if (!q.ok || kk < 1 || kk > PAINT_MAX_KK || unit < recs[k].pre_first) return;
    const uint32_t B = (uint32_t)q.w * q.C;
    const uint32_t cb = paint_col_blocks(B);
    const uint32_t u = unit - recs[k].pre_first;
    const uint32_t band = u / cb, bx = u - band * cb;
    const uint32_t col = bx * PAINT_BAND_COLS + threadIdx.x;
    const int32_t kh = q.h;
    const int32_t y0 = (int32_t)(band * PAINT_BAND_H), y1 = min(y0 + (int32_t)PAINT_BAND_H, kh);
    if (col >= B || y0 >= kh) return;
    const int32_t r = kk >> 1;
    const size_t stride = recs[k].stride;
    const uint8_t* base = recs[k].plane + (size_t)(q.y0 - recs[k].row0) * stride + (size_t)q.x0 * q.C + col;   // the rectangle's row 0, this byte column
    const uint64_t off = recs[k].scratch_off;
    if (off + 2ull * (uint64_t)kh * B > a.scratch_bytes) return;
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

// A cell is shared by `lanes` lanes of a wave (a power of two: the record's), which walk its bytes and reduce per component.
__global__ __launch_bounds__(256) void paint_yuv_cells(PaintYuvArgs a) {
    kptr<PaintYuvRec> recs = as_k(a.recs);
    const uint32_t unit = blockIdx.x;
    if (a.n_recs == 0u) return;
    const uint32_t k = paint_yuv_rec_of<true>(recs, a.n_recs, unit);
    const PaintYuvRect q = paint_yuv_rect(recs + k);
    const uint32_t C = q.C, L = recs[k].lanes;
    const int32_t size = recs[k].psize;
    if (!q.ok || size <= 0 || size > PAINT_MAX_CELL || L == 0u || L > 64u || (L & (L - 1u)) != 0u || L < C || unit < recs[k].pre_first) return;
    const int32_t kw = q.w, kh = q.h;
    const uint32_t s = (uint32_t)size;
    const uint32_t nx = paint_cells_x((uint32_t)kw, s), ny = paint_cells_x((uint32_t)kh, s);
    const uint64_t ncells = (uint64_t)nx * ny;
    const uint64_t off = recs[k].scratch_off;
    if (off + ncells * C > a.scratch_bytes) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per_wave = 64u / L;
    const uint64_t cell = (uint64_t)(unit - recs[k].pre_first) * (PAINT_WAVES * per_wave) + wave * per_wave + lane / L;
    const uint32_t sub = lane & (L - 1u);
    const bool valid = cell < ncells;
    uint32_t x0 = 0, y0 = 0, cw = 0, chh = 0;
    if (valid) {
        const uint32_t j = (uint32_t)(cell / nx), i = (uint32_t)(cell - (uint64_t)j * nx);
        x0 = i * s, y0 = j * s;
        cw = min(s, (uint32_t)kw - x0), chh = min(s, (uint32_t)kh - y0);
    }
    const size_t stride = recs[k].stride;
    const uint8_t* base = recs[k].plane + (size_t)((uint32_t)(q.y0 - recs[k].row0) + y0) * stride + ((size_t)q.x0 + x0) * C;
    const uint32_t cwb = cw * C, n_el = cwb * chh;   // (<= 4096 * 4096 * 2: 25 bits)
    uint32_t s0 = 0, s1 = 0;
    for (uint32_t e = sub; e < n_el; e += L) {
        const uint32_t row = e / cwb, cbyte = e - row * cwb;
        const uint32_t v = base[(size_t)row * stride + cbyte];
        const bool second = (cbyte & (C - 1u)) != 0u;
        s0 += second ? 0u : v;
        s1 += second ? v : 0u;
    }
    for (uint32_t d = L >> 1; d != 0u; d >>= 1) {   // (uniform: L is the record's)
        s0 += __shfl_xor(s0, d, 64);
        s1 += __shfl_xor(s1, d, 64);
    }
    if (valid && sub < C) {
        const uint32_t n = cw * chh;
        const uint32_t sum = sub == 0u ? s0 : s1;   // <= 4096^2 * 255 + 4096^2 / 2 < 2^32
        a.scratch[off + cell * C + sub] = (uint8_t)((sum + n / 2u) / n);
    }
}

// Every store lies inside the rectangle's span of a plane row (checked against the plane's size too); every scratch read lies inside
// the record's range and that inside the scratch (checked).
__global__ __launch_bounds__(256) void paint_yuv_apply(PaintYuvArgs a) {
    __shared__ uint32_t prefix[PAINT_WAVES][PAINT_YUV_PREFIX_MAX];
    kptr<PaintYuvRec> recs = as_k(a.recs);
    kptr<uint32_t> ovl = as_k(a.overlaps);
    const uint32_t unit = blockIdx.x;
    if (a.n_recs == 0u) return;
    const uint32_t k = paint_yuv_rec_of<false>(recs, a.n_recs, unit);
    const PaintGeom g = paint_geom(recs + k);
    const PaintYuvRect R = paint_yuv_rect(recs + k);
    const uint32_t C = R.C, sh = C - 1u, mode = a.mode, sub = recs[k].sub;
    const bool ellipse = a.ellipse != 0u;
    if (!R.ok || unit < recs[k].unit_first) return;   // (uniform)
    const int32_t kw = R.w, kh = R.h;
    const uint32_t B = (uint32_t)kw * C;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t bpr = paint_row_blocks(B);
    const uint32_t u = unit - recs[k].unit_first;
    const uint32_t by = u / bpr, bx = u - by * bpr;
    const size_t stride = recs[k].stride;
    uint8_t* k0 = recs[k].plane + (size_t)(R.y0 - recs[k].row0) * stride + (size_t)R.x0 * C;   // the rectangle's first byte
    const uint64_t off = recs[k].scratch_off;
    const uint32_t n_ovl = recs[k].ovl_count, ovl_first = recs[k].ovl_first;
    const bool ovl_ok = (uint64_t)ovl_first + n_ovl <= a.n_overlaps;
    // what phase 1 left must lie inside the scratch (uniform)
    const int32_t size = recs[k].psize;
    const uint32_t s = (uint32_t)max(size, 1);
    const uint32_t nx = paint_cells_x((uint32_t)kw, s);
    const bool scratch_ok = off + paint_scratch_bytes(mode, (uint32_t)kw, (uint32_t)kh, C, s) <= a.scratch_bytes;
    if ((mode == PAINT_BLUR || mode == PAINT_PIXELATE) && (!scratch_ok || size < 1)) return;
    const int32_t rad = size >> 1;
    const uint32_t kk2 = (uint32_t)size * (uint32_t)size;
    const uint32_t color = recs[k].color;

    for (uint32_t it = 0; it < PAINT_BLOCK_H / PAINT_WAVES; ++it) {   // (the same trip count for every wave: the barriers below)
        const uint32_t r = by * PAINT_BLOCK_H + it * PAINT_WAVES + wave;
        const bool row_ok = r < (uint32_t)kh;
        uint8_t* drow = k0 + (size_t)(row_ok ? r : 0u) * stride;
        const uint32_t m = (uint32_t)((uintptr_t)drow & 3u);
        const int32_t b0 = (int32_t)((bx * PAINT_BLOCK_SLOTS + lane) * 4u) - (int32_t)m;
        const int32_t lo = max(b0, 0), hi = min(b0 + 4, (int32_t)B);
        const int32_t py = R.y0 + (int32_t)r;   // the plane row

        int32_t q_lo = 0;
        if (mode == PAINT_BLUR) {
            // the wave's bytes [wb0, wb1) of the row -> its samples [p_lo, p_hi] -> the column sums it needs, [q_lo, q_hi], as
            // inclusive prefix sums per component in LDS: a lane sums a run of samples, the runs' totals are scanned across the wave
            const int32_t wb0 = max((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m, 0);
            const int32_t wb1 = min((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m + (int32_t)(PAINT_BLOCK_SLOTS * 4u), (int32_t)B);
            if (row_ok && wb0 < wb1) {
                const int32_t p_lo = wb0 >> sh, p_hi = (wb1 - 1) >> sh;
                q_lo = max(p_lo - rad, 0);
                const int32_t q_hi = min(p_hi + rad, kw - 1);
                const int32_t len = q_hi - q_lo + 1;
                if (((uint32_t)len << sh) <= PAINT_YUV_PREFIX_MAX) {   // (always: see PAINT_YUV_PREFIX_MAX)
                    const int32_t run = (len + 63) / 64;
                    const int32_t i0 = min((int32_t)lane * run, len), i1 = min(i0 + run, len);
                    const uint16_t* cs = reinterpret_cast<const uint16_t*>(a.scratch + off) + (size_t)r * B;
                    uint32_t t0 = 0, t1 = 0;
                    for (int32_t i = i0; i < i1; ++i) {
                        const uint32_t e = (uint32_t)(q_lo + i) << sh, o = (uint32_t)i << sh;
                        t0 += cs[e];
                        prefix[wave][o] = t0;
                        if (C > 1u) {
                            t1 += cs[e + 1u];
                            prefix[wave][o + 1u] = t1;
                        }
                    }
                    uint32_t x0 = t0, x1 = t1;   // inclusive scan of the runs' totals
                    for (uint32_t d = 1; d < 64u; d <<= 1) {
                        const uint32_t y0 = __shfl_up(x0, d, 64), y1 = __shfl_up(x1, d, 64);
                        if (lane >= d) x0 += y0, x1 += y1;
                    }
                    x0 -= t0, x1 -= t1;          // exclusive: what the lanes before this one hold
                    for (int32_t i = i0; i < i1; ++i) {
                        const uint32_t o = (uint32_t)i << sh;
                        prefix[wave][o] += x0;
                        if (C > 1u) prefix[wave][o + 1u] += x1;
                    }
                }
            }
            __syncthreads();
        }

        if (row_ok && lo < hi) {
            // the slot's samples ps .. pl of the rectangle's row (at most four): bit j of `mine` set iff sample ps + j is painted and owned
            const int32_t ps = lo >> sh, pl = (hi - 1) >> sh;
            uint32_t mine = 0;
            if (!ellipse) {
                // one evaluation of the shape per row, on uniform values; the lane compares in 32 bits
                const PaintRowSet rs = paint_yuv_row_set(g, sub, mode, py);
#pragma unroll
                for (int32_t j = 0; j < 4; ++j)
                    if (ps + j <= pl && paint_yuv_in_row(rs, R.x0 + ps + j)) mine |= 1u << j;
                if (ovl_ok)
                    for (uint32_t o = 0; o < n_ovl; ++o) {   // (uniform trip count, scalar loads of the later record)
                        const uint32_t hk = min(ovl[ovl_first + o], a.n_recs - 1u);
                        const PaintRowSet hs = paint_yuv_row_set(paint_geom(recs + hk), sub, mode, py);
#pragma unroll
                        for (int32_t j = 0; j < 4; ++j)
                            if (paint_yuv_in_row(hs, R.x0 + ps + j)) mine &= ~(1u << j);
                    }
            } else {
#pragma unroll
                for (int32_t j = 0; j < 4; ++j) {
                    if (ps + j > pl) continue;
                    const int32_t px = R.x0 + ps + j;
                    bool own = paint_yuv_in_set(g, sub, px, py, mode, true);
                    if (own && ovl_ok)
                        for (uint32_t o = 0; o < n_ovl; ++o) {
                            const uint32_t hk = min(ovl[ovl_first + o], a.n_recs - 1u);
                            if (paint_yuv_in_set(paint_geom(recs + hk), sub, px, py, mode, true)) {
                                own = false;
                                break;
                            }
                        }
                    if (own) mine |= 1u << j;
                }
            }
            uint32_t packed = 0, own = 0;   // own: bit q set iff byte q is in the row, painted and owned
            if (mine != 0u) {
#pragma unroll
                for (int32_t q = 0; q < 4; ++q) {
                    const int32_t b = b0 + q;
                    if (b < lo || b >= hi) continue;
                    const int32_t p = b >> sh;                          // sample of the rectangle's row, and its component
                    const uint32_t c = (uint32_t)b & sh;
                    if (((mine >> (p - ps)) & 1u) == 0u) continue;
                    uint32_t v;
                    if (mode == PAINT_BLUR) {
                        // sum over clamp(p + dx, 0, kw - 1), dx = -rad .. rad: the prefix difference plus the replicated ends
                        const int32_t ta = p - rad, tb = p + rad;
                        const int32_t ia = max(ta, 0) - q_lo, ib = min(tb, kw - 1) - q_lo;
                        const uint32_t* P = prefix[wave];
                        uint32_t sum = P[((uint32_t)ib << sh) + c] - (ia > 0 ? P[((uint32_t)(ia - 1) << sh) + c] : 0u);
                        if (ta < 0) sum += (uint32_t)(-ta) * P[c];   // (then q_lo = 0: P[c] is column sum 0)
                        if (tb > kw - 1) {                           // (then the staged run ends at kw - 1)
                            const int32_t il = kw - 1 - q_lo;
                            sum += (uint32_t)(tb - (kw - 1)) * (P[((uint32_t)il << sh) + c] - (il > 0 ? P[((uint32_t)(il - 1) << sh) + c] : 0u));
                        }
                        v = (sum + kk2 / 2u) / kk2;
                    } else if (mode == PAINT_PIXELATE) {
                        const uint32_t cell = (r / s) * nx + (uint32_t)p / s;
                        v = a.scratch[off + (((uint64_t)cell) << sh) + c];
                    } else {
                        v = (color >> (8u * c)) & 0xffu;
                    }
                    packed |= (v & 0xffu) << (8 * q);
                    own |= 1u << q;
                }
            }
            // (the rectangle lies inside the plane — checked above —, so bytes [lo, hi) of its row lie inside the plane's row)
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

int launch_paint_yuv(const PaintYuvArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_recs == 0u) return 0;
    hipStream_t st = (hipStream_t)stream_;
    if (a.n_pre_units != 0u) {
        if (a.mode == PAINT_BLUR) hipLaunchKernelGGL(paint_yuv_colsum, dim3(a.n_pre_units), dim3(256), 0, st, a);
        else if (a.mode == PAINT_PIXELATE) hipLaunchKernelGGL(paint_yuv_cells, dim3(a.n_pre_units), dim3(256), 0, st, a);
        const int rc = (int)hipGetLastError();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(paint_yuv_apply, dim3(a.n_units), dim3(256), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace vj
