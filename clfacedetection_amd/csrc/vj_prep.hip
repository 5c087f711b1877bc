// gfx950 kernels of vj_preprocess: the front end of an OpenCV caller's detect call — cvtColor(BGR2GRAY),
// resize(INTER_LINEAR), equalizeHist — for all frames of a call, sizes and channel counts mixed, device in, device out:
//   prep_resize<HIST>  the gray, resized image of every frame into the caller's buffer; HIST: and its histogram
//   (equalize_lut      the frame's 256-byte table from its histogram: vj_equalize.hip, as it is)
//   prep_apply         dst = lut[dst], in place
// The arithmetic is pyramid_levels' (vj_pyramid.hip), integer only: horizontal h = S[i0] * c0 + S[i1] * c1 with
// 11-bit weights, vertical (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, the 2 x 2 mean (sum + 2) >> 2 where the
// source is exactly twice the destination; BGR / BGRA frames go through the ingest conversion (bgr2gray) tap by tap; a frame that
// is not resized is copied through load_gray4.  The taps come from the host (build_taps).
//
// A workgroup is a PREP_BLOCK_W x PREP_BLOCK_H block of one frame's destination (the frame from a binary search of the records' unit
// prefix: uniform, scalar loads — as atlas_pack finds its frame), a wave one row of it at a time, a lane four neighbouring pixels:
// ONE aligned dword store (pyramid_levels stores bytes, one pixel per thread).  Pixels beyond dst_w inside the pitch are stored as 0.
#include <hip/hip_runtime.h>
#include "vj_prep_units.hpp"
#include "vj_devutil.hpp"

// The LDS histograms of prep_resize<true>: equalize_hist's scheme (vj_equalize.hip, measured in DESIGN.md §4.15) — a set per wave,
// a lane counts into copy (lane % PREP_HIST_COPIES), a bin's copies side by side, and a wave whose 256 pixels all have one value adds
// them with ONE atomic.
#ifndef PREP_HIST_COPIES
#define PREP_HIST_COPIES 4
#endif
static_assert(PREP_HIST_COPIES >= 1 && PREP_HIST_COPIES <= 16 && (PREP_HIST_COPIES & (PREP_HIST_COPIES - 1)) == 0, "copies per wave: a power of two up to 16");

namespace vj {

namespace {
constexpr uint32_t PREP_WAVES = 4;   // waves per workgroup

// the last frame whose first unit is <= unit; uniform, scalar loads
__device__ __forceinline__ uint32_t prep_frame_of(kptr<PrepFrameDev> frames, uint32_t n_frames, uint32_t unit) {
    uint32_t lo = 0, hi = n_frames;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (frames[mid].unit_first <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t prep_px(const uint8_t* row, uint32_t x, uint32_t ch) {
    if (ch <= 1u) return (uint32_t)row[x];
    const uint8_t* p = row + (size_t)x * ch;
    return bgr2gray(p[0], p[1], p[2]);
}

// Eight neighbouring gray pixels x .. x + 7 of a row (x + 8 <= the row's width), g[k] = pixel x + k: dword loads where the first
// one's address is a multiple of 4 (2 / 6 / 8 of them for gray / BGR / BGRA), else byte loads
__device__ __forceinline__ void prep_load8(const uint8_t* row, uint32_t x, uint32_t ch, uint32_t g[8]) {
    const uint8_t* p = row + (size_t)x * ch;
    if (((uintptr_t)p & 3u) == 0u) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
        if (ch <= 1u) {
            const uint32_t w0 = w[0], w1 = w[1];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                g[k] = (w0 >> (8u * k)) & 0xffu;
                g[4u + k] = (w1 >> (8u * k)) & 0xffu;
            }
        } else if (ch == 3u) {
#pragma unroll
            for (uint32_t q = 0; q < 2u; ++q) {   // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
                const uint32_t w0 = w[3u * q], w1 = w[3u * q + 1u], w2 = w[3u * q + 2u];
                g[4u * q] = bgr2gray(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu);
                g[4u * q + 1u] = bgr2gray(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu);
                g[4u * q + 2u] = bgr2gray((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu);
                g[4u * q + 3u] = bgr2gray((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24);
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) g[k] = bgr2gray(w[k] & 0xffu, (w[k] >> 8) & 0xffu, (w[k] >> 16) & 0xffu);
        }
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) g[k] = prep_px(row, x + k, ch);
}

struct PrepTap4 { uint4 a, b; };   // four PyrTaps: i0 | i1 << 16, c0 | c1 << 16 each

// The four pixels dx .. dx + 3 of destination row dy of frame f, packed; pixels beyond dw are 0.  dx < dw, dx a multiple of 4.
__device__ __forceinline__ uint32_t prep_row4(kptr<PrepFrameDev> frames, uint32_t f, const PyrTap* taps, uint32_t dx, uint32_t dy) {
    const uint32_t sw = frames[f].sw, sh = frames[f].sh, dw = frames[f].dw, ch = frames[f].channels, mode = frames[f].mode;
    const uint8_t* src = frames[f].src;
    const size_t stride = frames[f].stride;
    const uint32_t n = min(4u, dw - dx);
    if (mode == PREP_COPY) return load_gray4(src + (size_t)dy * stride, dx, sw, ch);
    uint32_t packed = 0;
    if (mode == PREP_AREA) {   // sw = 2 dw, sh = 2 dh: source columns 2 dx .. 2 dx + 7 of rows 2 dy, 2 dy + 1
        const uint32_t y0 = min(2u * dy, sh - 1u), y1 = min(2u * dy + 1u, sh - 1u);
        const uint8_t* r0 = src + (size_t)y0 * stride;
        const uint8_t* r1 = src + (size_t)y1 * stride;
        if (n == 4u && 2u * dx + 8u <= sw) {
            uint32_t g0[8], g1[8];
            prep_load8(r0, 2u * dx, ch, g0);
            prep_load8(r1, 2u * dx, ch, g1);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) packed |= ((g0[2u * k] + g0[2u * k + 1u] + g1[2u * k] + g1[2u * k + 1u] + 2u) >> 2) << (8u * k);
            return packed;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (k >= n) break;
            const uint32_t x0 = min(2u * (dx + k), sw - 1u), x1 = min(2u * (dx + k) + 1u, sw - 1u);
            packed |= ((prep_px(r0, x0, ch) + prep_px(r0, x1, ch) + prep_px(r1, x0, ch) + prep_px(r1, x1, ch) + 2u) >> 2) << (8u * k);
        }
        return packed;
    }
    // (the row's tap is uniform: scalar loads; the columns' runs are padded to 4 taps and start at a multiple of 4: two 16-byte loads)
    kptr<uint32_t> taps_k = as_k(reinterpret_cast<const uint32_t*>(taps));
    const uint32_t yt = frames[f].ytab + dy;
    const uint32_t wy0 = taps_k[2u * yt], wy1 = taps_k[2u * yt + 1u];
    const uint32_t y0 = min(wy0 & 0xffffu, sh - 1u), y1 = min(wy0 >> 16, sh - 1u);
    const int32_t b0 = (int32_t)(int16_t)(wy1 & 0xffffu), b1 = (int32_t)(int16_t)(wy1 >> 16);
    const uint8_t* r0 = src + (size_t)y0 * stride;
    const uint8_t* r1 = src + (size_t)y1 * stride;
    const uint4* tp = reinterpret_cast<const uint4*>(taps + frames[f].xtab + dx);
    const uint4 ta = tp[0], tb = tp[1];
    const uint32_t ti[4] = {ta.x, ta.z, tb.x, tb.z}, tc[4] = {ta.y, ta.w, tb.y, tb.w};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t x0 = min(ti[k] & 0xffffu, sw - 1u), x1 = min(ti[k] >> 16, sw - 1u);
        const int32_t c0 = (int32_t)(int16_t)(tc[k] & 0xffffu), c1 = (int32_t)(int16_t)(tc[k] >> 16);
        const int32_t s00 = (int32_t)prep_px(r0, x0, ch), s01 = (int32_t)prep_px(r0, x1, ch);
        const int32_t s10 = (int32_t)prep_px(r1, x0, ch), s11 = (int32_t)prep_px(r1, x1, ch);
        const int32_t h0 = s00 * c0 + s01 * c1, h1 = s10 * c0 + s11 * c1;
        const int32_t v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
        if (k < n) packed |= ((uint32_t)v & 0xffu) << (8u * k);
    }
    return packed;
}

// four packed pixels of which the first n count, into the wave's LDS histograms (equalize_hist's scheme); the whole wave calls it
__device__ __forceinline__ void prep_count4(uint32_t* wave_sub, uint32_t lane, uint32_t v, uint32_t n) {
    uint32_t* mine = wave_sub + (lane & (PREP_HIST_COPIES - 1u));
    const bool flat = n == 4u && v == (v & 0xffu) * 0x01010101u;
    // lane 0 holds pixels in every block of a row (its first column lies inside the frame): the wave's pixels are all its first one's
    const uint32_t v0 = __builtin_amdgcn_readfirstlane(v);
    const unsigned long long live = __ballot(n != 0u);   // (taken here: inside the branch below only lane 0 would vote)
    if (__ballot(flat && v == v0) == live) {
        if (lane == 0u) atomicAdd(&wave_sub[(v0 & 0xffu) * PREP_HIST_COPIES], 4u * (uint32_t)__popcll(live));
        return;
    }
    if (flat) {
        atomicAdd(&mine[(v & 0xffu) * PREP_HIST_COPIES], 4u);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
            if (c < n) atomicAdd(&mine[((v >> (8u * c)) & 0xffu) * PREP_HIST_COPIES], 1u);
    }
}
}  // namespace

// HIST: the four pixels a lane has just computed are counted into the workgroup's LDS histograms, lanes and bytes beyond dst_w masked
// out, and the counts merged into the frame's global u32[256] with one atomic per non-empty bin: the resized image is never read
// back for its histogram.  Every store lies inside the frame's image and that inside the buffer: dx < dw, so dx + 4 <= pitch.
template <bool HIST>
__global__ __launch_bounds__(256) void prep_resize(PrepArgs a) {
    __shared__ uint32_t sub[HIST ? PREP_WAVES : 1u][HIST ? 256 * PREP_HIST_COPIES : 1];
    kptr<PrepFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    const uint32_t f = prep_frame_of(frames, a.n_frames, unit);
    const uint32_t dw = frames[f].dw, dh = frames[f].dh, pitch = frames[f].pitch;
    const uint64_t off = frames[f].dst_off;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (HIST) {
        for (uint32_t i = threadIdx.x; i < PREP_WAVES * 256u * PREP_HIST_COPIES; i += 256u) (&sub[0][0])[i] = 0u;
        __syncthreads();
    }
    const uint32_t blocks_per_row = (dw + PREP_BLOCK_W - 1u) / PREP_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * PREP_BLOCK_W + lane * 4u;
    const uint32_t y1 = min((by + 1u) * PREP_BLOCK_H, dh);
    // the image inside the buffer (the host lays it out so; a store never leaves the buffer)
    const bool inside = (pitch & 3u) == 0u && (off & 3u) == 0u && pitch >= dw && off + (uint64_t)pitch * dh <= a.dst_bytes;
    for (uint32_t dy = by * PREP_BLOCK_H + wave; dy < y1; dy += PREP_WAVES) {   // (uniform: every lane of the wave walks the rows)
        const bool live = inside && dx < dw;
        const uint32_t v = live ? prep_row4(frames, f, a.taps, dx, dy) : 0u;
        if (live) *reinterpret_cast<uint32_t*>(a.dst + off + (size_t)dy * pitch + dx) = v;
        if (HIST) prep_count4(&sub[wave][0], lane, v, live ? min(4u, dw - dx) : 0u);
    }
    if (HIST) {
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < PREP_WAVES; ++k)
#pragma unroll
            for (uint32_t c = 0; c < PREP_HIST_COPIES; ++c) sum += sub[k][threadIdx.x * PREP_HIST_COPIES + c];
        if (sum) atomicAdd(&a.hist[(size_t)frames[f].hist_slot * 256u + threadIdx.x], sum);
    }
}

// -DPREP_UNFUSED_HIST (tests/measure_preprocess.py: what fusing the histogram into prep_resize buys): the histograms from the images
// prep_resize<false> has written, same blocks, same counting.
__global__ __launch_bounds__(256) void prep_hist(PrepArgs a) {
    __shared__ uint32_t sub[PREP_WAVES][256 * PREP_HIST_COPIES];
    kptr<PrepFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    const uint32_t f = prep_frame_of(frames, a.n_frames, unit);
    const uint32_t dw = frames[f].dw, dh = frames[f].dh, pitch = frames[f].pitch;
    const uint64_t off = frames[f].dst_off;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < PREP_WAVES * 256u * PREP_HIST_COPIES; i += 256u) (&sub[0][0])[i] = 0u;
    __syncthreads();
    const uint32_t blocks_per_row = (dw + PREP_BLOCK_W - 1u) / PREP_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * PREP_BLOCK_W + lane * 4u;
    const uint32_t y1 = min((by + 1u) * PREP_BLOCK_H, dh);
    const bool inside = (pitch & 3u) == 0u && (off & 3u) == 0u && pitch >= dw && off + (uint64_t)pitch * dh <= a.dst_bytes;
    for (uint32_t dy = by * PREP_BLOCK_H + wave; dy < y1; dy += PREP_WAVES) {
        const bool live = inside && dx < dw;
        const uint32_t v = live ? *reinterpret_cast<const uint32_t*>(a.dst + off + (size_t)dy * pitch + dx) : 0u;
        prep_count4(&sub[wave][0], lane, v, live ? min(4u, dw - dx) : 0u);
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < PREP_WAVES; ++k)
#pragma unroll
        for (uint32_t c = 0; c < PREP_HIST_COPIES; ++c) sum += sub[k][threadIdx.x * PREP_HIST_COPIES + c];
    if (sum) atomicAdd(&a.hist[(size_t)frames[f].hist_slot * 256u + threadIdx.x], sum);
}

// Applies every frame's table IN PLACE on the caller's buffer, per record — frames differ in size, which equalize_apply's destination
// (an equal batch) cannot express.  The same blocks; the table staged in LDS, one byte per thread, as equalize_apply stages it; dword
// loads and stores.  Pad columns hold 0 and stay 0: lut[0] is 0 in every table equalize_lut writes.
__global__ __launch_bounds__(256) void prep_apply(PrepArgs a) {
    __shared__ uint8_t lut[256];
    kptr<PrepFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    const uint32_t f = prep_frame_of(frames, a.n_frames, unit);
    lut[threadIdx.x] = a.lut[(size_t)frames[f].hist_slot * 256u + threadIdx.x];
    __syncthreads();
    const uint32_t dw = frames[f].dw, dh = frames[f].dh, pitch = frames[f].pitch;
    const uint64_t off = frames[f].dst_off;
    const uint32_t blocks_per_row = (dw + PREP_BLOCK_W - 1u) / PREP_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * PREP_BLOCK_W + (threadIdx.x & 63u) * 4u;
    const uint32_t y1 = min((by + 1u) * PREP_BLOCK_H, dh);
    if (dx >= dw || (pitch & 3u) != 0u || (off & 3u) != 0u || pitch < dw || off + (uint64_t)pitch * dh > a.dst_bytes) return;
    for (uint32_t dy = by * PREP_BLOCK_H + (threadIdx.x >> 6); dy < y1; dy += PREP_WAVES) {
        uint32_t* p = reinterpret_cast<uint32_t*>(a.dst + off + (size_t)dy * pitch + dx);
        *p = lut_gray4(lut, *p);
    }
}

int launch_prep_resize(const PrepArgs& a, bool hist, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    if (hist) hipLaunchKernelGGL(prep_resize<true>, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL(prep_resize<false>, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_prep_hist(const PrepArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    hipLaunchKernelGGL(prep_hist, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_prep_apply(const PrepArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    hipLaunchKernelGGL(prep_apply, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
