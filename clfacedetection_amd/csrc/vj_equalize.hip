// gfx950 kernels of VJ_FLAG_EQUALIZE_HIST and vj_equalize_hist: cv::equalizeHist for 8-bit single-channel images
// (OpenCV imgproc/histogram.cpp, 2.4.4 .. 4.x) on the gray image vj_grayscale returns, every frame on its own.  Three launches serve
// a whole sub-batch, each over ONE table of frame records (AtlasFrameDev: a batch of equal frames and the frames of an atlas alike):
//   equalize_hist    hist[f][v] = pixels of value v in frame f
//   equalize_lut     the frame's 256-byte table from its histogram
//   equalize_apply   dst = lut[src], into a gray batch at the device's 4-byte pitch (an atlas applies the table in atlas_pack<true>)
// Integer counts, one f32 division and one f32 multiplication per table entry: the result does not depend on the order of anything.
#include <hip/hip_runtime.h>
#include "vj_atlas_units.hpp"
#include "vj_devutil.hpp"

// Privatisation of the LDS histograms (measured: DESIGN.md §4.15, tests/measure_equalize.py).  Every wave counts into copies of its
// own, a lane into copy (lane % EQ_HIST_COPIES), a bin's copies side by side (neighbouring banks); EQ_HIST_BALLOT: a wave whose 256
// pixels all have one value adds them with ONE atomic — the constant or saturated areas in which all 64 lanes would hit one address.
// 64 x 1080p, stage time noise / constant / smooth: 1 copy without the ballot 0.228 / 0.272 / 0.233 ms (the constant batch pays the
// serialised adds), 1 copy with it 0.238 / 0.219 / 0.236, 4 copies without 0.228 / 0.221 / 0.233, 4 copies with it — the default, both
// remedies — 0.232 / 0.227 / 0.239, all three within the 0.01 ms a process differs from the next; 8 and 16 copies lose 0.05 and 0.14 ms.
#ifndef EQ_HIST_COPIES
#define EQ_HIST_COPIES 4
#endif
#ifndef EQ_HIST_BALLOT
#define EQ_HIST_BALLOT 1
#endif
static_assert(EQ_HIST_COPIES >= 1 && EQ_HIST_COPIES <= 16 && (EQ_HIST_COPIES & (EQ_HIST_COPIES - 1)) == 0, "copies per wave: a power of two up to 16");

namespace vj {

namespace {
constexpr uint32_t EQ_WAVES = 4;   // waves per workgroup of all three kernels

// the last frame whose first unit (HIST: hist_first, else unit_first) is <= unit; uniform, scalar loads — as atlas_pack finds its frame
template <bool HIST>
__device__ __forceinline__ uint32_t frame_of(kptr<AtlasFrameDev> frames, uint32_t n_frames, uint32_t unit) {
    uint32_t lo = 0, hi = n_frames;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((HIST ? frames[mid].hist_first : frames[mid].unit_first) <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}
}  // namespace

// A workgroup counts EQ_HIST_ROWS whole rows of one frame, wave k rows k, k + 4, ...; a lane takes four pixels of every 256 of the row
// through load_gray4 (so BGR / BGRA frames count the bytes vj_grayscale gives) and counts only those inside the row: the pixels a
// row's last dword holds beyond w, and the pad columns, are never counted.  Then one global atomic per non-empty bin.
__global__ __launch_bounds__(256) void equalize_hist(EqualizeArgs a) {
    __shared__ uint32_t sub[EQ_WAVES][256 * EQ_HIST_COPIES];
    kptr<AtlasFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    const uint32_t f = frame_of<true>(frames, a.n_frames, unit);
    const uint32_t w = frames[f].w, h = frames[f].h, ch = frames[f].channels;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < EQ_WAVES * 256u * EQ_HIST_COPIES; i += 256u) (&sub[0][0])[i] = 0u;
    __syncthreads();
    uint32_t* mine = &sub[wave][lane & (EQ_HIST_COPIES - 1u)];
    const uint32_t y0 = (unit - frames[f].hist_first) * EQ_HIST_ROWS;
    const uint32_t y1 = min(y0 + EQ_HIST_ROWS, h);
    for (uint32_t y = y0 + wave; y < y1; y += EQ_WAVES) {
        const uint8_t* row = frames[f].src + (size_t)y * frames[f].stride;
        for (uint32_t xb = 0; xb < w; xb += 256u) {   // (uniform: every lane of the wave walks the row's chunks)
            const uint32_t x = xb + lane * 4u;
            const uint32_t n = x < w ? min(4u, w - x) : 0u;
            const uint32_t v = n ? load_gray4(row, x, w, ch) : 0u;
            const bool flat = n == 4u && v == (v & 0xffu) * 0x01010101u;
#if EQ_HIST_BALLOT
            // lane 0 holds pixels in every chunk (xb < w): the wave's pixels are all its first one's
            const uint32_t v0 = __builtin_amdgcn_readfirstlane(v);
            const unsigned long long live = __ballot(n != 0u);   // (taken here: inside the branch below only lane 0 would vote)
            if (__ballot(flat && v == v0) == live) {
                if (lane == 0u) atomicAdd(&sub[wave][(v0 & 0xffu) * EQ_HIST_COPIES], 4u * (uint32_t)__popcll(live));
                continue;
            }
#endif
            if (flat) {
                atomicAdd(&mine[(v & 0xffu) * EQ_HIST_COPIES], 4u);
            } else {
#pragma unroll
                for (uint32_t c = 0; c < 4u; ++c)
                    if (c < n) atomicAdd(&mine[((v >> (8u * c)) & 0xffu) * EQ_HIST_COPIES], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < EQ_WAVES; ++k)
#pragma unroll
        for (uint32_t c = 0; c < EQ_HIST_COPIES; ++c) sum += sub[k][threadIdx.x * EQ_HIST_COPIES + c];
    if (sum) atomicAdd(&a.hist[(size_t)f * 256u + threadIdx.x], sum);
}

// One workgroup of 256 threads per frame, thread v the bin v.  i = the lowest non-empty bin; a frame of one value keeps its pixels
// (OpenCV's dst.setTo(i)): the identity.  Else scale = 255.f / (float)(total - hist[i]), one correctly rounded binary32 division;
// lut[i] = 0 and, for k > i, lut[k] = saturate_cast<uchar>((float)sum_k * scale) with sum_k = hist[i + 1] + .. + hist[k] as an int:
// int -> float rounds to nearest even (it matters above 2^24 pixels), one binary32 multiplication (-ffp-contract=off: nothing to fuse
// with), round half to even and clamp.  Entries below i are never read by a pixel of the frame: 0, so that lut[0] is 0 in every table.
__global__ __launch_bounds__(256) void equalize_lut(EqualizeArgs a) {
    __shared__ uint32_t scan[2][256];
    __shared__ unsigned long long nonzero[EQ_WAVES];
    const uint32_t f = blockIdx.x, t = threadIdx.x;
    kptr<AtlasFrameDev> frames = as_k(a.frames);
    const uint32_t total = frames[f].w * frames[f].h;
    const uint32_t hv = a.hist[(size_t)f * 256u + t];
    const unsigned long long m = __ballot(hv != 0u);
    if ((t & 63u) == 0u) nonzero[t >> 6] = m;
    __syncthreads();
    uint32_t i = 256u;
#pragma unroll
    for (int k = (int)EQ_WAVES - 1; k >= 0; --k)
        if (nonzero[k]) i = (uint32_t)k * 64u + (uint32_t)__builtin_ctzll(nonzero[k]);
    // inclusive scan of the bins above i (Hillis-Steele, eight steps; a frame has fewer than 2^30 pixels: no carry out of 32 bits)
    uint32_t cur = 0;
    scan[0][t] = t > i ? hv : 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const uint32_t s = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0u);
        cur ^= 1u;
        scan[cur][t] = s;
        __syncthreads();
    }
    const uint32_t sum = scan[cur][t];
    uint32_t out = t;   // (an empty or one-valued frame: the identity)
    if (i < 256u) {
        const uint32_t hi = a.hist[(size_t)f * 256u + i];
        if (hi != total) {
            const float scale = __fdiv_rn(255.f, (float)(int32_t)(total - hi));
            const int32_t q = __float2int_rn(__fmul_rn((float)(int32_t)sum, scale));
            out = t <= i ? 0u : (uint32_t)min(max(q, 0), 255);
        }
    }
    a.lut[(size_t)f * 256u + t] = (uint8_t)out;
}

// The pack kernel's shape: a workgroup is an ATLAS_BLOCK_W x ATLAS_BLOCK_H block of one frame, a wave one of its rows, a thread four
// pixels: load_gray4, four reads of the frame's table (staged in LDS, one byte per thread, one barrier before the first return) and
// one aligned dword store into frame f's image of the gray batch.  The store stays inside it: dx < w, so dx + 4 <= align4(w) <= pitch.
__global__ __launch_bounds__(256) void equalize_apply(EqualizeArgs a) {
    __shared__ uint8_t lut[256];
    kptr<AtlasFrameDev> frames = as_k(a.frames);
    const uint32_t unit = blockIdx.x;
    const uint32_t f = frame_of<false>(frames, a.n_frames, unit);
    lut[threadIdx.x] = a.lut[(size_t)f * 256u + threadIdx.x];
    __syncthreads();
    const uint32_t w = frames[f].w, h = frames[f].h;
    const uint32_t blocks_per_row = (w + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W;
    const uint32_t u = unit - frames[f].unit_first;
    const uint32_t by = u / blocks_per_row, bx = u - by * blocks_per_row;
    const uint32_t dx = bx * ATLAS_BLOCK_W + (threadIdx.x & 63u) * 4u, dy = by * ATLAS_BLOCK_H + (threadIdx.x >> 6);
    if (dy >= h || dx >= w || (a.dst_pitch & 3u) != 0u || dx + 4u > a.dst_pitch || dy >= a.dst_h) return;
    const uint8_t* row = frames[f].src + (size_t)dy * frames[f].stride;
    const uint32_t v = lut_gray4(lut, load_gray4(row, dx, w, frames[f].channels));
    *reinterpret_cast<uint32_t*>(a.dst + (size_t)f * a.dst_frame_bytes + (size_t)dy * a.dst_pitch + dx) = v;
}

int launch_equalize_hist(const EqualizeArgs& a, void* stream_) {
    if (a.n_hist_units == 0u || a.n_frames == 0u) return 0;
    hipLaunchKernelGGL(equalize_hist, dim3(a.n_hist_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_equalize_lut(const EqualizeArgs& a, void* stream_) {
    if (a.n_frames == 0u) return 0;
    hipLaunchKernelGGL(equalize_lut, dim3(a.n_frames), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_equalize_apply(const EqualizeArgs& a, void* stream_) {
    if (a.n_units == 0u || a.n_frames == 0u) return 0;
    hipLaunchKernelGGL(equalize_apply, dim3(a.n_units), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
