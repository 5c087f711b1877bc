// gfx950 kernels of the Canny edge map that CV_HAAR_DO_CANNY_PRUNING adds to the OpenCV profile:
// cvCanny(gray, edges, 0, 50, 3) (tempcv.cpp:1337-1343; OpenCV 2.4.2 imgproc, third-party, parity unpinned) as
// DESIGN.md §4.7 restates it — all integer arithmetic:
//   Sobel 3x3 with BORDER_REPLICATE, m = |dx| + |dy| (0 outside the frame), non-maximum suppression with the
//   fixed-point tangents TG22 = 13573 (2^15 tan 22.5°) and tan 67.5° = TG22 + 2 at 15 fractional bits,
//   candidates m > 0, strong candidates m > 50, edges = the 8-connected components of candidates that hold
//   a strong pixel.
// Hysteresis is a connected-components problem; it is solved with union-find labelling in a fixed number of
// launches, whatever the content (a weak path may snake across the whole frame, so repeated dilation has no
// bound):
//   1. canny_nms_local  a 64 x 16 tile per workgroup: gray (2-pixel clamped halo) staged in LDS with 4-pixel
//                       loads, Sobel + NMS -> class byte (0 none, 1 weak, 2 strong), union-find of the tile's
//                       candidates in LDS; every candidate's parent is its tile-local root (frame-local index)
//   2. canny_merge      the 8-neighbour pairs that cross a tile border, united in global memory
//                       (CAS on roots, larger root under smaller; path halving)
//   3. canny_resolve    every candidate's parent becomes its final root; strong candidates flag their root
//   4. canny_emit       edge = candidate && flag[root] ? 255 : 0
// Every parent read in launches 2-4 is an agent-scope atomic load: plain loads may hit a stale L1 line that
// another CU's workgroup has since changed (MI355X: L1 is not coherent between CUs within a launch).
#include <hip/hip_runtime.h>
#include "vj_device.hpp"
#include "vj_devutil.hpp"

namespace vj {

constexpr int32_t CN_TW = 64, CN_TH = 16;            // tile of output pixels
constexpr int32_t CN_GQ = (CN_TW + 8) / 4;           // gray quads per LDS row: x0 - 4 .. x0 + CN_TW + 3
constexpr int32_t CN_GH = CN_TH + 4;                 // gray rows: y0 - 2 .. y0 + CN_TH + 1
constexpr int32_t CN_MW = CN_TW + 2, CN_MH = CN_TH + 2;   // magnitudes: the tile and a 1-pixel ring
constexpr uint32_t CN_NONE = 0xffffffffu;

__device__ __forceinline__ uint32_t gray_px(const uint8_t* row, int32_t x, uint32_t ch) {
    if (ch <= 1u) return row[x];
    const uint8_t* p = row + (size_t)x * ch;
    return bgr2gray(p[0], p[1], p[2]);
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; halves the path on the way (a parent only ever moves to an ancestor, so a lost race is harmless)
__device__ __forceinline__ uint32_t uf_find(uint32_t* P, uint32_t x) {
    while (true) {
        const uint32_t p = uf_load(P + x);
        if (p == x) return x;
        const uint32_t gp = uf_load(P + p);
        if (gp == p) return p;
        uint32_t expect = p;
        __hip_atomic_compare_exchange_strong(P + x, &expect, gp, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = gp;
    }
}

__device__ __forceinline__ void uf_unite(uint32_t* P, uint32_t a, uint32_t b) {
    while (true) {
        a = uf_find(P, a);
        b = uf_find(P, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t expect = a;   // link the larger root under the smaller: parents only decrease, no cycle
        if (__hip_atomic_compare_exchange_strong(P + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    }
}

__device__ __forceinline__ uint32_t lds_find(uint32_t* L, uint32_t x) {
    while (true) {
        const uint32_t p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

// Playne & Hawick's merge: atomicMin on the larger root; if it was no longer a root, continue with what it pointed to
__device__ __forceinline__ void lds_unite(uint32_t* L, uint32_t a, uint32_t b) {
    while (true) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void canny_nms_local(CannyArgs a) {
    __shared__ uint32_t g4[CN_GH][CN_GQ];
    __shared__ int32_t mag[CN_MH][CN_MW];
    __shared__ uint32_t lab[CN_TH * CN_TW];
    __shared__ uint8_t cls_l[CN_TH * CN_TW];
    const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
    const int32_t x0 = (int32_t)blockIdx.x * CN_TW, y0 = (int32_t)blockIdx.y * CN_TH;
    const uint32_t frame = blockIdx.z, tid = threadIdx.x;
    const uint8_t* img = a.gray + (size_t)frame * a.gray_frame_bytes;
    // gray with a clamped halo (BORDER_REPLICATE), four pixels per load
    for (uint32_t i = tid; i < (uint32_t)(CN_GH * CN_GQ); i += 256u) {
        const int32_t r = (int32_t)i / CN_GQ, q = (int32_t)i % CN_GQ;
        const int32_t y = min(max(y0 + r - 2, 0), H - 1);
        const int32_t xq = x0 - 4 + 4 * q;
        const uint8_t* row = img + (size_t)y * a.gray_stride;
        uint32_t v = 0;
        if (xq >= 0 && xq + 4 <= W) {
            v = load_gray4(row, (uint32_t)xq, a.width, a.channels);
        } else {
#pragma unroll
            for (int32_t c = 0; c < 4; ++c) v |= gray_px(row, min(max(xq + c, 0), W - 1), a.channels) << (8 * c);
        }
        g4[r][q] = v;
    }
    __syncthreads();
    // gray at LDS column lx (frame x = x0 - 4 + lx), LDS row ly (frame y = y0 - 2 + ly)
    auto G = [&](int32_t lx, int32_t ly) -> int32_t { return (int32_t)((g4[ly][lx >> 2] >> ((lx & 3) * 8)) & 0xffu); };
    auto sobel = [&](int32_t lx, int32_t ly, int32_t& dx, int32_t& dy) {
        dx = (G(lx + 1, ly - 1) - G(lx - 1, ly - 1)) + 2 * (G(lx + 1, ly) - G(lx - 1, ly)) + (G(lx + 1, ly + 1) - G(lx - 1, ly + 1));
        dy = (G(lx - 1, ly + 1) - G(lx - 1, ly - 1)) + 2 * (G(lx, ly + 1) - G(lx, ly - 1)) + (G(lx + 1, ly + 1) - G(lx + 1, ly - 1));
    };
    for (uint32_t i = tid; i < (uint32_t)(CN_MH * CN_MW); i += 256u) {
        const int32_t my = (int32_t)i / CN_MW, mx = (int32_t)i % CN_MW;
        const int32_t x = x0 + mx - 1, y = y0 + my - 1;
        int32_t m = 0;   // 0 outside the frame
        if (x >= 0 && x < W && y >= 0 && y < H) {
            int32_t dx, dy;
            sobel(mx + 3, my + 1, dx, dy);
            m = abs(dx) + abs(dy);
        }
        mag[my][mx] = m;
    }
    __syncthreads();
    const int32_t tx = (int32_t)(tid & 63u);
#pragma unroll
    for (int32_t k = 0; k < 4; ++k) {
        const int32_t ty = (int32_t)(tid >> 6) + 4 * k, idx = ty * CN_TW + tx;
        const int32_t mx = tx + 1, my = ty + 1, m = mag[my][mx];
        uint8_t c = 0;
        if (m > 0) {   // (0 outside the frame)
            int32_t dx, dy;
            sobel(tx + 4, ty + 2, dx, dy);
            const int32_t ax = abs(dx), ay = abs(dy) << 15;
            const int32_t tg22x = ax * 13573, tg67x = tg22x + (ax << 16);
            bool cand;
            if (ay < tg22x) {
                cand = m > mag[my][mx - 1] && m >= mag[my][mx + 1];
            } else if (ay > tg67x) {
                cand = m > mag[my - 1][mx] && m >= mag[my + 1][mx];
            } else {
                const int32_t s = (dx ^ dy) < 0 ? -1 : 1;
                cand = m > mag[my - 1][mx - s] && m > mag[my + 1][mx + s];
            }
            if (cand) c = m > 50 ? 2 : 1;
        }
        cls_l[idx] = c;
        lab[idx] = c ? (uint32_t)idx : CN_NONE;
    }
    __syncthreads();
    // the tile's components: every candidate unites with its W, NW, N, NE candidate neighbours inside the tile
#pragma unroll
    for (int32_t k = 0; k < 4; ++k) {
        const int32_t ty = (int32_t)(tid >> 6) + 4 * k, idx = ty * CN_TW + tx;
        if (!cls_l[idx]) continue;
        if (tx > 0 && cls_l[idx - 1]) lds_unite(lab, (uint32_t)idx, (uint32_t)(idx - 1));
        if (ty > 0) {
            if (tx > 0 && cls_l[idx - CN_TW - 1]) lds_unite(lab, (uint32_t)idx, (uint32_t)(idx - CN_TW - 1));
            if (cls_l[idx - CN_TW]) lds_unite(lab, (uint32_t)idx, (uint32_t)(idx - CN_TW));
            if (tx + 1 < CN_TW && cls_l[idx - CN_TW + 1]) lds_unite(lab, (uint32_t)idx, (uint32_t)(idx - CN_TW + 1));
        }
    }
    __syncthreads();
    const size_t fbase = (size_t)frame * (size_t)a.width * (size_t)a.height;
#pragma unroll
    for (int32_t k = 0; k < 4; ++k) {
        const int32_t ty = (int32_t)(tid >> 6) + 4 * k, idx = ty * CN_TW + tx;
        const int32_t x = x0 + tx, y = y0 + ty;
        if (x >= W || y >= H) continue;
        const size_t p = fbase + (size_t)y * (size_t)W + (size_t)x;
        const uint8_t c = cls_l[idx];
        a.cls[p] = c;
        if (c) {
            const uint32_t r = lds_find(lab, (uint32_t)idx);
            a.label[p] = (uint32_t)(y0 + (int32_t)(r / CN_TW)) * (uint32_t)W + (uint32_t)(x0 + (int32_t)(r % CN_TW));
        }
    }
}

// the candidate pairs that cross a tile border: the top row (N, NW, NE), the left column (W, NW) and the right column (NE)
__global__ __launch_bounds__(128) void canny_merge(CannyArgs a) {
    const int32_t W = (int32_t)a.width, H = (int32_t)a.height;
    const int32_t t = (int32_t)threadIdx.x;
    int32_t tx, ty;
    if (t < CN_TW) { tx = t; ty = 0; }
    else if (t < CN_TW + CN_TH) { tx = 0; ty = t - CN_TW; }
    else if (t < CN_TW + 2 * CN_TH) { tx = CN_TW - 1; ty = t - CN_TW - CN_TH; }
    else return;
    const int32_t x = (int32_t)blockIdx.x * CN_TW + tx, y = (int32_t)blockIdx.y * CN_TH + ty;
    if (x >= W || y >= H) return;
    const size_t fbase = (size_t)blockIdx.z * (size_t)a.width * (size_t)a.height;
    const uint8_t* cls = a.cls + fbase;
    uint32_t* P = a.label + fbase;
    const uint32_t p = (uint32_t)(y * W + x);
    if (!cls[p]) return;
    const int32_t nb[4][2] = {{x - 1, y}, {x - 1, y - 1}, {x, y - 1}, {x + 1, y - 1}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t nx = nb[k][0], ny = nb[k][1];
        if (nx < 0 || ny < 0 || nx >= W) continue;
        if (nx / CN_TW == x / CN_TW && ny / CN_TH == y / CN_TH) continue;   // same tile: united in LDS already
        const uint32_t q = (uint32_t)(ny * W + nx);
        if (cls[q]) uf_unite(P, p, q);
    }
}

__global__ __launch_bounds__(256) void canny_resolve(CannyArgs a) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= a.width) return;
    const size_t fbase = (size_t)blockIdx.z * (size_t)a.width * (size_t)a.height;
    const uint32_t p = y * a.width + x;
    const uint8_t c = a.cls[fbase + p];
    if (!c) return;
    uint32_t* P = a.label + fbase;
    const uint32_t r = uf_find(P, p);
    __hip_atomic_store(P + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (c == 2) a.flag[fbase + r] = 1;
}

__global__ __launch_bounds__(256) void canny_emit(CannyArgs a) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y;
    if (x >= a.width) return;
    const size_t fbase = (size_t)blockIdx.z * (size_t)a.width * (size_t)a.height;
    const uint32_t p = y * a.width + x;
    uint8_t e = 0;
    if (a.cls[fbase + p] && a.flag[fbase + uf_load(a.label + fbase + p)]) e = 255;
    a.edges[(size_t)blockIdx.z * a.edge_frame_bytes + (size_t)y * a.edge_pitch + x] = e;
}

int launch_canny(const CannyArgs& a, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 tiles((a.width + CN_TW - 1u) / CN_TW, (a.height + CN_TH - 1u) / CN_TH, a.n_frames);
    const dim3 rows((a.width + 255u) / 256u, a.height, a.n_frames);
    hipError_t err = hipMemsetAsync(a.flag, 0, (size_t)a.width * a.height * a.n_frames, stream);
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(canny_nms_local, tiles, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(canny_merge, tiles, dim3(128), 0, stream, a);
    hipLaunchKernelGGL(canny_resolve, rows, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(canny_emit, rows, dim3(256), 0, stream, a);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------ the pruning test on the tile scales
__global__ __launch_bounds__(256) void cv_prune_mark(CvPruneArgs a) {
    const uint32_t lane = lane_id();
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    kptr<UnitDev> segs = as_k(a.segs);
    kptr<CvScaleDev> scales = as_k(a.scales);
    kptr<CvPruneDev> pr = as_k(a.prune);
    const uint32_t frame_bytes4 = a.frame_elems * 4u;
    const rsrc_t img = make_rsrc(a.sum, a.n_frames * frame_bytes4), eimg = make_rsrc(a.edge_sum, a.n_frames * frame_bytes4);
    const uint32_t total = a.n_segs * a.n_frames;
    for (uint32_t u = wave; u < total; u += n_waves) {
        const uint32_t frame = u / a.n_segs, r = u - frame * a.n_segs;
        const uint32_t slot = segs[r].scale, first = segs[r].first, wpr = segs[r].count;
        const uint32_t iy = (first - scales[slot].bits_base) / wpr, end_x = scales[slot].end_x;
        const double ystep = scales[slot].ystep;
        const uint32_t e0 = pr[slot].p0 * 4u, e1 = pr[slot].p1 * 4u, e2 = pr[slot].p2 * 4u, e3 = pr[slot].p3 * 4u;
        const uint32_t y = (uint32_t)__double2int_rn((double)iy * ystep);
        const size_t w0 = (size_t)frame * a.bits_frame_words + first;
        for (uint32_t w = 0; w < wpr; ++w) {
            const uint32_t ix = w * 64u + lane;
            const bool valid = ix < end_x;
            const uint32_t x = (uint32_t)__double2int_rn((double)(valid ? ix : 0u) * ystep);
            const uint32_t off = frame * frame_bytes4 + (y * a.stride + x) * 4u;
            const unsigned long long pm = __ballot(valid && cv_pruned(eimg, img, off, e0, e1, e2, e3));
            if (lane == 0) {
                a.prune_bits[w0 + w] = pm;
                if (pm != 0ull) {
                    a.bits[w0 + w] |= pm;
                    if (a.accept) a.accept[w0 + w] &= ~pm;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void cv_prune_visited(CvPruneArgs a) {
    const size_t n = (size_t)a.bits_frame_words * a.n_frames;
    uint32_t pruned = 0;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const unsigned long long pm = a.prune_bits[i];
        if (pm == 0ull) continue;
        const unsigned long long v = a.bits[i];
        pruned += (uint32_t)__popcll(v & pm);
        a.bits[i] = v & ~pm;
    }
    if (a.windows) {
        const unsigned long long s = (unsigned long long)__reduce_add_sync(~0ull, pruned);
        if (lane_id() == 0 && s != 0ull) atomicAdd(a.windows, s);
    }
}

int launch_cv_prune_mark(const CvPruneArgs& a, int n_blocks, void* stream_) {
    hipLaunchKernelGGL(cv_prune_mark, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

int launch_cv_prune_visited(const CvPruneArgs& a, int n_blocks, void* stream_) {
    hipLaunchKernelGGL(cv_prune_visited, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream_, a);
    return (int)hipGetLastError();
}

}  // namespace vj
