// cv::groupRectangles for the candidates of ONE frame by ONE workgroup of GROUP_THREADS threads (tempcv.cpp:130-243), as
// vj_group.cpp does it on the host: shared by group_frame (vj_group_dev.hip: the grouped faces of a first cascade become the
// regions of a second one) and cv_biggest_update (vj_cv_biggest.hip: CV_HAAR_FIND_BIGGEST_OBJECT's search step).
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include "vj_device.hpp"
#include "vj_devutil.hpp"

namespace vj {

constexpr uint32_t GROUP_THREADS = 1024;
constexpr size_t GROUP_LDS_BYTES = ((size_t)GROUP_MAX * 11u + 40u) * 4u;   // dynamic LDS of a kernel that calls group_classes

// ASimilarRects (tempcv.cpp:130-143), as vj_group.cpp evaluates it
__device__ __forceinline__ bool similar(int x1, int y1, int w1, int h1, int x2, int y2, int w2, int h2, double eps) {
    const double delta = eps * (double)(min(w1, w2) + min(h1, h2)) * 0.5;
    return (double)abs(x1 - x2) <= delta && (double)abs(y1 - y2) <= delta && (double)abs(x1 + w1 - x2 - w2) <= delta &&
           (double)abs(y1 + h1 - y2 - h2) <= delta;
}

// Order-preserving ranks of the set flags among items [0, n): rank_out[i] = number of set flags below i; returns the
// total.  Every thread of the workgroup calls it; scratch >= 33 words.
__device__ __forceinline__ uint32_t block_rank(const uint32_t* flag, uint32_t* rank_out, uint32_t n, uint32_t* scratch) {
    const uint32_t lane = lane_id(), wib = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += GROUP_THREADS) {   // at most two rounds
        const uint32_t i = i0 + threadIdx.x;
        const bool f = i < n && flag[i] != 0u;
        const unsigned long long m = __ballot(f);
        if (lane == 0u) scratch[wib] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < GROUP_THREADS / 64; ++w) {
            const uint32_t c = scratch[w];
            before += w < wib ? c : 0u;
            total += c;
        }
        if (i < n) rank_out[i] = carry + before + mbcnt(m);
        carry += total;
        __syncthreads();
    }
    return carry;
}
// The workgroup's LDS (GROUP_LDS_BYTES) as group_classes lays it out (words): keys / class sums share the front
struct GroupLds {
    uint64_t* keys;                 // [GROUP_MAX] u64 — dead after the decode
    int32_t *cx, *cy, *cw, *ch;     // class sums, then averages
    uint32_t* cn;                   // members per class
    int32_t *rx, *ry, *rw, *rh;     // the candidates
    uint32_t* label;                // component labels; after the filter: keep flags of the classes
    uint32_t* aux;                  // root flags -> class ranks; after the filter: output ranks of the kept classes
    uint32_t* scratch;              // 40 words
};
__device__ __forceinline__ GroupLds group_lds(uint32_t* lds) {
    GroupLds L;
    L.keys = reinterpret_cast<uint64_t*>(lds);
    L.cx = reinterpret_cast<int32_t*>(lds);
    L.cy = L.cx + GROUP_MAX;
    L.cw = L.cy + GROUP_MAX;
    L.ch = L.cw + GROUP_MAX;
    L.cn = reinterpret_cast<uint32_t*>(L.ch + GROUP_MAX);
    L.rx = reinterpret_cast<int32_t*>(L.cn + GROUP_MAX);
    L.ry = L.rx + GROUP_MAX;
    L.rw = L.ry + GROUP_MAX;
    L.rh = L.rw + GROUP_MAX;
    L.label = reinterpret_cast<uint32_t*>(L.rh + GROUP_MAX);
    L.aux = L.label + GROUP_MAX;
    L.scratch = L.aux + GROUP_MAX;
    return L;
}

// Groups n <= GROUP_MAX candidates (n != 0; every thread of the workgroup calls it).  key_at(i): the 64-bit sort key of candidate
// i, whose order is the canonical order of the list; decode(key, &x, &y, &w, &h): its rectangle.  Afterwards classes [0, *ncls) in
// partition()'s order hold their averaged rectangle in cx / cy / cw / ch and their member count in cn; label[c] != 0: class c
// survives the filter, aux[c]: its rank among the survivors.  Returns the number of survivors.
template <typename KeyAt, typename Decode>
__device__ __forceinline__ uint32_t group_classes(const GroupLds& L, uint32_t n, int32_t threshold, double eps, KeyAt key_at, Decode decode,
                                                  uint32_t* ncls_out) {
    uint64_t* keys = L.keys;
    int32_t *cx = L.cx, *cy = L.cy, *cw = L.cw, *ch = L.ch, *rx = L.rx, *ry = L.ry, *rw = L.rw, *rh = L.rh;
    uint32_t *cn = L.cn, *label = L.label, *aux = L.aux, *scratch = L.scratch;
    const uint32_t tid = threadIdx.x;
    // ---- canonical order: sort the frame's keys
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = tid; i < P; i += GROUP_THREADS) keys[i] = i < n ? key_at(i) : ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j != 0u; j >>= 1) {
            for (uint32_t i = tid; i < P; i += GROUP_THREADS) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const uint64_t a = keys[i], b = keys[l];
                    if (((i & k) == 0u) == (a > b)) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < n; i += GROUP_THREADS) {
        int32_t x, y, w, h;
        decode(keys[i], &x, &y, &w, &h);
        rx[i] = x;
        ry[i] = y;
        rw[i] = w;
        rh[i] = h;
        label[i] = i;
    }
    __syncthreads();
    // ---- connected components: label = smallest index of the component
    for (;;) {
        if (tid == 0u) scratch[36] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += GROUP_THREADS) {
            const int x1 = rx[i], y1 = ry[i], w1 = rw[i], h1 = rh[i];
            uint32_t m = label[i];
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t lj = label[j];   // racing with j's own update: any value read is a member of j's component
                if (lj < m && similar(x1, y1, w1, h1, rx[j], ry[j], rw[j], rh[j], eps)) m = lj;   // (symmetric in value)
            }
            if (m < label[i]) {
                label[i] = m;
                scratch[36] = 1u;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < n; i += GROUP_THREADS) {   // pointer jumping
            uint32_t l = label[i];
            while (label[l] < l) l = label[l];
            label[i] = l;
        }
        __syncthreads();
        if (scratch[36] == 0u) break;
        __syncthreads();
    }
    // ---- classes in order of first appearance
    for (uint32_t i = tid; i < n; i += GROUP_THREADS) aux[i] = label[i] == i ? 1u : 0u;
    __syncthreads();
    // a root's rank among the roots is its class index (aux is overwritten in place; only root positions are meaningful)
    const uint32_t ncls = block_rank(aux, aux, n, scratch);
    __syncthreads();
    for (uint32_t i = tid; i < ncls; i += GROUP_THREADS) {   // (the key array is dead: the sums live there)
        cx[i] = 0; cy[i] = 0; cw[i] = 0; ch[i] = 0; cn[i] = 0u;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += GROUP_THREADS) {
        const uint32_t c = aux[label[i]];
        // int accumulators as in the original (tempcv.cpp:167-172); atomics on int wrap like the host's unsigned adds
        atomicAdd(cx + c, rx[i]);
        atomicAdd(cy + c, ry[i]);
        atomicAdd(cw + c, rw[i]);
        atomicAdd(ch + c, rh[i]);
        atomicAdd(cn + c, 1u);
    }
    __syncthreads();
    auto sat = [](float v) { return v > (float)INT_MAX ? INT_MAX : (int)v; };
    for (uint32_t i = tid; i < ncls; i += GROUP_THREADS) {
        const float s = 1.f / (float)(int)cn[i];
        cx[i] = sat((float)cx[i] * s);
        cy[i] = sat((float)cy[i] * s);
        cw[i] = sat((float)cw[i] * s);
        ch[i] = sat((float)ch[i] * s);
    }
    __syncthreads();
    // ---- drop weak classes and small rectangles inside larger, better supported ones (tempcv.cpp:205-242)
    for (uint32_t i = tid; i < ncls; i += GROUP_THREADS) {
        const int n1 = (int)cn[i];
        uint32_t keep = n1 > threshold ? 1u : 0u;
        if (keep) {
            const int x1 = cx[i], y1 = cy[i], w1 = cw[i], h1 = ch[i];
            for (uint32_t j = 0; j < ncls; ++j) {
                const int n2 = (int)cn[j];
                if (j == i || n2 <= threshold) continue;
                const int x2 = cx[j], y2 = cy[j], w2 = cw[j], h2 = ch[j];
                const int dx = (double)w2 * eps > (double)INT_MAX ? INT_MAX : (int)((double)w2 * eps);
                const int dy = (double)h2 * eps > (double)INT_MAX ? INT_MAX : (int)((double)h2 * eps);
                typedef long long ll;
                if (x1 >= (ll)x2 - dx && y1 >= (ll)y2 - dy && (ll)x1 + w1 <= (ll)x2 + w2 + dx && (ll)y1 + h1 <= (ll)y2 + h2 + dy &&
                    (n2 > max(3, n1) || n1 < 3)) {
                    keep = 0u;
                    break;
                }
            }
        }
        label[i] = keep;   // (the labels are no longer needed)
    }
    __syncthreads();
    const uint32_t n_out = block_rank(label, aux, ncls, scratch);
    __syncthreads();
    *ncls_out = ncls;
    return n_out;
}

}  // namespace vj
