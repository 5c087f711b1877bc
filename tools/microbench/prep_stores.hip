// What the four-pixel dword store of prep_resize (csrc/vj_prep.hip) buys over pyramid_levels' byte stores
// (csrc/vj_pyramid.hip: one pixel per thread): both kernels resize the SAME batch — 64 gray frames of 1920 x 1080 on the device, one
// level of one size per frame, one launch each — to 960 x 540 (the 2 x 2 mean) and to 1000 x 562 (bilinear).  Times from events,
// median of nine launches after two warm-ups, twice (the A/A pair); the outputs are compared byte for byte.
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 -DVJ_BUILDING tools/microbench/prep_stores.hip \
//       clfacedetection_amd/csrc/{vj_cv_roi_levels_host,vj_cv_roi_host,vj_cascade,vj_group}.cpp -o prep_stores && ./prep_stores
#include "../../clfacedetection_amd/csrc/vj_pyramid.hip"
#include "../../clfacedetection_amd/csrc/vj_prep.hip"
#include "../../clfacedetection_amd/csrc/vj_cv_roi_levels_host.hpp"

#include <algorithm>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vj;

#define HIP_OK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

static float median_ms(const std::function<int()>& launch, hipStream_t s) {
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    std::vector<float> t;
    for (int k = 0; k < 11; ++k) {
        HIP_OK(hipEventRecord(a, s));
        if (launch()) {
            fprintf(stderr, "launch failed\n");
            exit(1);
        }
        HIP_OK(hipEventRecord(b, s));
        HIP_OK(hipEventSynchronize(b));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, a, b));
        if (k >= 2) t.push_back(ms);
    }
    HIP_OK(hipEventDestroy(a));
    HIP_OK(hipEventDestroy(b));
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main() {
    const uint32_t N = 64, W = 1920, H = 1080;
    hipStream_t s;
    HIP_OK(hipStreamCreate(&s));
    std::vector<uint8_t> host((size_t)N * W * H);
    uint32_t x = 12345u;
    for (uint8_t& v : host) {
        x = x * 1664525u + 1013904223u;
        v = (uint8_t)(x >> 24);
    }
    uint8_t* d_src;
    HIP_OK(hipMalloc(&d_src, host.size()));
    HIP_OK(hipMemcpy(d_src, host.data(), host.size(), hipMemcpyHostToDevice));
    const uint32_t sizes[][2] = {{960, 540}, {1000, 562}};
    for (const auto& sz : sizes) {
        const uint32_t dw = sz[0], dh = sz[1], pitch = (dw + 3u) & ~3u, xrun = (dw + 3u) & ~3u;
        const uint64_t frame_bytes = ((uint64_t)pitch * dh + 255u) & ~(uint64_t)255;
        const bool area = resize_is_area((int)W, (int)H, (int)dw, (int)dh);
        // taps: the columns' run padded to 4 taps with its last one, then the rows'
        std::vector<PyrTap> taps((size_t)xrun + dh);
        build_taps((int)W, (int)dw, false, area, taps.data());
        for (uint32_t k = dw; k < xrun; ++k) taps[k] = taps[dw - 1u];
        build_taps((int)H, (int)dh, true, area, taps.data() + xrun);
        PyrTap* d_taps;
        HIP_OK(hipMalloc(&d_taps, taps.size() * sizeof(PyrTap)));
        HIP_OK(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(PyrTap), hipMemcpyHostToDevice));
        uint8_t *d_a, *d_b;
        HIP_OK(hipMalloc(&d_a, frame_bytes * N));
        HIP_OK(hipMalloc(&d_b, frame_bytes * N));
        HIP_OK(hipMemset(d_a, 0, frame_bytes * N));
        HIP_OK(hipMemset(d_b, 0, frame_bytes * N));
        // pyramid_levels: one level at the canvas's origin, a canvas per frame
        const PyrLevelDev lv{0u, 0u, dw, dh, 0u, xrun, 0u, area ? 1u : 0u};
        PyrLevelDev* d_lv;
        HIP_OK(hipMalloc(&d_lv, sizeof(lv)));
        HIP_OK(hipMemcpy(d_lv, &lv, sizeof(lv), hipMemcpyHostToDevice));
        PyrArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.gray = d_src;
        pa.gray_frame_bytes = (uint64_t)W * H;
        pa.gray_stride = W;
        pa.channels = 1;
        pa.width = W;
        pa.height = H;
        pa.n_frames = N;
        pa.levels = d_lv;
        pa.n_levels = 1;
        pa.n_units = ((dw + PYR_UNIT_PX - 1u) / PYR_UNIT_PX) * dh;
        pa.taps = d_taps;
        pa.canvas = d_a;
        pa.canvas_pitch = pitch;
        pa.canvas_w = dw;
        pa.canvas_h = dh;
        pa.canvas_frame_bytes = frame_bytes;
        // prep_resize<false>: one record per frame
        std::vector<PrepFrameDev> recs(N);
        const uint32_t units = (uint32_t)prep_units(dw, dh);
        for (uint32_t i = 0; i < N; ++i) {
            PrepFrameDev& r = recs[i];
            memset(&r, 0, sizeof(r));
            r.src = d_src + (size_t)i * W * H;
            r.dst_off = frame_bytes * i;
            r.stride = W;
            r.channels = 1;
            r.sw = W;
            r.sh = H;
            r.dw = dw;
            r.dh = dh;
            r.pitch = pitch;
            r.xtab = 0;
            r.ytab = xrun;
            r.mode = area ? PREP_AREA : PREP_BILINEAR;
            r.unit_first = units * i;
            r.hist_slot = i;
        }
        PrepFrameDev* d_recs;
        HIP_OK(hipMalloc(&d_recs, recs.size() * sizeof(PrepFrameDev)));
        HIP_OK(hipMemcpy(d_recs, recs.data(), recs.size() * sizeof(PrepFrameDev), hipMemcpyHostToDevice));
        PrepArgs pr;
        memset(&pr, 0, sizeof(pr));
        pr.frames = d_recs;
        pr.n_frames = N;
        pr.n_units = units * N;
        pr.taps = d_taps;
        pr.dst = d_b;
        pr.dst_bytes = frame_bytes * N;
        float t_pyr[2], t_prep[2];
        for (int pair = 0; pair < 2; ++pair) {
            t_pyr[pair] = median_ms([&] { return launch_pyramid(pa, s); }, s);
            t_prep[pair] = median_ms([&] { return launch_prep_resize(pr, false, s); }, s);
        }
        std::vector<uint8_t> out_a(frame_bytes * N), out_b(frame_bytes * N);
        HIP_OK(hipMemcpy(out_a.data(), d_a, out_a.size(), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(out_b.data(), d_b, out_b.size(), hipMemcpyDeviceToHost));
        const bool same = out_a == out_b;
        const double bytes = (double)N * ((double)W * H + (double)dw * dh);
        printf("{\"to\": [%u, %u], \"area\": %d, \"pyramid_levels_ms\": [%.4f, %.4f], \"prep_resize_ms\": [%.4f, %.4f], \"bytes\": %.0f, "
               "\"pyramid_levels_tb_per_s\": %.3f, \"prep_resize_tb_per_s\": %.3f, \"outputs_equal\": %s}\n",
               dw, dh, (int)area, t_pyr[0], t_pyr[1], t_prep[0], t_prep[1], bytes, bytes / (0.5 * (t_pyr[0] + t_pyr[1])) / 1e9,
               bytes / (0.5 * (t_prep[0] + t_prep[1])) / 1e9, same ? "true" : "false");
        if (!same) return 1;
        for (void* p : {(void*)d_taps, (void*)d_a, (void*)d_b, (void*)d_lv, (void*)d_recs}) HIP_OK(hipFree(p));
    }
    HIP_OK(hipFree(d_src));
    HIP_OK(hipStreamDestroy(s));
    return 0;
}
