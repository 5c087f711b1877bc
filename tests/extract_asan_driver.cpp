// Sanitizer driver of the host planner of vj_extract (csrc/vj_extract_host.cpp: the argument checks, the mapping of regions to source
// pixels, the region records, taps and work units of a slice): built by tests/test_sanitizers_extract.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/extract_asan_driver.cpp csrc/vj_extract_host.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp
//       csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Frames of three channel counts in heap blocks that END with their last row, regions inside them, over every
// side and corner, wholly outside and with margins, to several output sizes (the copy, the 2 x 2 mean, bilinear), interleaved, planar
// and gray, the destination at every address mod 4, whole and in slices.  The work units are decoded as the kernel decodes them
// (region from the unit prefix, block, wave, lane -> the slot's bytes): every output byte of every region is covered exactly once,
// every tap the kernel would load lies inside its run, every clamped source index inside its frame — the bytes are read, so ASan
// sees each access — and a wide load happens only inside a crop that lies inside its frame.  Then the error cases.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_extract_host.hpp"
#include "../clfacedetection_amd/csrc/vj_prep_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

struct Frames {
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    std::vector<vj_image> im;
    void add(int w, int h, int ch, int pad) {
        const int stride = w * ch + pad;
        const size_t bytes = (size_t)(h - 1) * (size_t)stride + (size_t)w * ch;   // the block ends with the last row's last byte
        mem.emplace_back(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) mem.back()[i] = (uint8_t)(i * 7u + 1u);
        im.push_back(vj_image{mem.back().get(), w, h, stride, 0, ch});
    }
};

static volatile uint32_t sink;
static int clampi(int v, int hi) { return std::min(std::max(v, 0), hi); }

// one pixel read as the kernel reads it: inside the frame, and the bytes touched
static void read_px(const vj_image& f, int xs, int ys, uint32_t c, bool conv) {
    CHECK(xs >= 0 && xs < f.width && ys >= 0 && ys < f.height);
    const int ch = f.channels <= 1 ? 1 : f.channels;
    const uint8_t* p = f.data + (size_t)ys * (size_t)f.stride + (size_t)xs * ch;
    if (conv) sink = sink + p[0] + p[1] + p[2];
    else {
        CHECK((int)c < ch);
        sink = sink + p[c];
    }
}

// the whole call through the C entry point and the planner, then every slice of at most `max_frames` distinct frames, checked with
// the destination at address `dst_mod` mod 4
static void plan_all(const Frames& fr, const std::vector<vj_roi>& regions, const vj_extract_params& p, size_t max_frames, uint32_t dst_mod) {
    const int nf = (int)fr.im.size(), n = (int)regions.size();
    std::vector<vj_roi> src((size_t)n + 1);
    int channels = -1;
    uint64_t bytes = 1;
    CHECK(vj_extract_layout(fr.im.data(), nf, regions.data(), n, &p, src.data(), &channels, &bytes) == VJ_OK);
    ExtractLayout lay;
    CHECK(extract_layout(fr.im.data(), nf, regions.data(), n, &p, &lay) == VJ_OK && lay.bytes == bytes && lay.src.size() == (size_t)n);
    CHECK((int)lay.C == channels && (channels == 1 || channels == 3 || channels == 4));
    CHECK(lay.gray == ((p.flags & VJ_EXTRACT_GRAY) != 0u) && lay.planar == ((p.flags & VJ_EXTRACT_PLANAR) != 0u));
    CHECK(lay.out_w == (uint32_t)p.out_w && lay.out_h == (uint32_t)p.out_h);
    CHECK(lay.region_bytes == (uint64_t)p.out_w * p.out_h * lay.C && bytes == lay.region_bytes * (uint64_t)n);
    CHECK(lay.rows == (lay.planar ? lay.C * lay.out_h : lay.out_h) && lay.row_bytes == (lay.planar ? lay.out_w : lay.out_w * lay.C));
    const double sx = p.sx == 0 ? 1 : p.sx, sy = p.sy == 0 ? 1 : p.sy;
    for (int r = 0; r < n; ++r) {
        const vj_roi& g = regions[(size_t)r];
        const vj_roi& s = lay.src[(size_t)r];
        CHECK(memcmp(&s, &src[(size_t)r], sizeof(s)) == 0);
        const long w0 = std::max(1l, std::lrint(g.w * sx)), h0 = std::max(1l, std::lrint(g.h * sy));
        const long mx = std::lrint((double)w0 * p.margin), my = std::lrint((double)h0 * p.margin);
        CHECK(s.frame == g.frame && s.x == std::lrint(g.x * sx) - mx && s.y == std::lrint(g.y * sy) - my && s.w == w0 + 2 * mx && s.h == h0 + 2 * my);
    }
    std::vector<uint8_t> covered((size_t)bytes, 0);
    const uint32_t B = lay.row_bytes, R = lay.rows, C = lay.C;
    ExtractSlice sl;
    size_t slices = 0;
    for (size_t first = 0; first < (size_t)n; ++slices) {
        const size_t end = extract_slice_end(regions.data(), (size_t)n, first, max_frames);
        CHECK(end > first && end <= (size_t)n);
        const size_t m = end - first;
        CHECK(extract_plan_slice(fr.im.data(), regions.data(), lay, first, m, &sl) == VJ_OK);
        CHECK(sl.recs.size() == m && !sl.frames.empty());
        if (max_frames) {
            CHECK(sl.frames.size() <= max_frames);
            if (end < (size_t)n) {   // greedy: the next region names a frame the slice does not hold, and the slice is full
                CHECK(sl.frames.size() == max_frames);
                CHECK(std::find(sl.frames.begin(), sl.frames.end(), regions[end].frame) == sl.frames.end());
            }
        } else {
            CHECK(end == (size_t)n);
        }
        uint64_t unit = 0;
        for (size_t i = 0; i < m; ++i) {
            const ExtractRegionDev& d = sl.recs[i];
            const vj_roi& s = lay.src[first + i];
            const vj_image& f = fr.im[(size_t)s.frame];
            CHECK(std::find(sl.frames.begin(), sl.frames.end(), s.frame) != sl.frames.end());
            CHECK(d.src == f.data && d.stride == (uint32_t)f.stride && d.channels == (uint32_t)f.channels && d.fw == f.width && d.fh == f.height);
            CHECK(d.x0 == s.x && d.y0 == s.y && d.cw == (uint32_t)s.w && d.ch == (uint32_t)s.h && d.dst_off == (first + i) * lay.region_bytes);
            CHECK(d.unit_first == unit);
            unit += extract_units(B, R);
            CHECK((d.mode == EXTRACT_COPY) == (d.cw == lay.out_w && d.ch == lay.out_h));
            CHECK((d.mode == EXTRACT_AREA) == (d.cw == 2u * lay.out_w && d.ch == 2u * lay.out_h));
            if (d.mode == EXTRACT_COPY) continue;
            CHECK((size_t)d.xtab + lay.out_w <= sl.taps.size() && (size_t)d.ytab + lay.out_h <= sl.taps.size());
            for (uint32_t x = 0; x < lay.out_w; ++x) {   // every tap inside its run: the crop
                const PyrTap& tp = sl.taps[(size_t)d.xtab + x];
                CHECK(tp.i0 < d.cw && tp.i1 < d.cw);
                if (d.mode == EXTRACT_AREA) CHECK(tp.i0 == 2u * x && tp.i1 == 2u * x + 1u);
            }
            for (uint32_t y = 0; y < lay.out_h; ++y) {
                const PyrTap& tp = sl.taps[(size_t)d.ytab + y];
                CHECK(tp.i0 < d.ch && tp.i1 < d.ch);
                if (d.mode == EXTRACT_AREA) CHECK(tp.i0 == 2u * y && tp.i1 == 2u * y + 1u);
            }
        }
        CHECK(unit == sl.n_units);
        // the units as the kernel decodes them
        for (uint32_t u0 = 0; u0 < sl.n_units; ++u0) {
            uint32_t lo = 0, hi = (uint32_t)m;
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sl.recs[mid].unit_first <= u0) lo = mid;
                else hi = mid;
            }
            const ExtractRegionDev& d = sl.recs[lo];
            const vj_image& f = fr.im[(size_t)lay.src[first + lo].frame];
            CHECK(d.dst_off + (uint64_t)R * B <= bytes);
            const uint32_t bpr = extract_row_blocks(B), u = u0 - d.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            CHECK(by * EXTRACT_BLOCK_H < R);
            const bool conv = lay.gray && d.channels > 1u;
            const bool crop_inside = d.x0 >= 0 && d.y0 >= 0 && (int64_t)d.x0 + d.cw <= d.fw && (int64_t)d.y0 + d.ch <= d.fh;
            const bool wide_copy = crop_inside && d.mode == EXTRACT_COPY && !conv && (!lay.planar || d.channels == 1u) && d.channels == C;
            const bool wide_area = crop_inside && d.mode == EXTRACT_AREA && d.channels == 1u;
            for (uint32_t tid = 0; tid < 256u; ++tid) {
                const uint32_t lane = tid & 63u;
                for (uint32_t r = by * EXTRACT_BLOCK_H + (tid >> 6); r < std::min((by + 1u) * EXTRACT_BLOCK_H, R); r += 4u) {
                    const uint64_t row_at = d.dst_off + (uint64_t)r * B;
                    const uint32_t mis = (uint32_t)((dst_mod + row_at) & 3u);
                    const int32_t b0 = (int32_t)((bx * EXTRACT_BLOCK_SLOTS + lane) * 4u) - (int32_t)mis;
                    const int32_t blo = std::max(b0, 0), bhi = std::min(b0 + 4, (int32_t)B);
                    if (blo >= bhi) continue;
                    if (bhi - blo == 4) CHECK(((dst_mod + row_at + (uint64_t)b0) & 3u) == 0u);   // a whole slot is an aligned dword
                    uint32_t cpl = 0, y = r;
                    if (lay.planar) {
                        cpl = r / lay.out_h;
                        y = r - cpl * lay.out_h;
                    }
                    CHECK(y < lay.out_h && cpl < C);
                    int yi0, yi1;
                    if (d.mode == EXTRACT_COPY) yi0 = yi1 = (int)y;
                    else if (d.mode == EXTRACT_AREA) { yi0 = 2 * (int)y; yi1 = yi0 + 1; }
                    else { yi0 = sl.taps[(size_t)d.ytab + y].i0; yi1 = sl.taps[(size_t)d.ytab + y].i1; }
                    const int ys0 = clampi(d.y0 + yi0, d.fh - 1), ys1 = clampi(d.y0 + yi1, d.fh - 1);
                    if (bhi - blo == 4 && wide_copy) {   // four bytes of the crop row: inside the crop, so inside the frame's row
                        CHECK((uint32_t)b0 + 4u <= d.cw * d.channels && ys0 == d.y0 + yi0);
                        const uint8_t* q = f.data + (size_t)ys0 * (size_t)f.stride + (size_t)d.x0 * d.channels + (uint32_t)b0;
                        for (int k = 0; k < 4; ++k) sink = sink + q[k];
                    } else if (bhi - blo == 4 && wide_area) {   // eight bytes of two crop rows
                        CHECK(2u * (uint32_t)b0 + 8u <= d.cw && ys0 == d.y0 + yi0 && ys1 == d.y0 + yi1);
                        for (int ys : {ys0, ys1}) {
                            const uint8_t* q = f.data + (size_t)ys * (size_t)f.stride + (size_t)d.x0 + 2u * (uint32_t)b0;
                            for (int k = 0; k < 8; ++k) sink = sink + q[k];
                        }
                    }
                    for (int32_t b = blo; b < bhi; ++b) {
                        CHECK(covered[(size_t)(row_at + (uint64_t)b)] == 0);   // no byte twice
                        covered[(size_t)(row_at + (uint64_t)b)] = 1;
                        uint32_t x = (uint32_t)b, c = cpl;
                        if (!lay.planar && C > 1u) {
                            x = (uint32_t)b / C;
                            c = (uint32_t)b - x * C;
                        }
                        CHECK(x < lay.out_w && c < C);
                        int xi0, xi1;
                        if (d.mode == EXTRACT_COPY) xi0 = xi1 = (int)x;
                        else if (d.mode == EXTRACT_AREA) { xi0 = 2 * (int)x; xi1 = xi0 + 1; }
                        else { xi0 = sl.taps[(size_t)d.xtab + x].i0; xi1 = sl.taps[(size_t)d.xtab + x].i1; }
                        CHECK((uint32_t)xi1 < d.cw && (uint32_t)yi1 < d.ch);
                        const int xs0 = clampi(d.x0 + xi0, d.fw - 1), xs1 = clampi(d.x0 + xi1, d.fw - 1);
                        read_px(f, xs0, ys0, c, conv);
                        read_px(f, xs1, ys0, c, conv);
                        read_px(f, xs0, ys1, c, conv);
                        read_px(f, xs1, ys1, c, conv);
                    }
                }
            }
        }
        first = end;
    }
    for (uint64_t b = 0; b < bytes; ++b) CHECK(covered[(size_t)b] == 1);   // every byte of every region, once
    if (max_frames == 0 && n > 0) CHECK(slices == 1);
}

static vj_extract_params params(int ow, int oh, double sx, double sy, double margin, uint32_t flags, uint32_t reserved = 0) {
    vj_extract_params p;
    memset(&p, 0xff, sizeof(p));
    vj_extract_default(&p);
    CHECK(p.out_w == 0 && p.out_h == 0 && p.sx == 1 && p.sy == 1 && p.margin == 0 && p.flags == 0u && p.reserved == 0u);
    p.out_w = ow;
    p.out_h = oh;
    p.sx = sx;
    p.sy = sy;
    p.margin = margin;
    p.flags = flags;
    p.reserved = reserved;
    return p;
}

// regions of a 37 x 29 frame: inside, over each side and corner, wholly outside, the whole frame
static std::vector<vj_roi> regions_on(int frame) {
    return {{frame, 8, 6, 20, 17}, {frame, 9, 6, 20, 17}, {frame, 3, 4, 1, 1}, {frame, 5, 5, 2, 3}, {frame, 4, 7, 5, 5},
            {frame, -5, 8, 10, 10}, {frame, 30, 8, 10, 10}, {frame, 8, -5, 10, 10}, {frame, 8, 25, 10, 10},
            {frame, -3, -3, 10, 10}, {frame, 30, -3, 10, 10}, {frame, -3, 22, 10, 10}, {frame, 30, 22, 10, 10},
            {frame, 100, 100, 6, 6}, {frame, -40, 3, 6, 6}, {frame, 0, 0, 37, 29}};
}

int main() {
    for (int ch : {1, 3, 4}) {
        Frames fr;
        fr.add(37, 29, ch, 0);
        fr.add(37, 29, ch, 5);
        fr.add(9, 4, ch, 1);
        std::vector<vj_roi> regions = regions_on(0);
        for (const vj_roi& r : regions_on(1)) regions.push_back(r);
        regions.push_back(vj_roi{2, 0, 0, 9, 4});
        regions.push_back(vj_roi{0, 1, 1, 7, 7});
        regions.push_back(vj_roi{2, -2, -2, 13, 8});
        for (uint32_t flags : {0u, (uint32_t)VJ_EXTRACT_GRAY, (uint32_t)VJ_EXTRACT_PLANAR, (uint32_t)(VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR)})
            for (uint32_t mod = 0; mod < 4u; ++mod) {
                const size_t per = mod == 0u ? 0 : mod == 1u ? 1 : 2;
                plan_all(fr, regions, params(10, 10, 1, 1, 0, flags), per, mod);        // copies among them
                plan_all(fr, regions, params(5, 5, 1, 1, 0, flags), per, mod);          // the 2 x 2 mean of the 10 x 10 regions
                plan_all(fr, regions, params(20, 17, 1, 1, 0, flags), per, mod);
                plan_all(fr, regions, params(10, 17, 1, 1, 0, flags), per, mod);        // half on one axis only: bilinear
                plan_all(fr, regions, params(24, 24, 0.5, 0.5, 0.25, flags), per, mod); // ties and a margin
                plan_all(fr, regions, params(7, 3, 1.8, 1.8, 0.1, flags), per, mod);
                plan_all(fr, regions, params(1, 1, 0, 0, 0, flags), per, mod);
            }
        for (int w : {1, 2, 3, 4, 5, 6, 7, 8, 9, 21, 63, 64, 65, 85, 86, 255, 256, 257})
            for (int h : {1, 2, 5}) plan_all(fr, regions, params(w, h, 1, 1, 0, w % 2 ? 0u : (uint32_t)VJ_EXTRACT_PLANAR), 0, (uint32_t)(w + h) & 3u);
        plan_all(fr, {}, params(4, 4, 1, 1, 0, 0), 0, 0);
    }
    {   // frames of mixed channel counts: with VJ_EXTRACT_GRAY only
        Frames fr;
        fr.add(37, 29, 1, 3);
        fr.add(37, 29, 3, 0);
        fr.add(37, 29, 4, 1);
        std::vector<vj_roi> regions;
        for (int f = 0; f < 3; ++f)
            for (const vj_roi& r : regions_on(f)) regions.push_back(r);
        for (size_t per : {(size_t)0, (size_t)1, (size_t)2}) {
            plan_all(fr, regions, params(10, 10, 1, 1, 0, VJ_EXTRACT_GRAY), per, 1);
            plan_all(fr, regions, params(5, 5, 1, 1, 0.1, VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR), per, 3);
        }
        const vj_extract_params p = params(5, 5, 1, 1, 0, 0);
        std::vector<vj_roi> src(regions.size());
        int c = 0;
        uint64_t bytes = 5;
        CHECK(vj_extract_layout(fr.im.data(), 3, regions.data(), (int)regions.size(), &p, src.data(), &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "region 16") != nullptr && strstr(vj_last_error(), "channels") != nullptr);
    }
    {   // the ties: 5 x 0.5 gives 2, 7 x 0.5 gives 4
        Frames fr;
        fr.add(40, 30, 1, 0);
        const std::vector<vj_roi> regions = {{0, 5, 7, 5, 7}, {0, 7, 5, 7, 5}, {0, 1, 3, 1, 3}};
        const vj_extract_params p = params(3, 3, 0.5, 0.5, 0, 0);
        vj_roi src[3];
        int c = 0;
        uint64_t bytes = 0;
        CHECK(vj_extract_layout(fr.im.data(), 1, regions.data(), 3, &p, src, &c, &bytes) == VJ_OK && c == 1 && bytes == 27u);
        CHECK(src[0].x == 2 && src[0].y == 4 && src[0].w == 2 && src[0].h == 4 && src[1].x == 4 && src[1].y == 2 && src[1].w == 4 && src[1].h == 2);
        CHECK(src[2].x == 0 && src[2].y == 2 && src[2].w == 1 && src[2].h == 2);
        plan_all(fr, regions, p, 0, 2);
    }

    // ---- the error cases
    Frames fr;
    fr.add(37, 29, 3, 0);
    fr.add(9, 4, 3, 2);
    const std::vector<vj_roi> good = {{0, 0, 0, 4, 4}, {1, 1, 1, 2, 2}};
    const vj_extract_params ok = params(4, 4, 1, 1, 0, 0);
    vj_roi src[8];
    int c = 0;
    uint64_t bytes = 0;
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, &ok, src, &c, &bytes) == VJ_OK && c == 3 && bytes == 96u);
    CHECK(vj_extract_layout(nullptr, 2, good.data(), 2, &ok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, nullptr, 2, &ok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, nullptr, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, &ok, nullptr, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, &ok, src, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, &ok, src, &c, nullptr) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), -1, good.data(), 2, &ok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), -1, &ok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_layout(nullptr, 0, nullptr, 0, &ok, nullptr, &c, &bytes) == VJ_OK && bytes == 0);
    const vj_image bad_f[] = {{nullptr, 4, 4, 4, 0, 1}, {fr.im[0].data, 0, 4, 4, 0, 1}, {fr.im[0].data, 4, -1, 4, 0, 1}, {fr.im[0].data, 4, 4, 3, 0, 1},
                              {fr.im[0].data, 4, 4, 11, 0, 3}, {fr.im[0].data, 4, 4, 8, 0, 2}};
    for (const vj_image& b : bad_f) {
        const std::vector<vj_image> v = {fr.im[0], fr.im[1], b};
        bytes = 9;
        CHECK(vj_extract_layout(v.data(), 3, good.data(), 2, &ok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr);
    }
    for (const vj_roi& b : {vj_roi{2, 0, 0, 4, 4}, vj_roi{-1, 0, 0, 4, 4}, vj_roi{0, 0, 0, 0, 4}, vj_roi{0, 0, 0, 4, 0}, vj_roi{1, 0, 0, -3, 4}}) {
        const std::vector<vj_roi> v = {good[0], good[1], b};
        CHECK(vj_extract_layout(fr.im.data(), 2, v.data(), 3, &ok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "region 2") != nullptr);
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct { vj_extract_params p; const char* word; } bad_p[] = {
        {params(0, 4, 1, 1, 0, 0), "out_w"}, {params(4, 0, 1, 1, 0, 0), "out_h"}, {params(-4, 4, 1, 1, 0, 0), "out_w"}, {params(4, -1, 1, 1, 0, 0), "out_h"},
        {params(4, 4, -0.5, 1, 0, 0), "sx"}, {params(4, 4, 1, -0.5, 0, 0), "sy"}, {params(4, 4, 1, 1, -0.1, 0), "margin"},
        {params(4, 4, inf, 1, 0, 0), "sx"}, {params(4, 4, 1, nan, 0, 0), "sy"}, {params(4, 4, nan, nan, 0, 0), "sx"}, {params(4, 4, 1, 1, inf, 0), "margin"},
        {params(4, 4, 1, 1, nan, 0), "margin"}, {params(4, 4, 1, 1, 0, 4u), "flags"}, {params(4, 4, 1, 1, 0, 0x80000001u), "flags"},
        {params(4, 4, 1, 1, 0, 0, 1u), "reserved"}};
    for (const auto& b : bad_p) {
        CHECK(vj_extract_layout(fr.im.data(), 2, good.data(), 2, &b.p, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), b.word) != nullptr);
        CHECK(vj_extract_layout(nullptr, 0, nullptr, 0, &b.p, nullptr, &c, &bytes) == VJ_ERR_ARG);
    }
    // ---- the limits: sides up to 65535, coordinates within +-2^24, work units within a 32-bit index
    {
        const vj_roi big = {0, 0, 0, 65535, 65535};
        vj_extract_params p = params(65535, 1, 1, 1, 0, 0);
        CHECK(vj_extract_layout(fr.im.data(), 2, &big, 1, &p, src, &c, &bytes) == VJ_OK && bytes == 65535ull * 3ull);
        const vj_roi far_ok = {0, -(1 << 24), 1 << 23, 1, 1};
        CHECK(vj_extract_layout(fr.im.data(), 2, &far_ok, 1, &ok, src, &c, &bytes) == VJ_OK);
        struct { vj_roi r; vj_extract_params p; const char* word; } lim[] = {
            {{0, 0, 0, 4, 4}, params(65536, 4, 1, 1, 0, 0), "65535"}, {{0, 0, 0, 4, 4}, params(4, 65536, 1, 1, 0, 0), "65535"},
            {{0, 0, 0, 4, 4}, params(2147483647, 2147483647, 1, 1, 0, 0), "65535"},
            {{0, 0, 0, 65536, 4}, ok, "65535"}, {{0, 0, 0, 4, 65536}, ok, "65535"}, {{0, 0, 0, 2147483647, 2147483647}, ok, "65535"},
            {{0, 0, 0, 40000, 4}, params(4, 4, 2, 1, 0, 0), "65535"}, {{0, 0, 0, 4, 4}, params(4, 4, 1, 1e300, 0, 0), "65535"},
            {{0, 0, 0, 40000, 4}, params(4, 4, 1, 1, 0.5, 0), "65535"}, {{0, 0, 0, 4, 4}, params(4, 4, 1, 1, 1e300, 0), "65535"},
            {{0, (1 << 24) + 1, 0, 4, 4}, ok, "2^24"}, {{0, 0, -(1 << 24) - 1, 4, 4}, ok, "2^24"}, {{0, -2147483647 - 1, 2147483647, 4, 4}, ok, "2^24"},
            {{0, 1 << 23, 0, 4, 4}, params(4, 4, 3, 1, 0, 0), "2^24"}, {{0, 1 << 24, 0, 4, 4}, ok, "2^24"},
            {{0, -(1 << 24), 0, 4, 4}, params(4, 4, 1, 1, 0.5, 0), "2^24"}, {{0, 5, 5, 4, 4}, params(4, 4, 1e300, 1, 0, 0), "65535"}};
        for (const auto& b : lim) {
            const std::vector<vj_roi> v = {good[0], b.r};
            CHECK(vj_extract_layout(fr.im.data(), 2, v.data(), 2, &b.p, src, &c, &bytes) == VJ_ERR_LIMIT && bytes == 0);
            CHECK(strstr(vj_last_error(), b.word) != nullptr);
        }
        std::vector<vj_roi> many(2041, vj_roi{0, 0, 0, 2, 2});
        std::vector<vj_roi> src_many(many.size());
        p = params(65535, 65535, 1, 1, 0, VJ_EXTRACT_GRAY);   // 257 x 4096 blocks per region: 2040 regions fit
        CHECK(vj_extract_layout(fr.im.data(), 2, many.data(), 2041, &p, src_many.data(), &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "work units") != nullptr);
        CHECK(vj_extract_layout(fr.im.data(), 2, many.data(), 2040, &p, src_many.data(), &c, &bytes) == VJ_OK && c == 1);
    }
    // ---- a device-resident source that overlaps the destination (vj_extract checks it with vj_preprocess's function)
    {
        uint8_t* const base = (uint8_t*)(uintptr_t)0x10000;   // (addresses only: nothing is read)
        std::vector<vj_image> f = {{base + 4096, 16, 4, 16, 1, 1}, {base + 8192, 5, 3, 20, 1, 3}, {base, 16, 4, 16, 0, 1}};
        CHECK(prep_check_overlap(f.data(), 3, base, 4096) == VJ_OK);
        CHECK(prep_check_overlap(f.data(), 3, base + 1, 4096) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr);
        CHECK(prep_check_overlap(f.data(), 3, base + 8192 + 2 * 20 + 14, 1) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 1") != nullptr);
        CHECK(prep_check_overlap(f.data(), 3, base + 8192 + 2 * 20 + 15, 1) == VJ_OK);
    }
    printf("extract_asan_driver: OK\n");
    return 0;
}
