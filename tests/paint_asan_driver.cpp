// Sanitizer driver of the host planner of vj_paint (csrc/vj_paint_host.cpp: the argument checks and limits, the mapping and the
// clipping, the slices of whole frames, the region records bucketed by frame, their overlap lists, scratch offsets and work
// units): built by tests/test_sanitizers_paint.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/paint_asan_driver.cpp csrc/vj_paint_host.cpp csrc/vj_extract_host.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp
//       csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Frames of 1, 3 and 4 channels in heap blocks that END with their last row, their rows at every address
// mod 4; regions inside, across and outside the frames; every mode, with and without the ellipse; whole and in slices.  The work
// units are decoded as the kernels decode them (region from the unit prefix, then block, wave and lane, or band and column, or
// cell): the paint_apply units cover every byte of every K row exactly once — each byte is read, so ASan sees the access —, the
// phase-1 units every scratch element exactly once; the scratch ranges are disjoint and lie inside the reported bytes; the overlap
// lists equal a brute-force search; the slices hold whole frames.  Then the error cases.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_paint_host.hpp"

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
    void add(int w, int h, int ch, int pad, int off) {
        const int stride = w * ch + pad;
        const size_t bytes = (size_t)off + (size_t)(h - 1) * (size_t)stride + (size_t)w * ch;   // the block ends with the last row's last byte
        mem.emplace_back(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) mem.back()[i] = (uint8_t)(i * 7u + 1u);
        im.push_back(vj_image{mem.back().get() + off, w, h, stride, 0, ch});
    }
};

static volatile uint32_t sink;

template <bool PRE>
static uint32_t region_of(const std::vector<PaintRegionDev>& regs, uint32_t unit) {   // as paint_region_of
    uint32_t lo = 0, hi = (uint32_t)regs.size();
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((PRE ? regs[mid].pre_first : regs[mid].unit_first) <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

static void check_slice(const Frames& F, const PaintLayout& lay, const PaintSlice& sl, std::set<uintptr_t>* rows_mod4) {
    const size_t n = sl.recs.size();
    CHECK(sl.region.size() == n);
    // ordered by (frame, region index); every record's frame is one of the slice's
    for (size_t i = 0; i < n; ++i) {
        const vj_roi& k = lay.clipped[(size_t)sl.region[i]];
        CHECK(std::find(sl.frames.begin(), sl.frames.end(), k.frame) != sl.frames.end());
        CHECK(k.w > 0 && k.h > 0);
        if (i) {
            const vj_roi& q = lay.clipped[(size_t)sl.region[i - 1]];
            CHECK(q.frame < k.frame || (q.frame == k.frame && sl.region[i - 1] < sl.region[i]));
        }
        const PaintRegionDev& d = sl.recs[i];
        const vj_image& f = F.im[(size_t)k.frame];
        CHECK(d.frame == f.data && d.stride == (uint32_t)f.stride && d.row0 == 0 && d.fw == f.width && d.fh == f.height);
        CHECK(d.cx0 == k.x && d.cy0 == k.y && d.cx1 == k.x + k.w && d.cy1 == k.y + k.h);
        CHECK(d.cx0 >= 0 && d.cy0 >= 0 && d.cx1 <= f.width && d.cy1 <= f.height);
        CHECK(d.size == lay.sizes[(size_t)sl.region[i]]);
    }
    // the overlap lists against a brute-force search
    for (size_t i = 0; i < n; ++i) {
        std::vector<uint32_t> want;
        for (size_t j = i + 1; j < n; ++j) {
            const PaintRegionDev &a = sl.recs[i], &b = sl.recs[j];
            if (a.frame != b.frame) continue;
            bool meet = false;
            for (int y = a.cy0; y < a.cy1 && !meet; ++y)
                for (int x = a.cx0; x < a.cx1 && !meet; ++x) meet = x >= b.cx0 && x < b.cx1 && y >= b.cy0 && y < b.cy1;
            if (meet) want.push_back((uint32_t)j);
        }
        CHECK((size_t)sl.recs[i].ovl_first + sl.recs[i].ovl_count <= sl.overlaps.size());
        std::vector<uint32_t> got(sl.overlaps.begin() + sl.recs[i].ovl_first, sl.overlaps.begin() + sl.recs[i].ovl_first + sl.recs[i].ovl_count);
        CHECK(got == want);
    }
    // the scratch ranges: disjoint, inside the slice's bytes
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (const PaintRegionDev& d : sl.recs) {
        const uint64_t b = paint_scratch_bytes(lay.mode, (uint32_t)(d.cx1 - d.cx0), (uint32_t)(d.cy1 - d.cy0), d.channels, (uint32_t)std::max(d.size, 1));
        CHECK(d.scratch_off % 16u == 0u && d.scratch_off + b <= sl.scratch_bytes);
        if (b) ranges.emplace_back(d.scratch_off, d.scratch_off + b);
        CHECK((b != 0) == (lay.mode == PAINT_BLUR || lay.mode == PAINT_PIXELATE));
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i) CHECK(ranges[i - 1].second <= ranges[i].first);
    std::vector<uint8_t> scratch_hits((size_t)sl.scratch_bytes, 0);

    // paint_apply's units: every byte of every K row exactly once
    std::vector<std::vector<uint8_t>> hits(n);
    for (size_t i = 0; i < n; ++i) hits[i].assign((size_t)(sl.recs[i].cy1 - sl.recs[i].cy0) * (size_t)(sl.recs[i].cx1 - sl.recs[i].cx0) * sl.recs[i].channels, 0);
    for (uint32_t unit = 0; unit < sl.n_units; ++unit) {
        const uint32_t k = region_of<false>(sl.recs, unit);
        const PaintRegionDev& d = sl.recs[k];
        const uint32_t C = d.channels, kw = (uint32_t)(d.cx1 - d.cx0), kh = (uint32_t)(d.cy1 - d.cy0), B = kw * C;
        const uint32_t bpr = paint_row_blocks(B), u = unit - d.unit_first;
        CHECK(u < paint_apply_units(B, kh));
        const uint32_t by = u / bpr, bx = u - by * bpr;
        for (uint32_t wave = 0; wave < PAINT_WAVES; ++wave)
            for (uint32_t it = 0; it < PAINT_BLOCK_H / PAINT_WAVES; ++it) {
                const uint32_t r = by * PAINT_BLOCK_H + it * PAINT_WAVES + wave;
                if (r >= kh) continue;
                const uint8_t* drow = d.frame + (size_t)((uint32_t)(d.cy0 - d.row0) + r) * d.stride + (size_t)d.cx0 * C;
                const uint32_t m = (uint32_t)((uintptr_t)drow & 3u);
                rows_mod4->insert((uintptr_t)drow & 3u);
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const int32_t b0 = (int32_t)((bx * PAINT_BLOCK_SLOTS + lane) * 4u) - (int32_t)m;
                    const int32_t lo = std::max(b0, 0), hi = std::min(b0 + 4, (int32_t)B);
                    if (lo < hi && hi - lo == 4) CHECK(((uintptr_t)(drow + b0) & 3u) == 0u);   // a whole slot is an aligned dword
                    for (int32_t b = lo; b < hi; ++b) {
                        sink = sink + drow[b];
                        ++hits[k][(size_t)r * B + (size_t)b];
                    }
                }
            }
    }
    for (size_t i = 0; i < n; ++i)
        for (uint8_t h : hits[i]) CHECK(h == 1);

    // the phase-1 units: every scratch element of every region exactly once
    if (lay.mode == PAINT_BLUR || lay.mode == PAINT_PIXELATE) {
        for (uint32_t unit = 0; unit < sl.n_pre_units; ++unit) {
            const uint32_t k = region_of<true>(sl.recs, unit);
            const PaintRegionDev& d = sl.recs[k];
            const uint32_t C = d.channels, kw = (uint32_t)(d.cx1 - d.cx0), kh = (uint32_t)(d.cy1 - d.cy0), B = kw * C, u = unit - d.pre_first;
            if (lay.mode == PAINT_BLUR) {
                CHECK(u < paint_colsum_units(B, kh));
                const uint32_t cb = paint_col_blocks(B), band = u / cb, bx = u - band * cb;
                const int32_t r = d.size >> 1;
                for (uint32_t t = 0; t < 256u; ++t) {
                    const uint32_t col = bx * PAINT_BAND_COLS + t;
                    const uint32_t y0 = band * PAINT_BAND_H, y1 = std::min(y0 + PAINT_BAND_H, kh);
                    if (col >= B || y0 >= kh) continue;
                    const uint8_t* base = d.frame + (size_t)(d.cy0 - d.row0) * d.stride + (size_t)d.cx0 * C + col;
                    for (uint32_t y = y0; y < y1; ++y) {
                        // the rows the sliding window reads at y: the window's ends, clamped to K
                        sink = sink + base[(size_t)std::min((int32_t)y + r, (int32_t)kh - 1) * d.stride] + base[(size_t)std::max((int32_t)y - r, 0) * d.stride];
                        const uint64_t at = d.scratch_off + 2ull * ((uint64_t)y * B + col);
                        CHECK(at + 2u <= sl.scratch_bytes);
                        ++scratch_hits[(size_t)at];
                        ++scratch_hits[(size_t)at + 1u];
                    }
                }
            } else {
                const uint32_t s = (uint32_t)d.size, L = d.lanes;
                CHECK(L >= C && L <= 64u && (L & (L - 1u)) == 0u && L == paint_cell_lanes(s, C));
                CHECK(u < paint_cell_units(kw, kh, s, L));
                const uint32_t nx = paint_cells_x(kw, s), ny = paint_cells_x(kh, s), per_wave = 64u / L;
                for (uint32_t t = 0; t < 256u; ++t) {
                    const uint32_t lane = t & 63u, wave = t >> 6, sub = lane & (L - 1u);
                    const uint64_t cell = (uint64_t)u * (PAINT_WAVES * per_wave) + wave * per_wave + lane / L;
                    if (cell >= (uint64_t)nx * ny || sub >= C) continue;
                    const uint32_t j = (uint32_t)(cell / nx), i = (uint32_t)(cell - (uint64_t)j * nx);
                    const uint32_t x0 = i * s, y0 = j * s, cw = std::min(s, kw - x0), chh = std::min(s, kh - y0);
                    CHECK(cw > 0 && chh > 0);
                    const uint8_t* base = d.frame + (size_t)((uint32_t)(d.cy0 - d.row0) + y0) * d.stride + ((size_t)d.cx0 + x0) * C;
                    sink = sink + base[0] + base[(size_t)(chh - 1u) * d.stride + (size_t)cw * C - 1u];   // the cell's first and last byte
                    const uint64_t at = d.scratch_off + cell * C + sub;
                    CHECK(at < sl.scratch_bytes);
                    ++scratch_hits[(size_t)at];
                }
            }
        }
        for (const auto& rg : ranges)
            for (uint64_t at = rg.first; at < rg.second; ++at) CHECK(scratch_hits[(size_t)at] == 1);
        uint64_t used = 0;
        for (const auto& rg : ranges) used += rg.second - rg.first;
        uint64_t hit = 0;
        for (uint8_t h : scratch_hits) hit += h;
        CHECK(hit == used);
    } else {
        CHECK(sl.n_pre_units == 0u && sl.scratch_bytes == 0u);
    }
}

static void run_call(const Frames& F, const std::vector<vj_roi>& regions, const vj_paint_params& p, std::set<uintptr_t>* rows_mod4) {
    PaintLayout lay;
    CHECK(paint_layout(F.im.data(), (int)F.im.size(), regions.data(), (int)regions.size(), &p, &lay) == VJ_OK);
    CHECK(lay.clipped.size() == regions.size() && lay.sizes.size() == regions.size());
    for (size_t max_frames : {(size_t)0, (size_t)1, (size_t)2, (size_t)3}) {
        std::vector<int> seen_frames;
        std::vector<int> seen_regions;
        uint64_t scratch = 0, largest = 0;
        for (size_t first = 0; first < lay.touched.size();) {
            const size_t end = paint_slice_end(lay, first, max_frames);
            CHECK(end > first && end <= lay.touched.size() && (max_frames == 0 || end - first <= max_frames));
            PaintSlice sl;
            CHECK(paint_plan_slice(F.im.data(), lay, first, end, &sl) == VJ_OK);
            CHECK(sl.frames.size() == end - first);
            check_slice(F, lay, sl, rows_mod4);
            seen_frames.insert(seen_frames.end(), sl.frames.begin(), sl.frames.end());
            seen_regions.insert(seen_regions.end(), sl.region.begin(), sl.region.end());
            scratch += sl.scratch_bytes;
            largest = std::max(largest, sl.scratch_bytes);
            first = end;
        }
        // whole frames: every touched frame in exactly one slice, every region with a K in exactly one, with its frame
        CHECK(seen_frames == lay.touched);
        std::sort(seen_regions.begin(), seen_regions.end());
        std::vector<int> want;
        for (size_t r = 0; r < regions.size(); ++r)
            if (lay.clipped[r].w > 0) want.push_back((int)r);
        CHECK(seen_regions == want);
        CHECK(scratch == lay.scratch_bytes && largest <= lay.scratch_bytes && (max_frames != 0 || largest == lay.scratch_bytes));
    }
}

int main() {
    Frames F;
    // 1, 3 and 4 channels; pads and offsets that put the rows at every address mod 4
    F.add(37, 29, 1, 0, 0);
    F.add(37, 29, 3, 1, 1);
    F.add(37, 29, 4, 3, 2);
    F.add(300, 40, 3, 2, 3);
    F.add(9, 5, 1, 0, 1);      // a frame no region names
    F.add(70, 70, 4, 1, 0);
    std::vector<vj_roi> regions;
    const int frames_used[] = {3, 0, 2, 1, 5, 0, 3};   // mixed frame order
    for (int f : frames_used) {
        const int w = F.im[(size_t)f].width, h = F.im[(size_t)f].height;
        const vj_roi some[] = {{f, 3, 4, 1, 1}, {f, 20, 2, 1, 9}, {f, 9, 20, 11, 1}, {f, -5, 8, 10, 10}, {f, w - 7, 8, 10, 10}, {f, 8, -5, 10, 10},
                               {f, 8, h - 4, 10, 10}, {f, -3, -3, 10, 10}, {f, w - 7, h - 6, 10, 10}, {f, w + 50, h + 50, 6, 6}, {f, -40, 3, 6, 6},
                               {f, 0, 0, w, h}, {f, 2, 2, 20, 16}, {f, 10, 8, 22, 18}, {f, 6, 12, 12, 9}, {f, 2, 2, 20, 16}, {f, 1, 0, w - 1, 33}};
        regions.insert(regions.end(), std::begin(some), std::end(some));
    }
    std::set<uintptr_t> rows_mod4;
    for (int mode = 0; mode < 4; ++mode)
        for (uint32_t flags : {0u, (uint32_t)VJ_PAINT_ELLIPSE})
            for (int size : {0, 1, 2, 7, 64, 255}) {
                vj_paint_params p;
                vj_paint_default(&p);
                p.mode = mode;
                p.flags = flags;
                p.size = size;
                p.rel = 0.3;
                p.margin = size == 7 ? 0.25 : 0.0;
                p.sx = size == 2 ? 1.5 : 1.0;
                run_call(F, regions, p, &rows_mod4);
            }
    CHECK(rows_mod4.size() == 4u);

    // the layout entry point and the error cases
    {
        vj_paint_params p;
        vj_paint_default(&p);
        std::vector<vj_roi> k(regions.size());
        std::vector<int32_t> s(regions.size());
        uint64_t bytes = 1;
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), (int)regions.size(), &p, k.data(), s.data(), &bytes) == VJ_OK && bytes > 0);
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), nullptr, 0, &p, nullptr, nullptr, &bytes) == VJ_OK && bytes == 0);
        CHECK(vj_paint_layout(nullptr, 1, regions.data(), 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_ARG);
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &p, k.data(), s.data(), nullptr) == VJ_ERR_ARG);
        vj_paint_params q = p;
        q.mode = 4;
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &q, k.data(), s.data(), &bytes) == VJ_ERR_ARG);
        q = p;
        q.size = 256;
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &q, k.data(), s.data(), &bytes) == VJ_ERR_LIMIT);
        q = p;
        q.rel = 1e300;
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &q, k.data(), s.data(), &bytes) == VJ_ERR_LIMIT);
        q.mode = VJ_PAINT_OUTLINE;
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &q, k.data(), s.data(), &bytes) == VJ_OK && s[0] == 65536);
        const vj_roi huge = {0, 0, 0, 32768, 4}, far = {0, (1 << 24) + 1, 0, 4, 4}, none = {9, 0, 0, 4, 4};
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), &huge, 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_LIMIT);
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), &far, 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_LIMIT);
        CHECK(vj_paint_layout(F.im.data(), (int)F.im.size(), &none, 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_ARG);
        std::vector<vj_image> twice = F.im;
        twice.push_back(F.im[1]);
        CHECK(vj_paint_layout(twice.data(), (int)twice.size(), regions.data(), 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_ARG);
        twice.back().data += 5;
        CHECK(vj_paint_layout(twice.data(), (int)twice.size(), regions.data(), 1, &p, k.data(), s.data(), &bytes) == VJ_ERR_ARG);
        twice.back().on_device = 1;   // another address space: no overlap
        CHECK(vj_paint_layout(twice.data(), (int)twice.size(), regions.data(), 1, &p, k.data(), s.data(), &bytes) == VJ_OK);
        PaintLayout lay;
        CHECK(paint_layout(F.im.data(), (int)F.im.size(), regions.data(), (int)regions.size(), &p, &lay) == VJ_OK);
        PaintSlice sl;
        CHECK(paint_plan_slice(F.im.data(), lay, 2, lay.touched.size() + 1, &sl) == VJ_ERR_ARG);
    }
    printf("paint_asan_driver: OK\n");
    return 0;
}
