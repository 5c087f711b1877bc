// Sanitizer driver of the host planner of vj_paint_yuv (csrc/vj_paint_yuv_host.cpp on top of vj_paint_host.cpp and vj_yuv_host.cpp):
// built by tests/test_sanitizers_paint_yuv.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/paint_yuv_asan_driver.cpp csrc/vj_paint_yuv_host.cpp csrc/vj_paint_host.cpp csrc/vj_yuv_host.cpp csrc/vj_extract_host.cpp
//       csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  NV12, NV21 and I420 frames whose planes lie in heap blocks that END with their last row, at every address
// mod 4; regions inside, across and outside the frames; every mode, with and without the ellipse; whole and in slices of 1, 2 and 3
// frames.  The work units are decoded as the kernels decode them (record from the unit prefix, then block, wave and lane, or band
// and column, or cell): the paint_yuv_apply units cover every byte of every K and Kc row exactly once — each byte is read, so ASan
// sees the access —, the phase-1 units every scratch element exactly once; the scratch ranges are disjoint and lie inside the
// reported bytes; the overlap lists equal a brute-force search over the planes' rectangles; the row sets of the rectangles equal
// the painted-set test sample by sample; the slices hold whole frames.  Then the error cases.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_paint_yuv_host.hpp"

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
    std::vector<vj_yuv_image> im;
    uint8_t* plane(int row_bytes, int rows, int stride, int off) {
        const size_t bytes = (size_t)off + (size_t)(rows - 1) * (size_t)stride + (size_t)row_bytes;   // the block ends with the last row's last byte
        mem.emplace_back(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) mem.back()[i] = (uint8_t)(i * 7u + 1u);
        return mem.back().get() + off;
    }
    void add(int w, int h, int layout, int pad, int off) {
        vj_yuv_image f;
        memset(&f, 0, sizeof(f));
        f.width = w, f.height = h, f.layout = layout, f.on_device = 0;
        const int crow = layout == VJ_YUV_I420 ? w / 2 : w;
        f.y_stride = w + pad, f.c_stride = crow + ((pad + 1) % 4);
        f.y = plane(w, h, f.y_stride, off);
        f.c0 = plane(crow, h / 2, f.c_stride, (off + 1) % 4);
        f.c1 = layout == VJ_YUV_I420 ? plane(crow, h / 2, f.c_stride, (off + 2) % 4) : nullptr;
        im.push_back(f);
    }
};

static volatile uint32_t sink;

template <bool PRE>
static uint32_t rec_of(const std::vector<PaintYuvRec>& recs, uint32_t unit) {   // as paint_yuv_rec_of
    uint32_t lo = 0, hi = (uint32_t)recs.size();
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((PRE ? recs[mid].pre_first : recs[mid].unit_first) <= unit) lo = mid;
        else hi = mid;
    }
    return lo;
}

static void check_slice(const Frames& F, const PaintYuvLayout& lay, const PaintYuvSlice& sl, std::set<uintptr_t> rows_mod4[3], bool row_sets) {
    const PaintLayout& L = lay.luma;
    const size_t n = sl.recs.size();
    CHECK(sl.region.size() == n);
    // ordered by (frame, region index, plane); every record's frame is one of the slice's; the rectangles are K and Kc
    for (size_t i = 0; i < n; ++i) {
        const vj_roi &k = L.clipped[(size_t)sl.region[i]], &c = lay.chroma[(size_t)sl.region[i]];
        CHECK(std::find(sl.frames.begin(), sl.frames.end(), k.frame) != sl.frames.end());
        CHECK(k.w > 0 && k.h > 0 && c.w > 0 && c.h > 0 && c.frame == k.frame);
        const PaintYuvRec& d = sl.recs[i];
        if (i) {
            const vj_roi& q = L.clipped[(size_t)sl.region[i - 1]];
            CHECK(q.frame < k.frame || (q.frame == k.frame && sl.region[i - 1] < sl.region[i]) ||
                  (sl.region[i - 1] == sl.region[i] && sl.recs[i - 1].plane_id < d.plane_id));
        }
        const vj_yuv_image& f = F.im[(size_t)k.frame];
        const PaintYuvPlane q = paint_yuv_plane(f, d.plane_id);
        CHECK(q.p && d.plane == q.p && d.stride == q.stride && d.comps == q.comps && d.row0 == 0 && d.pw == q.w && d.ph == q.h);
        CHECK(d.comps == (d.plane_id == PAINT_YUV_PLANE_C0 && f.layout != VJ_YUV_I420 ? 2u : 1u) && d.sub == (d.plane_id != PAINT_YUV_PLANE_Y ? 1u : 0u));
        CHECK(d.cx0 == k.x && d.cy0 == k.y && d.cx1 == k.x + k.w && d.cy1 == k.y + k.h && d.size == L.sizes[(size_t)sl.region[i]]);
        const vj_roi& pr = d.sub ? c : k;
        CHECK(d.kx0 == pr.x && d.ky0 == pr.y && d.kx1 == pr.x + pr.w && d.ky1 == pr.y + pr.h);
        CHECK(d.kx0 >= 0 && d.ky0 >= 0 && d.kx1 <= d.pw && d.ky1 <= d.ph);
        if (d.sub) {
            CHECK(d.kx0 == d.cx0 >> 1 && d.ky0 == d.cy0 >> 1 && d.kx1 == (d.cx1 + 1) >> 1 && d.ky1 == (d.cy1 + 1) >> 1);
            if (L.mode == PAINT_PIXELATE) CHECK(d.psize == (d.size + 1) >> 1);
            if (L.mode == PAINT_BLUR) CHECK(d.psize == std::max((d.size >> 1) | 1, 3) && (d.psize & 1) && d.psize <= d.size);
        } else if (L.mode == PAINT_PIXELATE || L.mode == PAINT_BLUR) {
            CHECK(d.psize == d.size);
        }
        // rectangles: the row sets equal the painted-set test, sample by sample, a margin around the rectangle included
        const PaintGeom g = paint_geom(&d);
        for (int y = d.ky0 - 1; row_sets && y <= d.ky1; ++y) {
            const PaintRowSet rs = paint_yuv_row_set(g, d.sub, L.mode, y);
            for (int x = d.kx0 - 2; x <= d.kx1 + 1; ++x) CHECK(paint_yuv_in_row(rs, x) == paint_yuv_in_set(g, d.sub, x, y, L.mode, false));
        }
    }
    // every region of the slice has a record for every plane of its frame
    for (size_t i = 0; i < n;) {
        const vj_yuv_image& f = F.im[(size_t)L.clipped[(size_t)sl.region[i]].frame];
        const size_t planes = f.layout == VJ_YUV_I420 ? 3u : 2u;
        CHECK(i + planes <= n);
        for (size_t j = 0; j < planes; ++j) CHECK(sl.region[i + j] == sl.region[i] && sl.recs[i + j].plane_id == (uint32_t)j);
        i += planes;
    }
    // the overlap lists against a brute-force search over the samples of the rectangles
    for (size_t i = 0; i < n; ++i) {
        std::vector<uint32_t> want;
        for (size_t j = i + 1; j < n; ++j) {
            const PaintYuvRec &a = sl.recs[i], &b = sl.recs[j];
            if (a.plane != b.plane) continue;
            bool meet = false;
            for (int y = a.ky0; y < a.ky1 && !meet; ++y)
                for (int x = a.kx0; x < a.kx1 && !meet; ++x) meet = x >= b.kx0 && x < b.kx1 && y >= b.ky0 && y < b.ky1;
            if (meet) want.push_back((uint32_t)j);
        }
        CHECK((size_t)sl.recs[i].ovl_first + sl.recs[i].ovl_count <= sl.overlaps.size());
        std::vector<uint32_t> got(sl.overlaps.begin() + sl.recs[i].ovl_first, sl.overlaps.begin() + sl.recs[i].ovl_first + sl.recs[i].ovl_count);
        CHECK(got == want);
    }
    // the scratch ranges: disjoint, inside the slice's bytes
    std::vector<std::pair<uint64_t, uint64_t>> ranges;
    for (const PaintYuvRec& d : sl.recs) {
        const uint64_t b = paint_scratch_bytes(L.mode, (uint32_t)(d.kx1 - d.kx0), (uint32_t)(d.ky1 - d.ky0), d.comps, (uint32_t)std::max(d.psize, 1));
        CHECK(d.scratch_off % 16u == 0u && d.scratch_off + b <= sl.scratch_bytes);
        if (b) ranges.emplace_back(d.scratch_off, d.scratch_off + b);
        CHECK((b != 0) == (L.mode == PAINT_BLUR || L.mode == PAINT_PIXELATE));
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 1; i < ranges.size(); ++i) CHECK(ranges[i - 1].second <= ranges[i].first);
    std::vector<uint8_t> scratch_hits((size_t)sl.scratch_bytes, 0);

    // paint_yuv_apply's units: every byte of every rectangle row exactly once
    std::vector<std::vector<uint8_t>> hits(n);
    for (size_t i = 0; i < n; ++i) hits[i].assign((size_t)(sl.recs[i].ky1 - sl.recs[i].ky0) * (size_t)(sl.recs[i].kx1 - sl.recs[i].kx0) * sl.recs[i].comps, 0);
    for (uint32_t unit = 0; unit < sl.n_units; ++unit) {
        const uint32_t k = rec_of<false>(sl.recs, unit);
        const PaintYuvRec& d = sl.recs[k];
        const uint32_t C = d.comps, sh = C - 1u, kw = (uint32_t)(d.kx1 - d.kx0), kh = (uint32_t)(d.ky1 - d.ky0), B = kw * C;
        const uint32_t bpr = paint_row_blocks(B), u = unit - d.unit_first;
        CHECK(u < paint_apply_units(B, kh));
        const uint32_t by = u / bpr, bx = u - by * bpr;
        const int32_t rad = d.psize >> 1;
        for (uint32_t wave = 0; wave < PAINT_WAVES; ++wave)
            for (uint32_t it = 0; it < PAINT_BLOCK_H / PAINT_WAVES; ++it) {
                const uint32_t r = by * PAINT_BLOCK_H + it * PAINT_WAVES + wave;
                if (r >= kh) continue;
                const uint8_t* drow = d.plane + (size_t)((uint32_t)(d.ky0 - d.row0) + r) * d.stride + (size_t)d.kx0 * C;
                const uint32_t m = (uint32_t)((uintptr_t)drow & 3u);
                rows_mod4[d.plane_id].insert((uintptr_t)drow & 3u);
                if (L.mode == PAINT_BLUR) {   // the wave's staged prefix sums fit the LDS array
                    const int32_t wb0 = std::max((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m, 0);
                    const int32_t wb1 = std::min((int32_t)(bx * PAINT_BLOCK_SLOTS * 4u) - (int32_t)m + (int32_t)(PAINT_BLOCK_SLOTS * 4u), (int32_t)B);
                    if (wb0 < wb1) {
                        const int32_t q_lo = std::max((wb0 >> sh) - rad, 0), q_hi = std::min(((wb1 - 1) >> sh) + rad, (int32_t)kw - 1);
                        CHECK(((uint32_t)(q_hi - q_lo + 1) << sh) <= PAINT_YUV_PREFIX_MAX);
                    }
                }
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const int32_t b0 = (int32_t)((bx * PAINT_BLOCK_SLOTS + lane) * 4u) - (int32_t)m;
                    const int32_t lo = std::max(b0, 0), hi = std::min(b0 + 4, (int32_t)B);
                    if (lo >= hi) continue;
                    if (hi - lo == 4) CHECK(((uintptr_t)(drow + b0) & 3u) == 0u);   // a whole slot is an aligned dword
                    CHECK(((hi - 1) >> sh) - (lo >> sh) <= 3);                          // at most four samples: the lane's ownership bits
                    for (int32_t b = lo; b < hi; ++b) {
                        sink = sink + drow[b];
                        ++hits[k][(size_t)r * B + (size_t)b];
                    }
                }
            }
    }
    for (size_t i = 0; i < n; ++i)
        for (uint8_t h : hits[i]) CHECK(h == 1);

    // the phase-1 units: every scratch element of every record exactly once
    if (L.mode == PAINT_BLUR || L.mode == PAINT_PIXELATE) {
        for (uint32_t unit = 0; unit < sl.n_pre_units; ++unit) {
            const uint32_t k = rec_of<true>(sl.recs, unit);
            const PaintYuvRec& d = sl.recs[k];
            const uint32_t C = d.comps, kw = (uint32_t)(d.kx1 - d.kx0), kh = (uint32_t)(d.ky1 - d.ky0), B = kw * C, u = unit - d.pre_first;
            if (L.mode == PAINT_BLUR) {
                CHECK(u < paint_colsum_units(B, kh));
                const uint32_t cb = paint_col_blocks(B), band = u / cb, bx = u - band * cb;
                const int32_t r = d.psize >> 1;
                for (uint32_t t = 0; t < 256u; ++t) {
                    const uint32_t col = bx * PAINT_BAND_COLS + t;
                    const uint32_t y0 = band * PAINT_BAND_H, y1 = std::min(y0 + PAINT_BAND_H, kh);
                    if (col >= B || y0 >= kh) continue;
                    const uint8_t* base = d.plane + (size_t)(d.ky0 - d.row0) * d.stride + (size_t)d.kx0 * C + col;
                    for (uint32_t y = y0; y < y1; ++y) {
                        sink = sink + base[(size_t)std::min((int32_t)y + r, (int32_t)kh - 1) * d.stride] + base[(size_t)std::max((int32_t)y - r, 0) * d.stride];
                        const uint64_t at = d.scratch_off + 2ull * ((uint64_t)y * B + col);
                        CHECK(at + 2u <= sl.scratch_bytes);
                        ++scratch_hits[(size_t)at];
                        ++scratch_hits[(size_t)at + 1u];
                    }
                }
            } else {
                const uint32_t s = (uint32_t)d.psize, Ln = d.lanes;
                CHECK(Ln >= C && Ln <= 64u && (Ln & (Ln - 1u)) == 0u && Ln == paint_cell_lanes(s, C));
                CHECK(u < paint_cell_units(kw, kh, s, Ln));
                const uint32_t nx = paint_cells_x(kw, s), ny = paint_cells_x(kh, s), per_wave = 64u / Ln;
                for (uint32_t t = 0; t < 256u; ++t) {
                    const uint32_t lane = t & 63u, wave = t >> 6, sub = lane & (Ln - 1u);
                    const uint64_t cell = (uint64_t)u * (PAINT_WAVES * per_wave) + wave * per_wave + lane / Ln;
                    if (cell >= (uint64_t)nx * ny || sub >= C) continue;
                    const uint32_t j = (uint32_t)(cell / nx), i = (uint32_t)(cell - (uint64_t)j * nx);
                    const uint32_t x0 = i * s, y0 = j * s, cw = std::min(s, kw - x0), chh = std::min(s, kh - y0);
                    CHECK(cw > 0 && chh > 0);
                    const uint8_t* base = d.plane + (size_t)((uint32_t)(d.ky0 - d.row0) + y0) * d.stride + ((size_t)d.kx0 + x0) * C;
                    sink = sink + base[0] + base[(size_t)(chh - 1u) * d.stride + (size_t)cw * C - 1u];   // the cell's first and last byte
                    const uint64_t at = d.scratch_off + cell * C + sub;
                    CHECK(at < sl.scratch_bytes);
                    ++scratch_hits[(size_t)at];
                }
            }
        }
        for (const auto& rg : ranges)
            for (uint64_t at = rg.first; at < rg.second; ++at) CHECK(scratch_hits[(size_t)at] == 1);
        uint64_t used = 0, hit = 0;
        for (const auto& rg : ranges) used += rg.second - rg.first;
        for (uint8_t h : scratch_hits) hit += h;
        CHECK(hit == used);
    } else {
        CHECK(sl.n_pre_units == 0u && sl.scratch_bytes == 0u);
    }
}

static void run_call(const Frames& F, const std::vector<vj_roi>& regions, const vj_paint_params& p, std::set<uintptr_t> rows_mod4[3]) {
    PaintYuvLayout lay;
    CHECK(paint_yuv_layout(F.im.data(), (int)F.im.size(), regions.data(), (int)regions.size(), &p, &lay) == VJ_OK);
    const PaintLayout& L = lay.luma;
    CHECK(L.clipped.size() == regions.size() && lay.chroma.size() == regions.size() && lay.csizes.size() == regions.size());
    for (size_t max_frames : {(size_t)0, (size_t)1, (size_t)2, (size_t)3}) {
        std::vector<int> seen_frames, seen_regions;
        uint64_t scratch = 0, largest = 0;
        for (size_t first = 0; first < L.touched.size();) {
            const size_t end = paint_slice_end(L, first, max_frames);
            CHECK(end > first && end <= L.touched.size() && (max_frames == 0 || end - first <= max_frames));
            PaintYuvSlice sl;
            CHECK(paint_yuv_plan_slice(F.im.data(), lay, first, end, &sl) == VJ_OK);
            CHECK(sl.frames.size() == end - first);
            check_slice(F, lay, sl, rows_mod4, max_frames == 0 && !L.ellipse);   // (the row sets are the rectangles': once per call)
            seen_frames.insert(seen_frames.end(), sl.frames.begin(), sl.frames.end());
            for (size_t i = 0; i < sl.recs.size(); ++i)
                if (sl.recs[i].plane_id == PAINT_YUV_PLANE_Y) seen_regions.push_back(sl.region[i]);
            scratch += sl.scratch_bytes;
            largest = std::max(largest, sl.scratch_bytes);
            first = end;
        }
        // whole frames: every touched frame in exactly one slice, every region with a K in exactly one, with its frame
        CHECK(seen_frames == L.touched);
        std::sort(seen_regions.begin(), seen_regions.end());
        std::vector<int> want;
        for (size_t r = 0; r < regions.size(); ++r)
            if (L.clipped[r].w > 0) want.push_back((int)r);
        CHECK(seen_regions == want);
        CHECK(scratch == lay.scratch_bytes && largest <= lay.scratch_bytes && (max_frames != 0 || largest == lay.scratch_bytes));
    }
}

int main() {
    Frames F;
    // all layouts; pads and offsets that put the planes' rows at every address mod 4
    F.add(38, 30, VJ_YUV_NV12, 0, 0);
    F.add(38, 30, VJ_YUV_NV21, 1, 1);
    F.add(38, 30, VJ_YUV_I420, 3, 2);
    F.add(300, 40, VJ_YUV_NV12, 2, 3);
    F.add(10, 6, VJ_YUV_I420, 0, 1);     // a frame no region names
    F.add(524, 68, VJ_YUV_I420, 1, 0);
    F.add(2, 2, VJ_YUV_NV21, 1, 3);
    std::vector<vj_roi> regions;
    const int frames_used[] = {3, 0, 2, 1, 5, 0, 3, 6};   // mixed frame order
    for (int f : frames_used) {
        const int w = F.im[(size_t)f].width, h = F.im[(size_t)f].height;
        const vj_roi some[] = {{f, 4, 6, 1, 1}, {f, 7, 9, 1, 1}, {f, 11, 13, 2, 2}, {f, 21, 3, 1, 8}, {f, 9, 20, 11, 1}, {f, -5, 8, 10, 10},
                               {f, w - 7, 9, 10, 9}, {f, 8, -5, 11, 10}, {f, 9, h - 5, 10, 10}, {f, -3, -3, 10, 10}, {f, w - 7, h - 7, 10, 10},
                               {f, w + 50, h + 50, 6, 6}, {f, -40, 3, 6, 6}, {f, 0, 0, w, h}, {f, 3, 3, 20, 15}, {f, 11, 7, 22, 18}, {f, 6, 12, 13, 9},
                               {f, 3, 3, 20, 15}, {f, 2, 4, 5, 7}, {f, 7, 4, 5, 7}, {f, 1, 0, w - 1, 33}, {f, 0, 1, 1, 1}};
        regions.insert(regions.end(), std::begin(some), std::end(some));
    }
    std::set<uintptr_t> rows_mod4[3];
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
                p.color[0] = 17, p.color[1] = 201, p.color[2] = 94;
                run_call(F, regions, p, rows_mod4);
            }
    for (int id = 0; id < 3; ++id) CHECK(rows_mod4[id].size() == 4u);

    // the colour, the layout entry point and the error cases
    {
        vj_paint_params p;
        vj_paint_default(&p);
        p.color[0] = 255;   // B = 255 -> (41, 240, 110)
        PaintYuvLayout lay;
        CHECK(paint_yuv_layout(F.im.data(), (int)F.im.size(), regions.data(), 1, &p, &lay) == VJ_OK && lay.yc == 41 && lay.uc == 240 && lay.vc == 110);
        const size_t n = regions.size();
        std::vector<vj_roi> k(n), kc(n);
        std::vector<int32_t> s(n), cs(n);
        uint64_t bytes = 1;
        const int nf = (int)F.im.size();
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, regions.data(), (int)n, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_OK && bytes > 0);
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, nullptr, 0, &p, nullptr, nullptr, nullptr, nullptr, &bytes) == VJ_OK && bytes == 0);
        CHECK(vj_paint_yuv_layout(nullptr, 1, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), nullptr) == VJ_ERR_ARG);
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, regions.data(), 1, &p, k.data(), nullptr, s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        vj_paint_params q = p;
        q.mode = 4;
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, regions.data(), 1, &q, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        q = p;
        q.size = 256;
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, regions.data(), 1, &q, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_LIMIT);
        const vj_roi huge = {0, 0, 0, 32768, 4}, none = {9, 0, 0, 4, 4};
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, &huge, 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_LIMIT);
        CHECK(vj_paint_yuv_layout(F.im.data(), nf, &none, 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        // frames: odd sizes, a missing plane, a short stride, an unknown layout, a side above 65534
        std::vector<vj_yuv_image> bad = F.im;
        bad[0].width = 37;
        CHECK(vj_paint_yuv_layout(bad.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        bad = F.im, bad[2].c1 = nullptr;
        CHECK(vj_paint_yuv_layout(bad.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        bad = F.im, bad[1].c_stride = 37;
        CHECK(vj_paint_yuv_layout(bad.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        bad = F.im, bad[1].layout = 3;
        CHECK(vj_paint_yuv_layout(bad.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        bad = F.im, bad[1].width = 65536, bad[1].y_stride = bad[1].c_stride = 65536;
        CHECK(vj_paint_yuv_layout(bad.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_LIMIT);
        // planes that overlap: a frame twice; a plane inside another frame's; the planes of one frame
        std::vector<vj_yuv_image> twice = F.im;
        twice.push_back(F.im[1]);
        CHECK(vj_paint_yuv_layout(twice.data(), nf + 1, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        twice.back().on_device = 1;   // another address space: no overlap
        CHECK(vj_paint_yuv_layout(twice.data(), nf + 1, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_OK);
        twice = F.im;
        twice[0].c0 = twice[3].y + 5;
        CHECK(vj_paint_yuv_layout(twice.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        twice = F.im;
        twice[2].c1 = twice[2].c0 + 3;
        CHECK(vj_paint_yuv_layout(twice.data(), nf, regions.data(), 1, &p, k.data(), kc.data(), s.data(), cs.data(), &bytes) == VJ_ERR_ARG);
        CHECK(paint_yuv_layout(F.im.data(), nf, regions.data(), (int)n, &p, &lay) == VJ_OK);
        PaintYuvSlice sl;
        CHECK(paint_yuv_plan_slice(F.im.data(), lay, 2, lay.luma.touched.size() + 1, &sl) == VJ_ERR_ARG);
    }
    printf("paint_yuv_asan_driver: OK\n");
    return 0;
}
