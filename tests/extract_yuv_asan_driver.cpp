// Sanitizer driver of the host planner of vj_extract_yuv / vj_extract_affine_yuv (csrc/vj_extract_yuv_host.cpp: the argument checks
// through the planners of vj_yuv_to_bgr, vj_extract and vj_extract_affine, the region records with the planes, the taps and the work
// units of a slice): built by tests/test_sanitizers_extract_yuv.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/extract_yuv_asan_driver.cpp csrc/vj_extract_yuv_host.cpp csrc/vj_extract_host.cpp csrc/vj_affine_host.cpp
//       csrc/vj_yuv_host.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp
//       csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Frames of the three layouts whose planes lie in heap blocks of their own that END with the plane's last row, at
// every address mod 4 and with padded strides; regions inside them, over every side and corner, wholly outside and with margins, to
// several output sizes (the copy, the 2 x 2 mean, bilinear) and affines likewise; interleaved, planar and gray, three and four
// channels; the destination at every address mod 4; whole calls and slices of 1, 2 and 3 frames.  The work units are decoded as the
// kernels decode them (region from the unit prefix, block, wave, lane -> the slot's bytes -> the pixels -> the taps): every output
// byte of every region is covered exactly once, every tap lies inside its run, every clamped Y and chroma index inside its plane —
// the bytes are read, so ASan sees each access — and a 2-byte load happens only at an even address.  Then the error cases.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_extract_yuv_host.hpp"

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
    // a plane of `rows` rows of row_bytes bytes, `pad` more between rows, `off` bytes into a block that ends with its last byte
    const uint8_t* plane(int rows, int row_bytes, int pad, int off) {
        const size_t bytes = (size_t)off + (size_t)(rows - 1) * (size_t)(row_bytes + pad) + (size_t)row_bytes;
        mem.emplace_back(new uint8_t[bytes]);
        for (size_t i = 0; i < bytes; ++i) mem.back()[i] = (uint8_t)(i * 7u + 1u);
        return mem.back().get() + off;
    }
    void add(int w, int h, int layout, int pad, int variant) {
        const int cb = layout == VJ_YUV_I420 ? w / 2 : w;
        vj_yuv_image f;
        memset(&f, 0, sizeof(f));
        f.y = plane(h, w, pad, variant & 3);
        f.c0 = plane(h / 2, cb, pad + 1, (variant + 1) & 3);
        f.c1 = layout == VJ_YUV_I420 ? plane(h / 2, cb, pad + 1, (variant + 3) & 3) : nullptr;
        f.width = w, f.height = h, f.y_stride = w + pad, f.c_stride = cb + pad + 1, f.layout = layout, f.on_device = 0;
        im.push_back(f);
    }
};

static volatile uint32_t sink;
static uint64_t loads2, loads1;
static int clampi(int v, int hi) { return std::min(std::max(v, 0), hi); }

// one tap read as the kernels read it: the Y byte and the chroma sample of the clamped luma pixel, inside their planes
static void read_tap(const vj_yuv_image& f, const YuvPlanesDev& d, int xs, int ys) {
    CHECK(xs >= 0 && xs < d.fw && ys >= 0 && ys < d.fh);
    sink = sink + d.y[(size_t)ys * d.y_stride + (size_t)xs];
    const int cx = xs >> 1, cy = ys >> 1;
    CHECK(cx < d.fw / 2 && cy < d.fh / 2);
    if (d.layout == YUV_I420) {
        CHECK(d.c1 != nullptr);
        sink = sink + d.c0[(size_t)cy * d.c_stride + (size_t)cx] + d.c1[(size_t)cy * d.c_stride + (size_t)cx];
    } else {
        const uint8_t* p = d.c0 + (size_t)cy * d.c_stride + 2u * (size_t)cx;
        if (((uintptr_t)p & 1u) == 0u) {   // the 2-byte load: only here, at an even address, both bytes inside the row
            CHECK(2 * cx + 2 <= d.fw);
            ++loads2;
        } else {
            ++loads1;
        }
        sink = sink + p[0] + p[1];
    }
    (void)f;
}

static void check_planes(const vj_yuv_image& f, const YuvPlanesDev& d) {
    CHECK(d.y == f.y && d.c0 == f.c0 && d.c1 == (f.layout == VJ_YUV_I420 ? f.c1 : nullptr));
    CHECK(d.y_stride == (uint32_t)f.y_stride && d.c_stride == (uint32_t)f.c_stride && d.fw == f.width && d.fh == f.height && d.layout == (uint32_t)f.layout);
}

// the slot of (row r, lane) of block column bx as the kernels lay it: -> false when it holds no byte of the row
struct Slot { int32_t b0, lo, hi; uint64_t row_at; };
static bool slot_of(uint64_t dst_off, uint32_t r, uint32_t B, uint32_t bx, uint32_t lane, uint32_t dst_mod, Slot* s) {
    s->row_at = dst_off + (uint64_t)r * B;
    const uint32_t mis = (uint32_t)((dst_mod + s->row_at) & 3u);
    s->b0 = (int32_t)((bx * EXTRACT_BLOCK_SLOTS + lane) * 4u) - (int32_t)mis;
    s->lo = std::max(s->b0, 0), s->hi = std::min(s->b0 + 4, (int32_t)B);
    if (s->lo >= s->hi) return false;
    if (s->hi - s->lo == 4) CHECK(((dst_mod + s->row_at + (uint64_t)s->b0) & 3u) == 0u);   // a whole slot is an aligned dword
    return true;
}

static void check_counts(uint32_t C, bool gray, bool planar, uint32_t ow, uint32_t oh, uint32_t rows, uint32_t row_bytes, uint64_t region_bytes,
                         uint64_t bytes, uint64_t n, const vj_yuv_params& yp) {
    CHECK(C == (gray ? 1u : (uint32_t)yp.channels));
    CHECK(rows == (planar ? C * oh : oh) && row_bytes == (planar ? ow : ow * C));
    CHECK(region_bytes == (uint64_t)ow * oh * C && bytes == region_bytes * n);
}

static uint32_t unit_region(uint32_t u0, size_t m, const std::vector<uint32_t>& firsts) {
    uint32_t lo = 0, hi = (uint32_t)m;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (firsts[mid] <= u0) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the whole vj_extract_yuv call through the C entry point and the planner, then every slice of at most `max_frames` distinct frames
static void plan_all(const Frames& fr, const std::vector<vj_roi>& regions, const vj_extract_params& p, const vj_yuv_params& yp, size_t max_frames,
                     uint32_t dst_mod) {
    const int nf = (int)fr.im.size(), n = (int)regions.size();
    std::vector<vj_roi> src((size_t)n + 1);
    int channels = -1;
    uint64_t bytes = 1;
    CHECK(vj_extract_yuv_layout(fr.im.data(), nf, regions.data(), n, &p, &yp, src.data(), &channels, &bytes) == VJ_OK);
    ExtractYuvLayout L;
    CHECK(extract_yuv_layout(fr.im.data(), nf, regions.data(), n, &p, &yp, &L) == VJ_OK);
    const ExtractLayout& lay = L.lay;
    CHECK(lay.bytes == bytes && lay.src.size() == (size_t)n && (int)lay.C == channels && lay.region_pitch == lay.region_bytes);
    CHECK(L.src.luma.size() == (size_t)nf && L.src.channels == (uint32_t)yp.channels && L.src.swap_rb == ((yp.flags & VJ_YUV_RGB_ORDER) != 0u));
    check_counts(lay.C, lay.gray, lay.planar, lay.out_w, lay.out_h, lay.rows, lay.row_bytes, lay.region_bytes, bytes, (uint64_t)n, yp);
    for (int r = 0; r < n; ++r) CHECK(memcmp(&lay.src[(size_t)r], &src[(size_t)r], sizeof(vj_roi)) == 0);
    std::vector<uint8_t> covered((size_t)bytes, 0);
    const uint32_t B = lay.row_bytes, R = lay.rows, C = lay.C;
    ExtractYuvSlice sl;
    size_t slices = 0;
    for (size_t first = 0; first < (size_t)n; ++slices) {
        const size_t end = extract_slice_end(regions.data(), (size_t)n, first, max_frames);
        CHECK(end > first && end <= (size_t)n);
        const size_t m = end - first;
        CHECK(extract_yuv_plan_slice(fr.im.data(), regions.data(), L, first, m, &sl) == VJ_OK);
        CHECK(sl.recs.size() == m && sl.luma.recs.size() == m && !sl.luma.frames.empty());
        if (max_frames) CHECK(sl.luma.frames.size() <= max_frames);
        else CHECK(end == (size_t)n);
        uint64_t unit = 0;
        std::vector<uint32_t> firsts;
        for (size_t i = 0; i < m; ++i) {
            const ExtractYuvRegionDev& d = sl.recs[i];
            const vj_roi& s = lay.src[first + i];
            check_planes(fr.im[(size_t)s.frame], d.f);
            CHECK(std::find(sl.luma.frames.begin(), sl.luma.frames.end(), s.frame) != sl.luma.frames.end());
            CHECK(d.x0 == s.x && d.y0 == s.y && d.cw == (uint32_t)s.w && d.ch == (uint32_t)s.h && d.dst_off == (first + i) * lay.region_bytes);
            CHECK(d.f.unit_first == unit);
            firsts.push_back(d.f.unit_first);
            unit += extract_units(B, R);
            CHECK((d.mode == EXTRACT_COPY) == (d.cw == lay.out_w && d.ch == lay.out_h));
            CHECK((d.mode == EXTRACT_AREA) == (d.cw == 2u * lay.out_w && d.ch == 2u * lay.out_h));
            if (d.mode != EXTRACT_BILINEAR) continue;
            CHECK((size_t)d.xtab + lay.out_w <= sl.luma.taps.size() && (size_t)d.ytab + lay.out_h <= sl.luma.taps.size());
            for (uint32_t x = 0; x < lay.out_w; ++x) CHECK(sl.luma.taps[(size_t)d.xtab + x].i0 < d.cw && sl.luma.taps[(size_t)d.xtab + x].i1 < d.cw);
            for (uint32_t y = 0; y < lay.out_h; ++y) CHECK(sl.luma.taps[(size_t)d.ytab + y].i0 < d.ch && sl.luma.taps[(size_t)d.ytab + y].i1 < d.ch);
        }
        CHECK(unit == sl.luma.n_units);
        for (uint32_t u0 = 0; u0 < sl.luma.n_units; ++u0) {   // the units as extract_yuv_regions decodes them
            const uint32_t k = unit_region(u0, m, firsts);
            const ExtractYuvRegionDev& d = sl.recs[k];
            const vj_yuv_image& f = fr.im[(size_t)lay.src[first + k].frame];
            CHECK(d.dst_off + (uint64_t)R * B <= bytes);
            const uint32_t bpr = extract_row_blocks(B), u = u0 - d.f.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            CHECK(by * EXTRACT_BLOCK_H < R);
            for (uint32_t tid = 0; tid < 256u; ++tid)
                for (uint32_t r = by * EXTRACT_BLOCK_H + (tid >> 6); r < std::min((by + 1u) * EXTRACT_BLOCK_H, R); r += 4u) {
                    Slot s;
                    if (!slot_of(d.dst_off, r, B, bx, tid & 63u, dst_mod, &s)) continue;
                    uint32_t cpl = 0, y = r;
                    if (lay.planar) {
                        cpl = r / lay.out_h;
                        y = r - cpl * lay.out_h;
                    }
                    CHECK(y < lay.out_h && cpl < C);
                    int yi0, yi1;
                    if (d.mode == EXTRACT_COPY) yi0 = yi1 = (int)y;
                    else if (d.mode == EXTRACT_AREA) { yi0 = 2 * (int)y; yi1 = yi0 + 1; }
                    else { yi0 = sl.luma.taps[(size_t)d.ytab + y].i0; yi1 = sl.luma.taps[(size_t)d.ytab + y].i1; }
                    const int ys0 = clampi(d.y0 + yi0, d.f.fh - 1), ys1 = clampi(d.y0 + yi1, d.f.fh - 1);
                    uint32_t x_at = 0xffffffffu;
                    for (int32_t b = s.lo; b < s.hi; ++b) {
                        CHECK(covered[(size_t)(s.row_at + (uint64_t)b)] == 0);   // no byte twice
                        covered[(size_t)(s.row_at + (uint64_t)b)] = 1;
                        uint32_t x = (uint32_t)b, c = cpl;
                        if (!lay.planar && C > 1u) {
                            x = (uint32_t)b / C;
                            c = (uint32_t)b - x * C;
                        }
                        CHECK(x < lay.out_w && c < C);
                        if (x == x_at) continue;   // the taps of a pixel: once for the bytes of its slot
                        x_at = x;
                        int xi0, xi1;
                        if (d.mode == EXTRACT_COPY) xi0 = xi1 = (int)x;
                        else if (d.mode == EXTRACT_AREA) { xi0 = 2 * (int)x; xi1 = xi0 + 1; }
                        else { xi0 = sl.luma.taps[(size_t)d.xtab + x].i0; xi1 = sl.luma.taps[(size_t)d.xtab + x].i1; }
                        CHECK((uint32_t)xi1 < d.cw && (uint32_t)yi1 < d.ch);
                        const int xs0 = clampi(d.x0 + xi0, d.f.fw - 1), xs1 = clampi(d.x0 + xi1, d.f.fw - 1);
                        read_tap(f, d.f, xs0, ys0);
                        if (d.mode == EXTRACT_COPY) continue;
                        read_tap(f, d.f, xs1, ys0);
                        read_tap(f, d.f, xs0, ys1);
                        read_tap(f, d.f, xs1, ys1);
                    }
                }
        }
        first = end;
    }
    for (uint64_t b = 0; b < bytes; ++b) CHECK(covered[(size_t)b] == 1);   // every byte of every region, once
    if (max_frames == 0 && n > 0) CHECK(slices == 1);
}

// ... and the whole vj_extract_affine_yuv call
static void plan_all_affine(const Frames& fr, const std::vector<vj_affine>& affines, const vj_affine_params& p, const vj_yuv_params& yp, size_t max_frames,
                            uint32_t dst_mod) {
    const int nf = (int)fr.im.size(), n = (int)affines.size();
    int channels = -1;
    uint64_t bytes = 1;
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), nf, affines.data(), n, &p, &yp, &channels, &bytes) == VJ_OK);
    AffineYuvLayout L;
    CHECK(affine_yuv_layout(fr.im.data(), nf, affines.data(), n, &p, &yp, &L) == VJ_OK);
    const AffineLayout& lay = L.lay;
    CHECK(lay.bytes == bytes && (int)lay.C == channels);
    check_counts(lay.C, lay.gray, lay.planar, lay.out_w, lay.out_h, lay.rows, lay.row_bytes, lay.region_bytes, bytes, (uint64_t)n, yp);
    std::vector<uint8_t> covered((size_t)bytes, 0);
    const uint32_t B = lay.row_bytes, R = lay.rows, C = lay.C;
    AffineYuvSlice sl;
    for (size_t first = 0; first < (size_t)n;) {
        const size_t end = affine_slice_end(affines.data(), (size_t)n, first, max_frames);
        CHECK(end > first && end <= (size_t)n);
        const size_t m = end - first;
        CHECK(affine_yuv_plan_slice(fr.im.data(), affines.data(), L, first, m, &sl) == VJ_OK);
        CHECK(sl.recs.size() == m && !sl.luma.frames.empty() && (max_frames == 0 || sl.luma.frames.size() <= max_frames));
        uint64_t unit = 0;
        std::vector<uint32_t> firsts;
        for (size_t i = 0; i < m; ++i) {
            const AffineYuvRegionDev& d = sl.recs[i];
            check_planes(fr.im[(size_t)affines[first + i].frame], d.f);
            CHECK(d.dst_off == (first + i) * lay.region_bytes && d.f.unit_first == unit && memcmp(d.m, affines[first + i].m, sizeof(d.m)) == 0);
            firsts.push_back(d.f.unit_first);
            unit += extract_units(B, R);
        }
        CHECK(unit == sl.luma.n_units);
        for (uint32_t u0 = 0; u0 < sl.luma.n_units; ++u0) {   // the units as affine_yuv_regions decodes them
            const uint32_t k = unit_region(u0, m, firsts);
            const AffineYuvRegionDev& d = sl.recs[k];
            const vj_yuv_image& f = fr.im[(size_t)affines[first + k].frame];
            CHECK(d.dst_off + (uint64_t)R * B <= bytes);
            const uint32_t bpr = extract_row_blocks(B), u = u0 - d.f.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            CHECK(by * EXTRACT_BLOCK_H < R);
            for (uint32_t tid = 0; tid < 256u; ++tid)
                for (uint32_t r = by * EXTRACT_BLOCK_H + (tid >> 6); r < std::min((by + 1u) * EXTRACT_BLOCK_H, R); r += 4u) {
                    Slot s;
                    if (!slot_of(d.dst_off, r, B, bx, tid & 63u, dst_mod, &s)) continue;
                    uint32_t cpl = 0, y = r;
                    if (lay.planar) {
                        cpl = r / lay.out_h;
                        y = r - cpl * lay.out_h;
                    }
                    CHECK(y < lay.out_h && cpl < C);
                    const int32_t X0 = affine_row_term(d.m[1], d.m[2], y), Y0 = affine_row_term(d.m[4], d.m[5], y);
                    uint32_t x_at = 0xffffffffu;
                    for (int32_t b = s.lo; b < s.hi; ++b) {
                        CHECK(covered[(size_t)(s.row_at + (uint64_t)b)] == 0);
                        covered[(size_t)(s.row_at + (uint64_t)b)] = 1;
                        uint32_t x = (uint32_t)b, c = cpl;
                        if (!lay.planar && C > 1u) {
                            x = (uint32_t)b / C;
                            c = (uint32_t)b - x * C;
                        }
                        CHECK(x < lay.out_w && c < C);
                        if (x == x_at) continue;
                        x_at = x;
                        const int32_t X = (X0 + affine_col_term(d.m[0], x)) >> 5;   // int32 sums: UBSan sees an overflow
                        const int32_t Y = (Y0 + affine_col_term(d.m[3], x)) >> 5;
                        const int32_t sx = X >> 5, sy = Y >> 5;
                        const int xs0 = clampi(sx, d.f.fw - 1), xs1 = clampi(sx + 1, d.f.fw - 1);
                        const int ys0 = clampi(sy, d.f.fh - 1), ys1 = clampi(sy + 1, d.f.fh - 1);
                        read_tap(f, d.f, xs0, ys0);
                        read_tap(f, d.f, xs1, ys0);
                        read_tap(f, d.f, xs0, ys1);
                        read_tap(f, d.f, xs1, ys1);
                    }
                }
        }
        first = end;
    }
    for (uint64_t b = 0; b < bytes; ++b) CHECK(covered[(size_t)b] == 1);
}

static vj_extract_params params(int ow, int oh, double sx, double sy, double margin, uint32_t flags, uint32_t reserved = 0) {
    vj_extract_params p;
    vj_extract_default(&p);
    p.out_w = ow, p.out_h = oh, p.sx = sx, p.sy = sy, p.margin = margin, p.flags = flags, p.reserved = reserved;
    return p;
}
static vj_affine_params aparams(int ow, int oh, uint32_t flags, uint32_t reserved = 0) {
    vj_affine_params p;
    vj_affine_default(&p);
    p.out_w = ow, p.out_h = oh, p.flags = flags, p.reserved = reserved;
    return p;
}
static vj_yuv_params yparams(int channels, uint32_t flags = 0, uint32_t reserved = 0) {
    vj_yuv_params p;
    memset(&p, 0xff, sizeof(p));
    vj_yuv_default(&p);
    CHECK(p.channels == 3 && p.flags == 0u && p.reserved == 0u);
    p.channels = channels, p.flags = flags, p.reserved = reserved;
    return p;
}

// regions of a 38 x 30 frame: inside at the four parities of the origin, over each side and corner, wholly outside, the whole frame
static std::vector<vj_roi> regions_on(int frame) {
    return {{frame, 8, 6, 20, 17}, {frame, 9, 6, 20, 17}, {frame, 8, 7, 20, 17}, {frame, 9, 7, 20, 17}, {frame, 3, 4, 1, 1}, {frame, 5, 5, 2, 3},
            {frame, 4, 7, 5, 5}, {frame, -5, 8, 10, 10}, {frame, 31, 8, 10, 10}, {frame, 8, -5, 10, 10}, {frame, 8, 25, 10, 10},
            {frame, -3, -3, 10, 10}, {frame, 31, -3, 10, 10}, {frame, -3, 23, 10, 10}, {frame, 31, 23, 10, 10},
            {frame, 100, 100, 6, 6}, {frame, -40, 3, 6, 6}, {frame, 0, 0, 38, 30}};
}
static vj_affine affine(int frame, double m0, double m1, double m2, double m3, double m4, double m5) {
    vj_affine a;
    memset(&a, 0, sizeof(a));
    a.frame = frame;
    const double m[6] = {m0, m1, m2, m3, m4, m5};
    memcpy(a.m, m, sizeof(m));
    return a;
}
static std::vector<vj_affine> affines_on(int frame) {
    return {affine(frame, 1, 0, 0, 0, 1, 0), affine(frame, 1, 0, 3, 0, 1, -2), affine(frame, 1.1258, -0.65, 5.2, 0.65, 1.1258, -3.1),
            affine(frame, 1, 0.375, 2.25, 0.125, 1, -1.5), affine(frame, 5, 0, 1.3, 0, 5, 0.7), affine(frame, 0.25, 0, 10.1, 0, 0.25, 8.3),
            affine(frame, 0.9, -0.15, -6, 0.15, 0.9, 12), affine(frame, 0.9, -0.15, 34, 0.15, 0.9, 26), affine(frame, 1, 0, 100, 0, 1, 100),
            affine(frame, 1, 0, -60, 0, 1, 5), affine(frame, -1, 0, 37, 0, -1, 29)};
}

int main() {
    const uint32_t all_flags[] = {0u, (uint32_t)VJ_EXTRACT_GRAY, (uint32_t)VJ_EXTRACT_PLANAR, (uint32_t)(VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR)};
    for (int variant = 0; variant < 4; ++variant) {   // the planes at every address mod 4, the pair plane at odd and even ones
        Frames fr;
        fr.add(38, 30, VJ_YUV_NV12, variant, variant);
        fr.add(38, 30, VJ_YUV_NV21, (variant + 1) % 3, variant + 1);
        fr.add(38, 30, VJ_YUV_I420, 5, variant + 2);
        fr.add(10, 4, VJ_YUV_NV12, 1, variant + 3);
        std::vector<vj_roi> regions;
        std::vector<vj_affine> affines;
        for (int f = 0; f < 3; ++f) {
            for (const vj_roi& r : regions_on(f)) regions.push_back(r);
            for (const vj_affine& a : affines_on(f)) affines.push_back(a);
        }
        regions.push_back(vj_roi{3, 0, 0, 10, 4});
        regions.push_back(vj_roi{0, 1, 1, 7, 7});
        regions.push_back(vj_roi{3, -2, -2, 13, 8});
        affines.push_back(affine(3, 0.5, 0, 0, 0, 0.5, 0));
        affines.push_back(affine(0, 1, 0, 0.5, 0, 1, 0.5));
        for (uint32_t flags : all_flags)
            for (uint32_t mod = 0; mod < 4u; ++mod) {
                const size_t per = mod;   // whole calls, and slices of 1, 2 and 3 frames
                const vj_yuv_params yp = yparams(mod & 1u ? 4 : 3, mod & 2u ? (uint32_t)VJ_YUV_RGB_ORDER : 0u);
                plan_all(fr, regions, params(10, 10, 1, 1, 0, flags), yp, per, mod);        // copies among them
                plan_all(fr, regions, params(5, 5, 1, 1, 0, flags), yp, per, mod);          // the 2 x 2 mean of the 10 x 10 regions
                plan_all(fr, regions, params(20, 17, 1, 1, 0, flags), yp, per, mod);
                plan_all(fr, regions, params(24, 24, 0.5, 0.5, 0.25, flags), yp, per, mod); // ties and a margin
                plan_all(fr, regions, params(7, 3, 1.8, 1.8, 0.1, flags), yp, per, mod);
                plan_all(fr, regions, params(1, 1, 0, 0, 0, flags), yp, per, mod);
                plan_all_affine(fr, affines, aparams(12, 10, flags), yp, per, mod);
                plan_all_affine(fr, affines, aparams(33, 21, flags), yp, per, (mod + 1u) & 3u);
                plan_all_affine(fr, affines, aparams(1, 1, flags), yp, per, mod);
            }
        if (variant == 0)
            for (int w : {1, 2, 3, 4, 5, 6, 7, 8, 9, 21, 63, 64, 65, 85, 86, 255, 256, 257})
                for (int h : {1, 2, 5, 17}) {
                    const vj_yuv_params yp = yparams(w % 3 == 0 ? 4 : 3);
                    plan_all(fr, regions, params(w, h, 1, 1, 0, w % 2 ? 0u : (uint32_t)VJ_EXTRACT_PLANAR), yp, 0, (uint32_t)(w + h) & 3u);
                    plan_all_affine(fr, affines, aparams(w, h, w % 2 ? (uint32_t)VJ_EXTRACT_PLANAR : 0u), yp, 0, (uint32_t)(w + h + 1) & 3u);
                }
        plan_all(fr, {}, params(4, 4, 1, 1, 0, 0), yparams(3), 0, 0);
        plan_all_affine(fr, {}, aparams(4, 4, 0), yparams(3), 0, 0);
    }
    CHECK(loads2 > 0 && loads1 > 0);   // both ways of loading a pair were walked

    // ---- the error cases
    Frames fr;
    fr.add(38, 30, VJ_YUV_NV12, 0, 0);
    fr.add(10, 4, VJ_YUV_I420, 2, 1);
    const std::vector<vj_roi> good = {{0, 0, 0, 4, 4}, {1, 1, 1, 2, 2}};
    const std::vector<vj_affine> agood = {affine(0, 1, 0, 0, 0, 1, 0), affine(1, 1, 0, 1, 0, 1, 1)};
    const vj_extract_params ok = params(4, 4, 1, 1, 0, 0);
    const vj_affine_params aok = aparams(4, 4, 0);
    const vj_yuv_params yok = yparams(3), y4 = yparams(4);
    vj_roi src[8];
    int c = 0;
    uint64_t bytes = 0;
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &yok, src, &c, &bytes) == VJ_OK && c == 3 && bytes == 96u);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &y4, src, &c, &bytes) == VJ_OK && c == 4 && bytes == 128u);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &aok, &y4, &c, &bytes) == VJ_OK && c == 4 && bytes == 128u);
    CHECK(vj_extract_yuv_layout(nullptr, 2, good.data(), 2, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0 && c == 0);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, nullptr, 2, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, nullptr, &yok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, nullptr, src, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "null") != nullptr);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &yok, nullptr, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &yok, src, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &yok, src, &c, nullptr) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), -1, good.data(), 2, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), -1, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_yuv_layout(nullptr, 0, nullptr, 0, &ok, &yok, nullptr, &c, &bytes) == VJ_OK && bytes == 0 && c == 3);
    CHECK(vj_extract_affine_yuv_layout(nullptr, 2, agood.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG && bytes == 0 && c == 0);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, nullptr, 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, nullptr, &yok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &aok, nullptr, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "null") != nullptr);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &aok, &yok, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &aok, &yok, &c, nullptr) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_yuv_layout(nullptr, 0, nullptr, 0, &aok, &y4, &c, &bytes) == VJ_OK && bytes == 0 && c == 4);
    // the frames by vj_yuv_to_bgr's rules
    const vj_yuv_image g = fr.im[0];
    const vj_yuv_image bad_f[] = {{nullptr, g.c0, nullptr, 38, 30, 38, 39, 0, 0}, {g.y, nullptr, nullptr, 38, 30, 38, 39, 0, 0}, {g.y, g.c0, nullptr, 38, 30, 38, 39, 2, 0},
                                  {g.y, g.c0, nullptr, 0, 30, 38, 39, 0, 0}, {g.y, g.c0, nullptr, 37, 30, 38, 39, 0, 0}, {g.y, g.c0, nullptr, 38, 29, 38, 39, 0, 0},
                                  {g.y, g.c0, nullptr, 38, 30, 37, 39, 0, 0}, {g.y, g.c0, nullptr, 38, 30, 38, 37, 0, 0}, {g.y, g.c0, nullptr, 38, 30, 38, 39, 3, 0}};
    for (const vj_yuv_image& b : bad_f) {
        const std::vector<vj_yuv_image> v = {fr.im[0], fr.im[1], b};
        bytes = 9;
        CHECK(vj_extract_yuv_layout(v.data(), 3, good.data(), 2, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0 && strstr(vj_last_error(), "frame 2") != nullptr);
        CHECK(vj_extract_affine_yuv_layout(v.data(), 3, agood.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 2") != nullptr);
    }
    {
        const std::vector<vj_yuv_image> v = {fr.im[0], {g.y, g.c0, nullptr, 65536, 2, 65536, 65536, 0, 0}};
        CHECK(vj_extract_yuv_layout(v.data(), 2, good.data(), 1, &ok, &yok, src, &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "65534") != nullptr);
        CHECK(vj_extract_affine_yuv_layout(v.data(), 2, agood.data(), 1, &aok, &yok, &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "65534") != nullptr);
    }
    // yp
    for (const vj_yuv_params& b : {yparams(1), yparams(5), yparams(3, 2u), yparams(3, 0, 1u)}) {
        CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &ok, &b, src, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "vj_yuv_params") != nullptr);
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &aok, &b, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "vj_yuv_params") != nullptr);
    }
    // the regions, affines and parameters by vj_extract's and vj_extract_affine's rules
    for (const vj_roi& b : {vj_roi{2, 0, 0, 4, 4}, vj_roi{-1, 0, 0, 4, 4}, vj_roi{0, 0, 0, 0, 4}, vj_roi{0, 0, 0, 4, 0}}) {
        const std::vector<vj_roi> v = {good[0], good[1], b};
        CHECK(vj_extract_yuv_layout(fr.im.data(), 2, v.data(), 3, &ok, &yok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0 && strstr(vj_last_error(), "region 2") != nullptr);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (const vj_extract_params& b : {params(0, 4, 1, 1, 0, 0), params(4, -1, 1, 1, 0, 0), params(4, 4, -0.5, 1, 0, 0), params(4, 4, 1, nan, 0, 0),
                                       params(4, 4, 1, 1, -0.1, 0), params(4, 4, 1, 1, 0, 4u), params(4, 4, 1, 1, 0, 0, 1u)})
        CHECK(vj_extract_yuv_layout(fr.im.data(), 2, good.data(), 2, &b, &yok, src, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
    {
        vj_affine b = agood[1];
        b.frame = 2;
        std::vector<vj_affine> v = {agood[0], b};
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, v.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "affine 1") != nullptr);
        v[1] = agood[1];
        v[1].m[4] = nan;
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, v.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "m[4]") != nullptr);
        v[1] = agood[1];
        v[1].reserved = 1;
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, v.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "reserved") != nullptr);
        v[1] = affine(1, 1, 0, 524289.0, 0, 1, 0);
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, v.data(), 2, &aok, &yok, &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "2^19") != nullptr);
        for (const vj_affine_params& bp : {aparams(0, 4, 0), aparams(4, 4, 4u), aparams(4, 4, 0, 1u)})
            CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &bp, &yok, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        const vj_affine_params big = aparams(65536, 4, 0);
        CHECK(vj_extract_affine_yuv_layout(fr.im.data(), 2, agood.data(), 2, &big, &yok, &c, &bytes) == VJ_ERR_LIMIT);
    }
    // the limits of the mapping, and the work units of the decoded channels
    {
        const vj_roi lim[] = {{0, 0, 0, 65536, 4}, {0, (1 << 24) + 1, 0, 4, 4}};
        for (const vj_roi& b : lim) CHECK(vj_extract_yuv_layout(fr.im.data(), 2, &b, 1, &ok, &yok, src, &c, &bytes) == VJ_ERR_LIMIT && bytes == 0);
        std::vector<vj_roi> many(683, vj_roi{0, 0, 0, 2, 2});
        std::vector<vj_roi> src_many(many.size());
        const vj_extract_params p = params(65535, 65535, 1, 1, 0, 0);   // 768 x 4096 blocks per region of three channels: 682 regions fit
        CHECK(vj_extract_yuv_layout(fr.im.data(), 2, many.data(), 683, &p, &yok, src_many.data(), &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "work units") != nullptr);
        CHECK(vj_extract_yuv_layout(fr.im.data(), 2, many.data(), 682, &p, &yok, src_many.data(), &c, &bytes) == VJ_OK && c == 3);
    }
    // a device-resident source plane that overlaps the destination (both calls check it with vj_yuv_to_bgr's function)
    {
        uint8_t* const base = (uint8_t*)(uintptr_t)0x10000;   // (addresses only: nothing is read)
        std::vector<vj_yuv_image> f = {{base + 4096, base + 8192, nullptr, 16, 4, 16, 16, 0, 1}, {base + 12288, base + 12400, base + 12500, 8, 4, 8, 4, 2, 1},
                                       {base, base + 100, nullptr, 16, 4, 16, 16, 0, 0}};
        CHECK(yuv_decode_check_overlap(f.data(), 3, base, 4096) == VJ_OK);
        CHECK(yuv_decode_check_overlap(f.data(), 3, base + 1, 4096) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr && strstr(vj_last_error(), "y plane") != nullptr);
        CHECK(yuv_decode_check_overlap(f.data(), 3, base + 8192 + 16 + 15, 1) == VJ_ERR_ARG && strstr(vj_last_error(), "c0 plane") != nullptr);
        CHECK(yuv_decode_check_overlap(f.data(), 3, base + 8192 + 32, 1) == VJ_OK);
        CHECK(yuv_decode_check_overlap(f.data(), 3, base + 12500 + 4 + 3, 1) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 1") != nullptr && strstr(vj_last_error(), "c1 plane") != nullptr);
    }
    printf("extract_yuv_asan_driver: OK\n");
    return 0;
}
