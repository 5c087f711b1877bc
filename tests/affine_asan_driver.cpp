// Sanitizer driver of the host planner of vj_extract_affine (csrc/vj_affine_host.cpp: the argument checks and limits, the layout, the
// two matrix helpers, the region records and work units of a slice): built by tests/test_sanitizers_affine.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/affine_asan_driver.cpp csrc/vj_affine_host.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp
//       csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Frames of three channel counts in heap blocks that END with their last row; identities, translations, turns,
// shears, scalings, regions across every side and wholly outside, and matrices AT the 2^19 limit, to several output sizes,
// interleaved, planar and gray, the destination at every address mod 4, whole and in slices.  The work units are decoded as the
// kernel decodes them (region from the unit prefix, block, wave, lane -> the slot's bytes; the row terms once per row, the column
// terms per pixel, in int32 as the kernel adds and shifts them — UBSan watches the sums): every output byte of every region is
// covered exactly once, every clamped source index lies inside its frame — the bytes are read, so ASan sees each access.  Then the
// error cases.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_affine_host.hpp"
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

static vj_affine affine(int frame, double m0, double m1, double m2, double m3, double m4, double m5) {
    vj_affine a;
    memset(&a, 0, sizeof(a));
    a.frame = frame;
    const double m[6] = {m0, m1, m2, m3, m4, m5};
    memcpy(a.m, m, sizeof(m));
    return a;
}

static vj_affine_params params(int ow, int oh, uint32_t flags, uint32_t reserved = 0) {
    vj_affine_params p;
    memset(&p, 0xff, sizeof(p));
    vj_affine_default(&p);
    CHECK(p.out_w == 0 && p.out_h == 0 && p.flags == 0u && p.reserved == 0u);
    p.out_w = ow;
    p.out_h = oh;
    p.flags = flags;
    p.reserved = reserved;
    return p;
}

// the whole call through the C entry point and the planner, then every slice of at most `max_frames` distinct frames, checked with
// the destination at address `dst_mod` mod 4
static void plan_all(const Frames& fr, const std::vector<vj_affine>& affines, const vj_affine_params& p, size_t max_frames, uint32_t dst_mod) {
    const int nf = (int)fr.im.size(), n = (int)affines.size();
    int channels = -1;
    uint64_t bytes = 1;
    CHECK(vj_extract_affine_layout(fr.im.data(), nf, affines.data(), n, &p, &channels, &bytes) == VJ_OK);
    AffineLayout lay;
    CHECK(affine_layout(fr.im.data(), nf, affines.data(), n, &p, &lay) == VJ_OK && lay.bytes == bytes);
    CHECK((int)lay.C == channels && (channels == 1 || channels == 3 || channels == 4));
    CHECK(lay.gray == ((p.flags & VJ_EXTRACT_GRAY) != 0u) && lay.planar == ((p.flags & VJ_EXTRACT_PLANAR) != 0u));
    CHECK(lay.out_w == (uint32_t)p.out_w && lay.out_h == (uint32_t)p.out_h);
    CHECK(lay.region_bytes == (uint64_t)p.out_w * p.out_h * lay.C && bytes == lay.region_bytes * (uint64_t)n);
    CHECK(lay.rows == (lay.planar ? lay.C * lay.out_h : lay.out_h) && lay.row_bytes == (lay.planar ? lay.out_w : lay.out_w * lay.C));
    std::vector<uint8_t> covered((size_t)bytes, 0);
    const uint32_t B = lay.row_bytes, R = lay.rows, C = lay.C;
    AffineSlice sl;
    size_t slices = 0;
    for (size_t first = 0; first < (size_t)n; ++slices) {
        const size_t end = affine_slice_end(affines.data(), (size_t)n, first, max_frames);
        CHECK(end > first && end <= (size_t)n);
        const size_t m = end - first;
        CHECK(affine_plan_slice(fr.im.data(), affines.data(), lay, first, m, &sl) == VJ_OK);
        CHECK(sl.recs.size() == m && !sl.frames.empty());
        if (max_frames) {
            CHECK(sl.frames.size() <= max_frames);
            if (end < (size_t)n) {   // greedy: the next affine names a frame the slice does not hold, and the slice is full
                CHECK(sl.frames.size() == max_frames);
                CHECK(std::find(sl.frames.begin(), sl.frames.end(), affines[end].frame) == sl.frames.end());
            }
        } else {
            CHECK(end == (size_t)n);
        }
        uint64_t unit = 0;
        for (size_t i = 0; i < m; ++i) {
            const AffineRegionDev& d = sl.recs[i];
            const vj_affine& g = affines[first + i];
            const vj_image& f = fr.im[(size_t)g.frame];
            CHECK(std::find(sl.frames.begin(), sl.frames.end(), g.frame) != sl.frames.end());
            CHECK(d.src == f.data && d.stride == (uint32_t)f.stride && d.channels == (uint32_t)f.channels && d.fw == f.width && d.fh == f.height);
            CHECK(memcmp(d.m, g.m, sizeof(g.m)) == 0 && d.dst_off == (first + i) * lay.region_bytes);
            CHECK(d.unit_first == unit);
            unit += extract_units(B, R);
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
            const AffineRegionDev& d = sl.recs[lo];
            const vj_image& f = fr.im[(size_t)affines[first + lo].frame];
            CHECK(d.dst_off + (uint64_t)R * B <= bytes);
            const uint32_t bpr = extract_row_blocks(B), u = u0 - d.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            CHECK(by * EXTRACT_BLOCK_H < R);
            const bool conv = lay.gray && d.channels > 1u;
            for (uint32_t wave = 0; wave < 4u; ++wave)
                for (uint32_t r = by * EXTRACT_BLOCK_H + wave; r < std::min((by + 1u) * EXTRACT_BLOCK_H, R); r += 4u) {
                    const uint64_t row_at = d.dst_off + (uint64_t)r * B;
                    const uint32_t mis = (uint32_t)((dst_mod + row_at) & 3u);
                    uint32_t cpl = 0, y = r;
                    if (lay.planar) {
                        cpl = r / lay.out_h;
                        y = r - cpl * lay.out_h;
                    }
                    CHECK(y < lay.out_h && cpl < C);
                    const int32_t X0 = affine_row_term(d.m[1], d.m[2], y), Y0 = affine_row_term(d.m[4], d.m[5], y);   // once per row
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const int32_t b0 = (int32_t)((bx * EXTRACT_BLOCK_SLOTS + lane) * 4u) - (int32_t)mis;
                        const int32_t blo = std::max(b0, 0), bhi = std::min(b0 + 4, (int32_t)B);
                        if (blo >= bhi) continue;
                        if (bhi - blo == 4) CHECK(((dst_mod + row_at + (uint64_t)b0) & 3u) == 0u);   // a whole slot is an aligned dword
                        for (int32_t b = blo; b < bhi; ++b) {
                            CHECK(covered[(size_t)(row_at + (uint64_t)b)] == 0);   // no byte twice
                            covered[(size_t)(row_at + (uint64_t)b)] = 1;
                            uint32_t x = (uint32_t)b, c = cpl;
                            if (!lay.planar && C > 1u) {
                                x = (uint32_t)b / C;
                                c = (uint32_t)b - x * C;
                            }
                            CHECK(x < lay.out_w && c < C);
                            const int32_t X = (X0 + affine_col_term(d.m[0], x)) >> 5;   // int32 sums: UBSan sees an overflow
                            const int32_t Y = (Y0 + affine_col_term(d.m[3], x)) >> 5;
                            const int32_t sx = X >> 5, sy = Y >> 5;
                            const uint32_t fx = (uint32_t)(X & 31), fy = (uint32_t)(Y & 31);
                            const uint32_t w00 = (32u - fx) * (32u - fy) * 32u, w01 = fx * (32u - fy) * 32u, w10 = (32u - fx) * fy * 32u, w11 = fx * fy * 32u;
                            CHECK(w00 + w01 + w10 + w11 == 32768u);
                            const int xs0 = clampi(sx, d.fw - 1), xs1 = clampi(sx + 1, d.fw - 1);
                            const int ys0 = clampi(sy, d.fh - 1), ys1 = clampi(sy + 1, d.fh - 1);
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

// matrices on a 37 x 29 frame: the identity, translations across sides and corners and outside, a quarter turn, a 30 degree turn at
// scale 1.3 and its mirror, a shear, a 5 x down-scale, a 4 x up-scale
static std::vector<vj_affine> affines_on(int frame) {
    const double a = 1.3 * std::cos(std::acos(-1.0) / 6), b = 1.3 * std::sin(std::acos(-1.0) / 6);
    return {affine(frame, 1, 0, 0, 0, 1, 0), affine(frame, 1, 0, 8, 0, 1, 6), affine(frame, 1, 0, -5, 0, 1, 8), affine(frame, 1, 0, 30, 0, 1, 25),
            affine(frame, 1, 0, -3, 0, 1, -3), affine(frame, 1, 0, 100, 0, 1, 100), affine(frame, 1, 0, -40, 0, 1, 3),
            affine(frame, 0, 1, 5, -1, 0, 12), affine(frame, a, -b, 18 - a * 16 + b * 10, b, a, 14 - b * 16 - a * 10),
            affine(frame, -a, -b, 18 + a * 16 + b * 10, -b, a, 14 + b * 16 - a * 10), affine(frame, 1, 0.375, 2.25, 0.125, 1, -1.5),
            affine(frame, 5, 0, 1.3, 0, 5, 0.7), affine(frame, 0.25, 0, 10.1, 0, 0.25, 8.3), affine(frame, 1.0 + 1.0 / 2048, 0, 3.0 / 1024, 0, 1.0 + 1.0 / 2048, 28.0 / 1024)};
}

int main() {
    for (int ch : {1, 3, 4}) {
        Frames fr;
        fr.add(37, 29, ch, 0);
        fr.add(37, 29, ch, 5);
        fr.add(9, 4, ch, 1);
        std::vector<vj_affine> affines = affines_on(0);
        for (const vj_affine& a : affines_on(1)) affines.push_back(a);
        affines.push_back(affine(2, 1, 0, 0, 0, 1, 0));
        affines.push_back(affine(0, 0.5, 0.25, 1, -0.25, 0.5, 7));
        affines.push_back(affine(2, 1, 0, -2, 0, 1, -2));
        for (uint32_t flags : {0u, (uint32_t)VJ_EXTRACT_GRAY, (uint32_t)VJ_EXTRACT_PLANAR, (uint32_t)(VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR)})
            for (uint32_t mod = 0; mod < 4u; ++mod) {
                const size_t per = mod == 0u ? 0 : mod == 1u ? 1 : 2;
                plan_all(fr, affines, params(10, 10, flags), per, mod);
                plan_all(fr, affines, params(33, 21, flags), per, mod);
                plan_all(fr, affines, params(7, 3, flags), per, mod);
                plan_all(fr, affines, params(1, 1, flags), per, mod);
            }
        for (int w : {1, 2, 3, 4, 5, 6, 7, 8, 9, 21, 63, 64, 65, 85, 86, 255, 256, 257})
            for (int h : {1, 2, 5, 17}) plan_all(fr, affines, params(w, h, w % 2 ? 0u : (uint32_t)VJ_EXTRACT_PLANAR), 0, (uint32_t)(w + h) & 3u);
        plan_all(fr, {}, params(4, 4, 0), 0, 0);
        // matrices AT the 2^19 limit (out_w - 1 = out_h - 1 = 16, so every product is exact): the sums reach 2^30 + 16 and stay in int32
        const double L = AFFINE_COORD_MAX, s = L / 16;
        const std::vector<vj_affine> at_limit = {affine(0, s, 0, L, s, 0, L), affine(0, -s, 0, -L, -s, 0, -L), affine(1, s, -s, L, -s, s, -L),
                                                 affine(1, -s, s, -L, s, -s, L), affine(2, 1, 1, L - 16, 1, -1, -L + 16), affine(0, s, 2 * s, -L, -s, -2 * s, L)};
        for (uint32_t flags : {0u, (uint32_t)VJ_EXTRACT_GRAY, (uint32_t)VJ_EXTRACT_PLANAR}) plan_all(fr, at_limit, params(17, 17, flags), 2, 1 + flags);
    }
    {   // frames of mixed channel counts: with VJ_EXTRACT_GRAY only
        Frames fr;
        fr.add(37, 29, 1, 3);
        fr.add(37, 29, 3, 0);
        fr.add(37, 29, 4, 1);
        std::vector<vj_affine> affines;
        for (int f = 0; f < 3; ++f)
            for (const vj_affine& a : affines_on(f)) affines.push_back(a);
        for (size_t per : {(size_t)0, (size_t)1, (size_t)2}) {
            plan_all(fr, affines, params(10, 10, VJ_EXTRACT_GRAY), per, 1);
            plan_all(fr, affines, params(5, 5, VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR), per, 3);
        }
        const vj_affine_params p = params(5, 5, 0);
        int c = 0;
        uint64_t bytes = 5;
        CHECK(vj_extract_affine_layout(fr.im.data(), 3, affines.data(), (int)affines.size(), &p, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "affine 14") != nullptr && strstr(vj_last_error(), "channels") != nullptr);
    }

    // ---- the matrix helpers
    {
        double m[6];
        CHECK(vj_affine_from_rect(8, 6, 20, 17, 64, 34, m) == VJ_OK);
        CHECK(m[0] == 20.0 / 64 && m[1] == 0 && m[2] == 8 + 0.5 * 20 / 64 - 0.5 && m[3] == 0 && m[4] == 17.0 / 34 && m[5] == 6 + 0.5 * 17 / 34 - 0.5);
        CHECK(vj_affine_from_rect(5, 6, 24, 20, 24, 20, m) == VJ_OK && m[0] == 1 && m[2] == 5 && m[4] == 1 && m[5] == 6);
        CHECK(vj_affine_from_eyes(30, 40, 70, 52, 112, 112, 0.3, 0.7, 0.35, m) == VJ_OK);
        const double d = (0.7 - 0.3) * 112, a = (70.0 - 30.0) / d, b = (52.0 - 40.0) / d, cxl = 0.3 * 112, cy = 0.35 * 112;
        CHECK(m[0] == a && m[1] == -b && m[2] == 30 - a * cxl + b * cy && m[3] == b && m[4] == a && m[5] == 40 - b * cxl - a * cy);
        CHECK(std::fabs(m[0] * (0.7 * 112) + m[1] * cy + m[2] - 70) < 1e-9 && std::fabs(m[3] * (0.7 * 112) + m[4] * cy + m[5] - 52) < 1e-9);
        CHECK(vj_affine_from_eyes(50, 20, 50, 60, 32, 32, 0.3, 0.7, 0.35, m) == VJ_OK && m[0] == 0 && m[4] == 0);   // a vertical eye line
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        CHECK(vj_affine_from_rect(0, 0, 4, 4, 4, 4, nullptr) == VJ_ERR_ARG && vj_affine_from_rect(nan, 0, 4, 4, 4, 4, m) == VJ_ERR_ARG);
        CHECK(vj_affine_from_rect(0, 0, 0, 4, 4, 4, m) == VJ_ERR_ARG && vj_affine_from_rect(0, 0, 4, inf, 4, 4, m) == VJ_ERR_ARG);
        CHECK(vj_affine_from_rect(0, 0, 4, 4, 0, 4, m) == VJ_ERR_ARG && vj_affine_from_rect(0, 0, 4, 4, 4, -1, m) == VJ_ERR_ARG);
        CHECK(vj_affine_from_eyes(0, 0, 1, 0, 4, 4, 0.3, 0.7, 0.35, nullptr) == VJ_ERR_ARG && vj_affine_from_eyes(0, nan, 1, 0, 4, 4, 0.3, 0.7, 0.35, m) == VJ_ERR_ARG);
        CHECK(vj_affine_from_eyes(0, 0, 1, 0, 4, 4, 0.7, 0.3, 0.35, m) == VJ_ERR_ARG && strstr(vj_last_error(), "ex_r") != nullptr);
        CHECK(vj_affine_from_eyes(3, 4, 3, 4, 4, 4, 0.3, 0.7, 0.35, m) == VJ_ERR_ARG && strstr(vj_last_error(), "coincide") != nullptr);
        CHECK(vj_affine_from_eyes(0, 0, 1, 0, 0, 4, 0.3, 0.7, 0.35, m) == VJ_ERR_ARG && vj_affine_from_eyes(0, 0, 1, 0, 4, 4, 0.3, inf, 0.35, m) == VJ_ERR_ARG);
    }

    // ---- the error cases
    Frames fr;
    fr.add(37, 29, 3, 0);
    fr.add(9, 4, 3, 2);
    const std::vector<vj_affine> good = {affine(0, 1, 0, 0, 0, 1, 0), affine(1, 0, 1, 1, -1, 0, 2)};
    const vj_affine_params ok = params(4, 4, 0);
    int c = 0;
    uint64_t bytes = 0;
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, &ok, &c, &bytes) == VJ_OK && c == 3 && bytes == 96u);
    CHECK(vj_extract_affine_layout(nullptr, 2, good.data(), 2, &ok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, nullptr, 2, &ok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, nullptr, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, &ok, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, &ok, &c, nullptr) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), -1, good.data(), 2, &ok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), -1, &ok, &c, &bytes) == VJ_ERR_ARG);
    CHECK(vj_extract_affine_layout(nullptr, 0, nullptr, 0, &ok, &c, &bytes) == VJ_OK && bytes == 0);
    const vj_image bad_f[] = {{nullptr, 4, 4, 4, 0, 1}, {fr.im[0].data, 0, 4, 4, 0, 1}, {fr.im[0].data, 4, -1, 4, 0, 1}, {fr.im[0].data, 4, 4, 3, 0, 1},
                              {fr.im[0].data, 4, 4, 11, 0, 3}, {fr.im[0].data, 4, 4, 8, 0, 2}};
    for (const vj_image& b : bad_f) {
        const std::vector<vj_image> v = {fr.im[0], fr.im[1], b};
        bytes = 9;
        CHECK(vj_extract_affine_layout(v.data(), 3, good.data(), 2, &ok, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr);
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    {
        vj_affine res = good[0];
        res.reserved = 3;
        std::vector<vj_affine> bad = {affine(2, 1, 0, 0, 0, 1, 0), affine(-1, 1, 0, 0, 0, 1, 0), res};
        for (int i = 0; i < 6; ++i)
            for (double v : {nan, inf, -inf}) {
                vj_affine a = good[1];
                a.m[i] = v;
                bad.push_back(a);
            }
        for (const vj_affine& b : bad) {
            const std::vector<vj_affine> v = {good[0], good[1], b};
            CHECK(vj_extract_affine_layout(fr.im.data(), 2, v.data(), 3, &ok, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
            CHECK(strstr(vj_last_error(), "affine 2") != nullptr);
        }
    }
    struct { vj_affine_params p; const char* word; } bad_p[] = {
        {params(0, 4, 0), "out_w"}, {params(4, 0, 0), "out_h"}, {params(-4, 4, 0), "out_w"}, {params(4, -1, 0), "out_h"},
        {params(4, 4, 4u), "flags"}, {params(4, 4, 0x80000001u), "flags"}, {params(4, 4, 0, 1u), "reserved"}};
    for (const auto& b : bad_p) {
        CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, &b.p, &c, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), b.word) != nullptr);
        CHECK(vj_extract_affine_layout(nullptr, 0, nullptr, 0, &b.p, &c, &bytes) == VJ_ERR_ARG);
    }
    // ---- the limits: sides up to 65535, the four magnitudes up to 2^19, work units within a 32-bit index
    {
        vj_affine_params p = params(65535, 1, 0);
        CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 1, &p, &c, &bytes) == VJ_OK && bytes == 65535ull * 3ull);
        for (const vj_affine_params& q : {params(65536, 4, 0), params(4, 65536, 0), params(2147483647, 2147483647, 0)}) {
            CHECK(vj_extract_affine_layout(fr.im.data(), 2, good.data(), 2, &q, &c, &bytes) == VJ_ERR_LIMIT && bytes == 0);
            CHECK(strstr(vj_last_error(), "65535") != nullptr);
        }
        const double L = AFFINE_COORD_MAX, up = std::nextafter(L, inf), s = L / 16, s_up = std::nextafter(s, inf);
        const vj_affine_params q = params(17, 17, 0);
        struct { vj_affine a; const char* word; } lim[] = {
            {affine(0, s_up, 0, 0, 0, 1, 0), "m[0]"}, {affine(0, 1, 0, 0, -s_up, 1, 0), "m[3]"}, {affine(0, 1, 0, up, 0, 1, 0), "m[2]"},
            {affine(0, 1, 0, 0, 0, 1, -up), "m[5]"}, {affine(0, 1, 1, L - 15, 0, 1, 0), "m[1]"}, {affine(0, 1, 0, 0, 0, -2, -L + 31), "m[4]"},
            {affine(0, 1e300, 0, 0, 0, 1, 0), "m[0]"}, {affine(0, 1, 1e308, 1e308, 0, 1, 0), "m[2]"}, {affine(0, 1, 0, 0, 0, -1e308, 0), "m[4]"}};
        for (const auto& b : lim) {
            const std::vector<vj_affine> v = {good[0], b.a};
            CHECK(vj_extract_affine_layout(fr.im.data(), 2, v.data(), 2, &q, &c, &bytes) == VJ_ERR_LIMIT && bytes == 0);
            CHECK(strstr(vj_last_error(), "affine 1") != nullptr && strstr(vj_last_error(), b.word) != nullptr && strstr(vj_last_error(), "2^19") != nullptr);
        }
        std::vector<vj_affine> many(2041, good[0]);
        p = params(65535, 65535, VJ_EXTRACT_GRAY);   // 257 x 4096 blocks per region: 2040 regions fit
        CHECK(vj_extract_affine_layout(fr.im.data(), 2, many.data(), 2041, &p, &c, &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "work units") != nullptr);
        CHECK(vj_extract_affine_layout(fr.im.data(), 2, many.data(), 2040, &p, &c, &bytes) == VJ_OK && c == 1);
    }
    // ---- a device-resident source that overlaps the destination (vj_extract_affine checks it with vj_preprocess's function)
    {
        uint8_t* const base = (uint8_t*)(uintptr_t)0x10000;   // (addresses only: nothing is read)
        std::vector<vj_image> f = {{base + 4096, 16, 4, 16, 1, 1}, {base + 8192, 5, 3, 20, 1, 3}, {base, 16, 4, 16, 0, 1}};
        CHECK(prep_check_overlap(f.data(), 3, base, 4096) == VJ_OK);
        CHECK(prep_check_overlap(f.data(), 3, base + 1, 4096) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr);
    }
    printf("affine_asan_driver: OK\n");
    return 0;
}
