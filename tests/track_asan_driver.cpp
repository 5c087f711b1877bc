// Sanitizer driver of the host planner of vj_track (csrc/vj_track_host.cpp: the argument checks, the two vj_extract layouts, the
// scratch layout, the slices, the box of a match) and the planners it uses: built by tests/test_sanitizers_track.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/track_asan_driver.cpp csrc/vj_track_host.cpp csrc/vj_extract_host.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp
//       csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Rows inside, across and outside frames of three channel counts, forward, backward and at their own frame, the
// ends of t and r and pairs between, whole and in slices.  The scratch is a heap block of exactly the layout's bytes: every patch
// the extraction records point at lies inside it, at a multiple of 16, none overlapping another; and the index arithmetic of the
// match kernel (vj_track.hip) is walked with the kernel's own index functions (csrc/vj_track_units.hpp) — every dword it loads from
// scratch is read here, so ASan sees each access, every LDS index is checked against the arrays' sizes, every displacement is owned
// by exactly one lane's unit.  Then the error cases.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_track_host.hpp"

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

static vj_track_params params(int t, int r, double sx, double sy, uint32_t flags = 0, uint32_t reserved = 0) {
    vj_track_params p;
    memset(&p, 0xff, sizeof(p));
    vj_track_default(&p);
    CHECK(p.tmpl == 32 && p.radius == 8 && p.sx == 0 && p.sy == 0 && p.flags == 0u && p.reserved == 0u);
    p.tmpl = t;
    p.radius = r;
    p.sx = sx;
    p.sy = sy;
    p.flags = flags;
    p.reserved = reserved;
    return p;
}

// The match kernel's walk over one row's patches, with the kernel's own index functions and array sizes (vj_track_units.hpp,
// which vj_track.hip includes too): what is checked here is what the kernel computes, not a copy of it.
static void walk_match(const uint8_t* tmpl, const uint8_t* search, uint32_t t, uint32_t r) {
    const TrackGeom g = track_geom(t, r);
    CHECK((g.P * g.P) % 4u == 0u && g.n_t <= TRACK_T_DWORDS && g.n_sl + TRACK_S_PAD <= TRACK_S_DWORDS);
    CHECK(((uintptr_t)tmpl & 3u) == 0u && ((uintptr_t)search & 3u) == 0u);
    std::vector<uint8_t> loaded((size_t)g.P * g.P, 0);
    for (uint32_t i = 0; i < g.n_t; ++i)
        for (int b = 0; b < 4; ++b) sink = sink + tmpl[4u * i + (uint32_t)b];
    for (uint32_t i = 0; i < g.n_sl; ++i) {
        const TrackFill f = track_fill(g, i);
        const uint32_t y = i / g.Pd, q = i - y * g.Pd, off = y * g.P + 4u * q;
        CHECK(y < g.P && (f.phase == 0u || f.phase == 2u) && f.phase == (off & 3u) && f.lo < g.n_s && f.hi < g.n_s);
        for (int b = 0; b < 4; ++b) sink = sink + search[4u * f.lo + (uint32_t)b];
        if (f.phase != 0u)
            for (int b = 0; b < 4; ++b) sink = sink + search[4u * f.hi + (uint32_t)b];
        // the bytes of row y that exist among the dword's four: each comes from the dword the fill reads it from
        for (uint32_t b = 0; b < 4u && 4u * q + b < g.P; ++b) {
            const uint32_t at = off + b, from = f.phase + b < 4u ? f.lo : f.hi;
            CHECK(at < g.P * g.P && at / 4u == from && (f.phase + b) % 4u == at % 4u);
            loaded[(size_t)y * g.P + 4u * q + b] = 1;
        }
    }
    for (uint8_t v : loaded) CHECK(v == 1);
    std::vector<uint8_t> owned((size_t)g.side * g.side, 0);
    for (uint32_t tid = 0; tid < TRACK_THREADS; ++tid)
        for (uint32_t unit = tid; unit < g.n_units; unit += TRACK_THREADS) {
            uint32_t dyi, u;
            track_unit(g, unit, &dyi, &u);
            CHECK(dyi < g.side && u < g.U);
            for (uint32_t i = 0; i < t; ++i) {
                const uint32_t sb = track_s_base(g, i, dyi, u), tb = track_t_base(g, i);
                CHECK(tb + g.td <= g.n_t && sb + g.td < g.n_sl + TRACK_S_PAD);   // the window's second dword: at most one past the patch's rows
                // the bytes a valid displacement compares lie inside row i + dyi of the patch
                for (uint32_t q = 0; q < 4u && 4u * u + q < g.side; ++q) CHECK(4u * u + q + t <= g.P && i + dyi < g.P && sb == (i + dyi) * g.Pd + u);
            }
            for (uint32_t q = 0; q < 4u; ++q) {
                const uint32_t dxi = 4u * u + q;
                if (dxi >= g.side) continue;
                CHECK(owned[(size_t)dyi * g.side + dxi] == 0);
                owned[(size_t)dyi * g.side + dxi] = 1;
                const int32_t dx = (int32_t)dxi - (int32_t)r, dy = (int32_t)dyi - (int32_t)r;
                const uint64_t key = track_key(g, 1044480u, dyi, dxi);   // the fields do not run into each other
                CHECK((key >> 32) == 1044480u && ((key >> 16) & 0xffffu) == (uint32_t)(dx * dx + dy * dy) && ((key >> 8) & 0xffu) == dyi && (key & 0xffu) == dxi);
            }
        }
    for (uint8_t v : owned) CHECK(v == 1);
}

static void plan_all(const Frames& fr, const std::vector<vj_track_row>& rows, const vj_track_params& p, size_t max_frames) {
    const int nf = (int)fr.im.size(), n = (int)rows.size();
    std::vector<vj_roi> tr((size_t)n + 1), sr((size_t)n + 1);
    uint64_t bytes = 1;
    CHECK(vj_track_layout(fr.im.data(), nf, rows.data(), n, &p, tr.data(), sr.data(), &bytes) == VJ_OK);
    TrackLayout lay;
    CHECK(track_layout(fr.im.data(), nf, rows.data(), n, &p, &lay) == VJ_OK && lay.scratch_bytes == bytes);
    const uint32_t t = (uint32_t)p.tmpl, r = (uint32_t)p.radius, P = t + 2u * r;
    CHECK(lay.t == t && lay.r == r && lay.tmpl.gray && lay.search.gray && lay.tmpl.C == 1u && lay.search.C == 1u);
    CHECK(lay.tmpl.region_bytes == (uint64_t)t * t && lay.tmpl.region_pitch == lay.tmpl.region_bytes && lay.tmpl.region_bytes % 16u == 0u);
    CHECK(lay.search.region_bytes == (uint64_t)P * P && lay.search.region_pitch % 16u == 0u && lay.search.region_pitch >= lay.search.region_bytes &&
          lay.search.region_pitch < lay.search.region_bytes + 16u);
    CHECK(lay.tmpl_off == 0 && lay.search_off == (uint64_t)n * t * t && bytes == lay.search_off + (uint64_t)n * lay.search.region_pitch);
    const double sx = p.sx == 0 ? 1 : p.sx, sy = p.sy == 0 ? 1 : p.sy, margin = (double)r / t;
    for (int k = 0; k < n; ++k) {
        const vj_track_row& g = rows[(size_t)k];
        const vj_roi &a = lay.tmpl.src[(size_t)k], &s = lay.search.src[(size_t)k];
        CHECK(memcmp(&a, &tr[(size_t)k], sizeof(a)) == 0 && memcmp(&s, &sr[(size_t)k], sizeof(s)) == 0);
        const long w0 = std::max(1l, std::lrint(g.w * sx)), h0 = std::max(1l, std::lrint(g.h * sy));
        const long mx = std::lrint((double)w0 * margin), my = std::lrint((double)h0 * margin);
        CHECK(a.frame == g.src_frame && a.x == std::lrint(g.x * sx) && a.y == std::lrint(g.y * sy) && a.w == w0 && a.h == h0);
        CHECK(s.frame == g.dst_frame && s.x == a.x - mx && s.y == a.y - my && s.w == w0 + 2 * mx && s.h == h0 + 2 * my);
        if (w0 == (long)t) CHECK(mx == (long)r);   // a box of the template's size is searched at identity
        // the box of a match at the corners of the search range
        for (int dy : {-(int)r, 0, (int)r})
            for (int dx : {-(int)r, 0, (int)r}) {
                vj_track_result o;
                track_result(lay, (size_t)k, TrackMatchDev{dx, dy, 5u, 7u}, &o);
                CHECK(o.dx == dx && o.dy == dy && o.sad == 5u && o.sad0 == 7u && o.w == a.w && o.h == a.h);
                CHECK(o.x == a.x + std::lrint(dx * (double)s.w / P) && o.y == a.y + std::lrint(dy * (double)s.h / P));
                if (dx == (int)r) CHECK(std::labs((long)o.x - a.x - mx) <= 1);   // r patch pixels are the margin
            }
    }
    // the scratch: a heap block of exactly the layout's bytes, at a multiple of 16 like a device allocation
    std::unique_ptr<uint8_t[]> block(new uint8_t[(size_t)bytes + 16u]);
    uint8_t* scratch = block.get() + ((16u - ((uintptr_t)block.get() & 15u)) & 15u);
    // (only [scratch, scratch + bytes) is touched below; the spare bytes behind it are what the alignment did not use)
    memset(scratch, 0x5a, (size_t)bytes);
    std::vector<uint8_t> claimed((size_t)bytes, 0);
    ExtractSlice sl;
    size_t slices = 0;
    for (size_t first = 0; first < (size_t)n; ++slices) {
        const size_t end = track_slice_end(rows.data(), (size_t)n, first, max_frames);
        CHECK(end > first && end <= (size_t)n);
        std::vector<int> seen;
        for (size_t k = first; k < end; ++k)
            for (int f : {rows[k].src_frame, rows[k].dst_frame})
                if (std::find(seen.begin(), seen.end(), f) == seen.end()) seen.push_back(f);
        if (max_frames) {
            CHECK(seen.size() <= max_frames || end == first + 1);   // (a row that names two frames is a slice of its own under a bound of 1)
            if (end < (size_t)n) {   // greedy: the next row would take the slice over the bound
                std::vector<int> more = seen;
                for (int f : {rows[end].src_frame, rows[end].dst_frame})
                    if (std::find(more.begin(), more.end(), f) == more.end()) more.push_back(f);
                CHECK(more.size() > max_frames);
            }
        } else {
            CHECK(end == (size_t)n);
        }
        for (int which = 0; which < 2; ++which) {
            const ExtractLayout& el = which ? lay.search : lay.tmpl;
            const std::vector<vj_roi>& regions = which ? lay.search_regions : lay.tmpl_regions;
            const uint64_t off = which ? lay.search_off : lay.tmpl_off;
            CHECK(extract_plan_slice(fr.im.data(), regions.data(), el, first, end - first, &sl) == VJ_OK && sl.recs.size() == end - first);
            for (size_t i = 0; i < end - first; ++i) {
                const ExtractRegionDev& d = sl.recs[i];
                CHECK(d.dst_off == (first + i) * el.region_pitch && d.dst_off + el.region_bytes <= el.bytes && (off + d.dst_off) % 16u == 0u);
                CHECK(off + d.dst_off + el.region_bytes <= bytes);
                for (uint64_t b = 0; b < el.region_bytes; ++b) {
                    CHECK(claimed[(size_t)(off + d.dst_off + b)] == 0);   // no byte of the scratch belongs to two patches
                    claimed[(size_t)(off + d.dst_off + b)] = 1;
                }
                CHECK(d.src == fr.im[(size_t)regions[first + i].frame].data && d.cw == (uint32_t)el.src[first + i].w && d.ch == (uint32_t)el.src[first + i].h);
            }
        }
        for (size_t k = first; k < end; ++k) walk_match(scratch + lay.tmpl_off + k * (size_t)t * t, scratch + lay.search_off + k * lay.search.region_pitch, t, r);
        first = end;
    }
    if (max_frames == 0 && n > 0) CHECK(slices == 1);
}

int main() {
    Frames fr;
    fr.add(37, 29, 1, 3);
    fr.add(41, 33, 3, 0);
    fr.add(37, 29, 4, 1);
    fr.add(9, 4, 3, 2);
    std::vector<vj_track_row> rows;
    const int boxes[][4] = {{8, 6, 20, 17}, {3, 4, 1, 1}, {-5, 8, 10, 10}, {30, 8, 10, 10}, {8, -5, 10, 10}, {8, 25, 10, 10}, {-3, -3, 10, 10},
                            {30, 22, 10, 10}, {100, 100, 6, 6}, {-40, 3, 6, 6}, {0, 0, 37, 29}, {5, 5, 24, 24}, {2, 2, 8, 8}, {1, 1, 64, 64}};
    int k = 0;
    for (const auto& b : boxes)
        for (int rep = 0; rep < 2; ++rep, ++k) {
            const int src = k % 4, dst = (src + (k % 3 == 0 ? 0 : k % 3 == 1 ? 1 : 3)) % 4;   // its own frame, forward, backward
            rows.push_back(vj_track_row{src, dst, b[0], b[1], b[2], b[3]});
        }
    const int tr[][2] = {{8, 1}, {8, 16}, {64, 1}, {64, 16}, {12, 3}, {36, 7}, {32, 8}, {24, 5}, {16, 4}, {64, 15}, {60, 16}};
    for (const auto& q : tr)
        for (size_t per : {(size_t)0, (size_t)1, (size_t)2, (size_t)3}) {
            plan_all(fr, rows, params(q[0], q[1], 1, 1), per);
            plan_all(fr, rows, params(q[0], q[1], 1.8, 0.5), per);
            plan_all(fr, rows, params(q[0], q[1], 0, 0), per);
        }
    plan_all(fr, {}, params(32, 8, 1, 1), 0);
    plan_all(fr, {rows[0]}, params(32, 8, 1, 1), 1);

    // ---- the error cases
    const std::vector<vj_track_row> good = {{0, 1, 0, 0, 4, 4}, {1, 1, 1, 1, 2, 2}};
    const vj_track_params ok = params(32, 8, 1, 1);
    vj_roi a[8], s[8];
    uint64_t bytes = 0;
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, &ok, a, s, &bytes) == VJ_OK && bytes == 2u * 1024u + 2u * 2304u);
    CHECK(vj_track_layout(nullptr, 4, good.data(), 2, &ok, a, s, &bytes) == VJ_ERR_ARG && bytes == 0);
    CHECK(vj_track_layout(fr.im.data(), 4, nullptr, 2, &ok, a, s, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, nullptr, a, s, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, &ok, nullptr, s, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, &ok, a, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, &ok, a, s, nullptr) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), -1, good.data(), 2, &ok, a, s, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(fr.im.data(), 4, good.data(), -1, &ok, a, s, &bytes) == VJ_ERR_ARG);
    CHECK(vj_track_layout(nullptr, 0, nullptr, 0, &ok, nullptr, nullptr, &bytes) == VJ_OK && bytes == 0);
    const vj_image bad_f[] = {{nullptr, 4, 4, 4, 0, 1}, {fr.im[0].data, 0, 4, 4, 0, 1}, {fr.im[0].data, 4, -1, 4, 0, 1}, {fr.im[0].data, 4, 4, 3, 0, 1},
                              {fr.im[0].data, 4, 4, 11, 0, 3}, {fr.im[0].data, 4, 4, 8, 0, 2}};
    for (const vj_image& b : bad_f) {
        const std::vector<vj_image> v = {fr.im[0], fr.im[1], b};
        bytes = 9;
        CHECK(vj_track_layout(v.data(), 3, good.data(), 2, &ok, a, s, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr);
    }
    struct { vj_track_row r; const char* word; } bad_r[] = {{{4, 0, 0, 0, 4, 4}, "src_frame"}, {{-1, 0, 0, 0, 4, 4}, "src_frame"}, {{0, 4, 0, 0, 4, 4}, "dst_frame"},
                                                            {{0, -2147483647 - 1, 0, 0, 4, 4}, "dst_frame"}, {{0, 1, 0, 0, 0, 4}, "region 2"},
                                                            {{0, 1, 0, 0, 4, 0}, "region 2"}, {{1, 0, 0, 0, -3, 4}, "region 2"}};
    for (const auto& b : bad_r) {
        const std::vector<vj_track_row> v = {good[0], good[1], b.r};
        CHECK(vj_track_layout(fr.im.data(), 4, v.data(), 3, &ok, a, s, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), b.word) != nullptr && strstr(vj_last_error(), " 2") != nullptr);
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct { vj_track_params p; const char* word; } bad_p[] = {
        {params(4, 8, 1, 1), "tmpl"}, {params(68, 8, 1, 1), "tmpl"}, {params(30, 8, 1, 1), "tmpl"}, {params(0, 8, 1, 1), "tmpl"}, {params(-32, 8, 1, 1), "tmpl"},
        {params(2147483644, 8, 1, 1), "tmpl"}, {params(32, 0, 1, 1), "radius"}, {params(32, 17, 1, 1), "radius"}, {params(32, -1, 1, 1), "radius"},
        {params(32, 2147483647, 1, 1), "radius"}, {params(32, 8, 1, 1, 1u), "flags"}, {params(32, 8, 1, 1, 0x80000000u), "flags"},
        {params(32, 8, 1, 1, 0, 1u), "reserved"}, {params(32, 8, -0.5, 1), "sx"}, {params(32, 8, 1, -0.5), "sy"}, {params(32, 8, inf, 1), "sx"},
        {params(32, 8, 1, nan), "sy"}, {params(32, 8, nan, nan), "sx"}};
    for (const auto& b : bad_p) {
        CHECK(vj_track_layout(fr.im.data(), 4, good.data(), 2, &b.p, a, s, &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), b.word) != nullptr);
        CHECK(vj_track_layout(nullptr, 0, nullptr, 0, &b.p, nullptr, nullptr, &bytes) == VJ_ERR_ARG);
    }
    // ---- the limits are vj_extract's: sides up to 65535 with the margin, coordinates within +-2^24
    {
        const vj_track_row big = {0, 1, 0, 0, 43690, 43690};   // 43690 + 2 * cvRound(43690 / 4) = 65534
        CHECK(vj_track_layout(fr.im.data(), 4, &big, 1, &ok, a, s, &bytes) == VJ_OK && s[0].w == 65534);
        struct { vj_track_row r; vj_track_params p; const char* word; } lim[] = {
            {{0, 1, 0, 0, 65536, 4}, ok, "65535"}, {{0, 1, 0, 0, 4, 65536}, ok, "65535"}, {{0, 1, 0, 0, 43692, 4}, ok, "65535"},
            {{0, 1, 0, 0, 4, 60000}, params(8, 16, 1, 1), "65535"}, {{0, 1, 0, 0, 40000, 4}, params(32, 8, 2, 1), "65535"},
            {{0, 1, 0, 0, 4, 40000}, params(32, 8, 1, 2), "65535"}, {{0, 1, (1 << 24) + 1, 0, 4, 4}, ok, "2^24"},
            {{0, 1, 0, -(1 << 24) - 1, 4, 4}, ok, "2^24"}, {{0, 1, -(1 << 24), 0, 400, 4}, ok, "2^24"}};
        for (const auto& b : lim) {
            const std::vector<vj_track_row> v = {good[0], b.r};
            CHECK(vj_track_layout(fr.im.data(), 4, v.data(), 2, &b.p, a, s, &bytes) == VJ_ERR_LIMIT && bytes == 0);
            CHECK(strstr(vj_last_error(), b.word) != nullptr && strstr(vj_last_error(), "region 1") != nullptr);
        }
    }
    printf("track_asan_driver: OK\n");
    return 0;
}
