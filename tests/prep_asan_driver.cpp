// Sanitizer driver of the host planner of vj_preprocess (csrc/vj_prep_host.cpp: the argument checks, the layout, the frame records
// and taps of a slice): built by tests/test_sanitizers_prep.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/prep_asan_driver.cpp csrc/vj_prep_host.cpp csrc/vj_atlas_host.cpp csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp
//       csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  The eleven sizes of tests/mixed_cases.py plus frames of widths 1 .. 9, to a fixed size, by factors (the ties of
// cvRound) and without a resize, whole and in slices: every image inside the buffer, none overlapping, offsets at multiples of 256,
// the work units — decoded as the kernels decode them — covering every dword of every row of every image once, every tap the kernel
// would load inside the taps table and naming source pixels inside the frame; then the error cases.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_prep_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static const int SIZES[][2] = {{240, 180}, {131, 97}, {141, 111}, {211, 61}, {67, 171}, {29, 29}, {155, 133}, {88, 88}, {240, 180}, {31, 22}, {127, 103}};
static uint8_t px[64];

static uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }

static std::vector<vj_image> frames_of_the_cases() {
    std::vector<vj_image> f;
    for (const auto& s : SIZES) f.push_back(vj_image{px, s[0], s[1], s[0], 0, 1});
    for (int w = 1; w <= 9; ++w) {
        const int ch = w % 3 == 0 ? 3 : w % 3 == 1 ? 4 : 1;
        f.push_back(vj_image{px, w, 1 + w % 5, w * ch + w % 2, 0, ch});
    }
    return f;
}

// the layout through the C entry point and through the planner, then every slice of `per_slice` frames, checked
static uint64_t plan_all(const std::vector<vj_image>& frames, const vj_prep& p, size_t per_slice) {
    const int n = (int)frames.size();
    std::vector<vj_image> out((size_t)n);
    uint64_t bytes = 1;
    CHECK(vj_preprocess_layout(frames.data(), n, &p, out.data(), &bytes) == VJ_OK);
    PrepLayout lay;
    CHECK(prep_layout(frames.data(), n, &p, &lay) == VJ_OK && lay.bytes == bytes && lay.slots.size() == (size_t)n);
    CHECK(lay.equalize == ((p.flags & VJ_PREP_EQUALIZE) != 0u));
    uint64_t end = 0;
    for (int i = 0; i < n; ++i) {
        const PrepSlot& t = lay.slots[(size_t)i];
        const vj_image& o = out[(size_t)i];
        CHECK((uint64_t)(uintptr_t)o.data == t.off && o.width == (int)t.dw && o.height == (int)t.dh && o.stride == (int)t.pitch && o.on_device == 1 && o.channels == 1);
        CHECK(t.dw >= 1u && t.dh >= 1u && t.pitch == align4(t.dw) && t.off % 256u == 0u && t.off >= end && t.off - end < 256u);
        if (p.dst_w > 0) CHECK((int)t.dw == p.dst_w && (int)t.dh == p.dst_h);
        else if (p.fx > 0) CHECK(t.dw == (uint32_t)std::max(1l, std::lrint(frames[(size_t)i].width * p.fx)) && t.dh == (uint32_t)std::max(1l, std::lrint(frames[(size_t)i].height * p.fy)));
        else CHECK((int)t.dw == frames[(size_t)i].width && (int)t.dh == frames[(size_t)i].height);
        end = t.off + (uint64_t)t.pitch * t.dh;
    }
    CHECK(end == bytes);
    std::vector<uint8_t> covered((size_t)bytes, 0);
    PrepSlice sl;
    for (size_t first = 0; first < (size_t)n; first += per_slice) {
        const size_t m = std::min(per_slice, (size_t)n - first);
        CHECK(prep_plan_slice(frames.data(), lay, first, m, &sl) == VJ_OK);
        CHECK(sl.recs.size() == m && sl.eq.size() == m && sl.taps.size() % 4u == 0u);
        uint64_t unit = 0;
        for (size_t i = 0; i < m; ++i) {
            const PrepFrameDev& d = sl.recs[i];
            const PrepSlot& t = lay.slots[first + i];
            CHECK(d.src == frames[first + i].data && d.stride == (uint32_t)frames[first + i].stride && d.channels == t.ch);
            CHECK(d.sw == t.sw && d.sh == t.sh && d.dw == t.dw && d.dh == t.dh && d.pitch == t.pitch && d.dst_off == t.off);
            CHECK(d.unit_first == unit && d.hist_slot == (uint32_t)i);
            CHECK(sl.eq[i].w == t.dw && sl.eq[i].h == t.dh);
            unit += prep_units(d.dw, d.dh);
            if (d.mode == PREP_COPY) {
                CHECK(d.sw == d.dw && d.sh == d.dh);
                continue;
            }
            CHECK(d.sw != d.dw || d.sh != d.dh);
            CHECK((d.mode == PREP_AREA) == (d.sw == 2u * d.dw && d.sh == 2u * d.dh));
            CHECK(d.xtab % 4u == 0u && (size_t)d.xtab + align4(d.dw) <= sl.taps.size() && (size_t)d.ytab + align4(d.dh) <= sl.taps.size());
            for (uint32_t x = 0; x < align4(d.dw); ++x) {   // (the pad taps repeat the last one)
                const PyrTap& tp = sl.taps[(size_t)d.xtab + x];
                CHECK(tp.i0 < d.sw && tp.i1 < d.sw);
                if (x >= d.dw) CHECK(memcmp(&tp, &sl.taps[(size_t)d.xtab + d.dw - 1u], sizeof(tp)) == 0);
                if (d.mode == PREP_AREA && x < d.dw) CHECK(tp.i0 == 2u * x && tp.i1 == 2u * x + 1u);
            }
            for (uint32_t y = 0; y < d.dh; ++y) CHECK(sl.taps[(size_t)d.ytab + y].i0 < d.sh && sl.taps[(size_t)d.ytab + y].i1 < d.sh);
        }
        CHECK(unit == sl.n_units);
        // the units as the kernels decode them: a binary search of the unit prefix, then block, wave and lane -> the dword (dx, dy)
        for (uint32_t u0 = 0; u0 < sl.n_units; ++u0) {
            uint32_t lo = 0, hi = (uint32_t)m;
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (sl.recs[mid].unit_first <= u0) lo = mid;
                else hi = mid;
            }
            const PrepFrameDev& d = sl.recs[lo];
            const uint32_t bpr = (d.dw + PREP_BLOCK_W - 1u) / PREP_BLOCK_W, u = u0 - d.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            CHECK(by * PREP_BLOCK_H < d.dh && bx * PREP_BLOCK_W < d.dw);   // lane 0 of every wave's first row holds pixels
            for (uint32_t tid = 0; tid < 256u; ++tid) {
                const uint32_t dx = bx * PREP_BLOCK_W + (tid & 63u) * 4u;
                if (dx >= d.dw) continue;
                for (uint32_t dy = by * PREP_BLOCK_H + (tid >> 6); dy < std::min((by + 1u) * PREP_BLOCK_H, d.dh); dy += 4u) {
                    const uint64_t at = d.dst_off + (uint64_t)dy * d.pitch + dx;
                    CHECK(at % 4u == 0u && at + 4u <= bytes);
                    for (uint32_t k = 0; k < 4u; ++k) {
                        CHECK(covered[(size_t)at + k] == 0);                    // no two images overlap, no dword twice
                        covered[(size_t)at + k] = 1;
                    }
                }
            }
        }
    }
    for (int i = 0; i < n; ++i) {                                               // every dword of every row of every image, once
        const PrepSlot& t = lay.slots[(size_t)i];
        for (uint64_t b = 0; b < (uint64_t)t.pitch * t.dh; ++b) CHECK(covered[(size_t)(t.off + b)] == 1);
    }
    return bytes;
}

static vj_prep prep(int dw, int dh, double fx, double fy, uint32_t flags, uint32_t reserved = 0) {
    vj_prep p;
    memset(&p, 0xff, sizeof(p));
    vj_prep_default(&p);
    CHECK(p.dst_w == 0 && p.dst_h == 0 && p.fx == 0 && p.fy == 0 && p.flags == 0u && p.reserved == 0u);
    p.dst_w = dw;
    p.dst_h = dh;
    p.fx = fx;
    p.fy = fy;
    p.flags = flags;
    p.reserved = reserved;
    return p;
}

int main() {
    const std::vector<vj_image> frames = frames_of_the_cases();
    const size_t n = frames.size();
    // ---- a fixed size (up-scaling of the small frames included), factors, no resize; whole, in slices of 4 and one by one
    for (size_t per : {n, (size_t)4, (size_t)1}) {
        plan_all(frames, prep(120, 90, 0, 0, VJ_PREP_EQUALIZE), per);       // the two 240 x 180 frames: exactly half, the 2 x 2 mean
        plan_all(frames, prep(5, 3, 0, 0, VJ_PREP_EQUALIZE), per);
        plan_all(frames, prep(257, 2, 0, 0, 0), per);
        plan_all(frames, prep(0, 0, 0.5, 0.5, VJ_PREP_EQUALIZE), per);
        plan_all(frames, prep(0, 0, 1.0, 1.0, 0), per);                     // the identity: copies
        plan_all(frames, prep(0, 0, 2.5, 0.3, 0), per);
        plan_all(frames, prep(0, 0, 1e-9, 1e-9, VJ_PREP_EQUALIZE), per);    // everything to 1 x 1
        plan_all(frames, prep(0, 0, 0, 0, VJ_PREP_EQUALIZE), per);
        plan_all(frames, prep(9, 8, 0.5, 0.5, 0), per);                     // dst_w / dst_h come first
    }
    {   // the ties: 5 x 0.5 gives 2, 7 x 0.5 gives 4
        const std::vector<vj_image> f = {{px, 5, 7, 5, 0, 1}, {px, 7, 5, 7, 0, 1}, {px, 1, 1, 1, 0, 1}};
        const vj_prep p = prep(0, 0, 0.5, 0.5, 0);
        vj_image out[3];
        uint64_t bytes = 0;
        CHECK(vj_preprocess_layout(f.data(), 3, &p, out, &bytes) == VJ_OK);
        CHECK(out[0].width == 2 && out[0].height == 4 && out[1].width == 4 && out[1].height == 2 && out[2].width == 1 && out[2].height == 1);
        CHECK(bytes == 512u + 4u);
        plan_all(f, p, 3);
    }
    {   // widths 1 .. 9 of one height to every width 1 .. 9
        std::vector<vj_image> f;
        for (int w = 1; w <= 9; ++w) f.push_back(vj_image{px, w, 3, w, 0, 1});
        for (int w = 1; w <= 9; ++w) plan_all(f, prep(w, 1 + w % 3, 0, 0, VJ_PREP_EQUALIZE), f.size());
    }
    {   // no frames
        const vj_prep p = prep(0, 0, 0, 0, 0);
        uint64_t bytes = 5;
        CHECK(vj_preprocess_layout(nullptr, 0, &p, nullptr, &bytes) == VJ_OK && bytes == 0);
    }

    // ---- the error cases
    const vj_prep ok = prep(0, 0, 0.5, 0.5, VJ_PREP_EQUALIZE);
    std::vector<vj_image> out(n + 1);
    uint64_t bytes = 0;
    CHECK(vj_preprocess_layout(nullptr, 1, &ok, out.data(), &bytes) == VJ_ERR_ARG);
    CHECK(vj_preprocess_layout(frames.data(), (int)n, nullptr, out.data(), &bytes) == VJ_ERR_ARG);
    CHECK(vj_preprocess_layout(frames.data(), (int)n, &ok, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_preprocess_layout(frames.data(), (int)n, &ok, out.data(), nullptr) == VJ_ERR_ARG);
    CHECK(vj_preprocess_layout(frames.data(), -1, &ok, out.data(), &bytes) == VJ_ERR_ARG);
    const vj_image bad[] = {{nullptr, 4, 4, 4, 0, 1}, {px, 0, 4, 4, 0, 1}, {px, 4, -1, 4, 0, 1}, {px, 4, 4, 3, 0, 1}, {px, 4, 4, 11, 0, 3}, {px, 4, 4, 8, 0, 2}};
    for (const vj_image& b : bad) {
        const std::vector<vj_image> v = {frames[0], frames[1], b};
        bytes = 9;
        CHECK(vj_preprocess_layout(v.data(), 3, &ok, out.data(), &bytes) == VJ_ERR_ARG && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr);
    }
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    struct { vj_prep p; const char* word; } bad_p[] = {
        {prep(5, 0, 0, 0, 0), "dst_w"}, {prep(0, 5, 0, 0, 0), "dst_h"}, {prep(-5, -5, 0, 0, 0), "dst_w"}, {prep(5, -1, 0, 0, 0), "dst_h"},
        {prep(0, 0, 0.5, 0, 0), "fx"}, {prep(0, 0, 0, 0.5, 0), "fy"}, {prep(0, 0, -0.5, -0.5, 0), "fx"}, {prep(0, 0, 0.5, -0.5, 0), "fy"},
        {prep(0, 0, inf, 1, 0), "fx"}, {prep(0, 0, 1, nan, 0), "fy"}, {prep(0, 0, -inf, -inf, 0), "fx"}, {prep(4, 4, nan, nan, 0), "fx"},
        {prep(0, 0, 0, 0, 2u), "flags"}, {prep(0, 0, 0, 0, 0x80000001u), "flags"}, {prep(0, 0, 0, 0, 0, 1u), "reserved"}};
    for (const auto& b : bad_p) {
        CHECK(vj_preprocess_layout(frames.data(), (int)n, &b.p, out.data(), &bytes) == VJ_ERR_ARG);
        CHECK(strstr(vj_last_error(), b.word) != nullptr);
        CHECK(vj_preprocess_layout(nullptr, 0, &b.p, nullptr, &bytes) == VJ_ERR_ARG);
    }
    // ---- the limits: sides up to 65535, work units within a 32-bit index
    {
        const std::vector<vj_image> f = {{px, 65535, 1, 65535, 0, 1}};
        vj_prep p = prep(65535, 65535, 0, 0, 0);
        CHECK(vj_preprocess_layout(f.data(), 1, &p, out.data(), &bytes) == VJ_OK && bytes == 65536ull * 65535ull);
        const vj_image big[] = {{px, 65536, 1, 65536, 0, 1}, {px, 1, 65536, 1, 0, 1}};
        for (const vj_image& b : big) {
            p = prep(0, 0, 0, 0, 0);
            CHECK(vj_preprocess_layout(&b, 1, &p, out.data(), &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "frame 0") != nullptr);
        }
        for (const vj_prep& q : {prep(65536, 1, 0, 0, 0), prep(1, 65536, 0, 0, 0), prep(0, 0, 8192.5, 1, 0), prep(0, 0, 1, 1e300, 0), prep(2147483647, 2147483647, 0, 0, 0)})
            CHECK(vj_preprocess_layout(frames.data(), 1, &q, out.data(), &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "65535") != nullptr);
        std::vector<vj_image> many(4097, vj_image{px, 4, 4, 4, 0, 1});
        std::vector<vj_image> out_many(many.size());
        p = prep(65535, 65535, 0, 0, 0);
        CHECK(vj_preprocess_layout(many.data(), 4097, &p, out_many.data(), &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "work units") != nullptr);
        CHECK(vj_preprocess_layout(many.data(), 4095, &p, out_many.data(), &bytes) == VJ_OK);
    }
    // ---- a device-resident source that overlaps the destination
    {
        uint8_t* const base = (uint8_t*)(uintptr_t)0x10000;   // (addresses only: nothing is read)
        std::vector<vj_image> f = {{base + 4096, 16, 4, 16, 1, 1}, {base + 8192, 5, 3, 20, 1, 3}, {base, 16, 4, 16, 0, 1}};
        CHECK(prep_check_overlap(f.data(), 3, base, 4096) == VJ_OK);            // ends where frame 0 begins; the host frame is not looked at
        CHECK(prep_check_overlap(f.data(), 3, base, 4097) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr);
        CHECK(prep_check_overlap(f.data(), 3, base + 4096 + 64, 100) == VJ_OK);  // begins where frame 0 ends
        CHECK(prep_check_overlap(f.data(), 3, base + 4096 + 63, 100) == VJ_ERR_ARG);
        CHECK(prep_check_overlap(f.data(), 3, base + 8192 + 2 * 20 + 14, 1) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 1") != nullptr);   // its last byte
        CHECK(prep_check_overlap(f.data(), 3, base + 8192 + 2 * 20 + 15, 1) == VJ_OK);                                                     // a source ends with its last row
        CHECK(prep_check_overlap(f.data(), 0, base, 1 << 20) == VJ_OK);
    }
    printf("prep_asan_driver: OK\n");
    return 0;
}
