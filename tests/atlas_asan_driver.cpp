// Sanitizer driver of the host planner of the mixed-size entry points (csrc/vj_atlas_host.cpp): built by
// tests/test_sanitizers_atlas.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/atlas_asan_driver.cpp csrc/vj_atlas_host.cpp csrc/vj_cascade.cpp
// (no HIP involved).  The eleven sizes of tests/mixed_cases.py plus frames of widths 1 .. 9, planned with the library's budget, with
// one that splits the frames over three atlases and with one smaller than the largest frame: every slot inside its atlas, no two
// overlapping, origins at multiples of 4 columns, the pack units — decoded as the kernel decodes them — covering every dword of every
// row of every frame once, the oversized frames and the own-call groups reported, the atlas dimensions on the ladder.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_atlas_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static const int SIZES[][2] = {{240, 180}, {131, 97}, {141, 111}, {211, 61}, {67, 171}, {29, 29}, {155, 133}, {88, 88}, {240, 180}, {31, 22}, {127, 103}};

struct Totals { size_t atlases = 0, frames = 0; std::vector<int> oversized; uint32_t max_w = 0, max_h = 0; };

static uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }

// every atlas of the list, checked
static Totals plan_all(const std::vector<AtlasSize>& sizes, const std::vector<int>& order, uint64_t budget, int max_frames) {
    Totals t;
    AtlasPlan pl;
    std::vector<uint8_t> seen_frame(sizes.size(), 0);
    for (size_t pos = 0; pos < order.size(); pos += pl.n_frames) {
        CHECK(atlas_plan(sizes, order, pos, budget, max_frames, &pl) == VJ_OK);
        CHECK(pl.n_frames >= 1 && pos + pl.n_frames <= order.size());
        if (pl.oversized) {
            CHECK(pl.n_frames == 1 && pl.slots.empty() && pl.n_units == 0u);
            t.oversized.push_back(order[pos]);
            continue;
        }
        CHECK(max_frames <= 0 || pl.n_frames <= (size_t)max_frames);
        CHECK(pl.slots.size() == pl.n_frames && pl.pitch == pl.w && pl.pitch % 4u == 0u);
        CHECK(pl.h < 65535u && (uint64_t)(pl.w + 1u) * (pl.h + 3ull) < (1ull << 30));
        CHECK(atlas_ladder(pl.w) == pl.w && atlas_ladder(pl.h) == pl.h);   // on the ladder
        std::vector<uint8_t> covered((size_t)pl.pitch * pl.h, 0);
        uint64_t unit = 0, slot_px = 0;
        for (size_t i = 0; i < pl.slots.size(); ++i) {
            const AtlasSlot& s = pl.slots[i];
            CHECK(s.frame == order[pos + i] && !seen_frame[(size_t)s.frame]);   // in the order taken, each frame once
            seen_frame[(size_t)s.frame] = 1;
            CHECK((int)s.w == sizes[(size_t)s.frame].w && (int)s.h == sizes[(size_t)s.frame].h);
            CHECK(s.ox % 4u == 0u && s.ox + align4(s.w) <= pl.w && s.oy + s.h <= pl.h);
            for (uint32_t y = 0; y < s.h; ++y)
                for (uint32_t x = 0; x < align4(s.w); ++x) {
                    uint8_t& c = covered[(size_t)(s.oy + y) * pl.pitch + s.ox + x];
                    CHECK(c == 0);                                             // no two slots overlap
                    c = 1;
                }
            slot_px += (uint64_t)align4(s.w) * s.h;
            CHECK(s.unit_first == unit);
            unit += (uint64_t)((s.w + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W) * ((s.h + ATLAS_BLOCK_H - 1u) / ATLAS_BLOCK_H);
        }
        CHECK(unit == pl.n_units);
        CHECK(slot_px <= budget);                                               // the slots stay within the budget
        // the units as atlas_pack decodes them: a binary search of the unit prefix, then block and thread -> the dword (dx, dy)
        std::vector<std::vector<uint8_t>> hit(pl.slots.size());
        for (size_t i = 0; i < pl.slots.size(); ++i) hit[i].assign((size_t)(align4(pl.slots[i].w) / 4u) * pl.slots[i].h, 0);
        for (uint32_t u0 = 0; u0 < pl.n_units; ++u0) {
            uint32_t lo = 0, hi = (uint32_t)pl.slots.size();
            while (hi - lo > 1u) {
                const uint32_t mid = (lo + hi) >> 1;
                if (pl.slots[mid].unit_first <= u0) lo = mid;
                else hi = mid;
            }
            const AtlasSlot& s = pl.slots[lo];
            const uint32_t bpr = (s.w + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W, u = u0 - s.unit_first;
            const uint32_t by = u / bpr, bx = u - by * bpr;
            for (uint32_t tid = 0; tid < 256u; ++tid) {
                const uint32_t dx = bx * ATLAS_BLOCK_W + (tid & 63u) * 4u, dy = by * ATLAS_BLOCK_H + (tid >> 6);
                if (dy >= s.h || dx >= s.w) continue;
                CHECK(s.ox + dx + 4u <= pl.pitch && s.oy + dy < pl.h);
                uint8_t& c = hit[lo][(size_t)dy * (align4(s.w) / 4u) + dx / 4u];
                CHECK(c == 0);
                c = 1;
            }
        }
        for (const auto& h : hit)
            for (uint8_t c : h) CHECK(c == 1);                                  // every dword of every row of every frame, once
        t.atlases += 1;
        t.frames += pl.n_frames;
        if ((uint64_t)pl.w * pl.h > (uint64_t)t.max_w * t.max_h) { t.max_w = pl.w; t.max_h = pl.h; }
    }
    return t;
}

int main() {
    // ---- the ladder: at or above v, at most a quarter and one step of 32 more, monotone, idempotent
    uint32_t prev = 0;
    for (uint32_t v = 1; v <= 70000u; ++v) {
        const uint32_t l = atlas_ladder(v);
        CHECK(l >= v && l <= v + v / 4u + 32u && l >= prev && atlas_ladder(l) == l && l % 32u == 0u);
        prev = l;
    }
    CHECK(atlas_ladder(1) == 32u && atlas_ladder(240) == 256u && atlas_ladder(180) == 192u && atlas_ladder(1081) == 1280u);

    std::vector<AtlasSize> sizes;
    for (const auto& s : SIZES) sizes.push_back(AtlasSize{s[0], s[1], 1});
    for (int w = 1; w <= 9; ++w) sizes.push_back(AtlasSize{w, 1 + w % 5, w % 3 == 0 ? 3 : w % 3 == 1 ? 4 : 1});
    std::vector<int> order(sizes.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;

    // ---- the library's budget: one atlas holds everything
    Totals t = plan_all(sizes, order, ATLAS_DEFAULT_PX, 0);
    CHECK(t.atlases == 1 && t.frames == sizes.size() && t.oversized.empty());
    // ... frames per atlas capped ("max_subbatch")
    t = plan_all(sizes, order, ATLAS_DEFAULT_PX, 2);
    CHECK(t.atlases == (sizes.size() + 1) / 2 && t.frames == sizes.size() && t.oversized.empty());
    // ---- a budget that splits the frames over three atlases
    t = plan_all(sizes, order, 70000u, 0);
    CHECK(t.atlases == 3 && t.frames == sizes.size() && t.oversized.empty());
    // ---- a budget smaller than the largest frame: the two 240 x 180 frames fit no empty atlas, the others make three
    t = plan_all(sizes, order, 42000u, 0);
    CHECK(t.oversized.size() == 2 && t.oversized[0] == 0 && t.oversized[1] == 8 && t.frames == sizes.size() - 2 && t.atlases == 3);
    // ... and one that holds a frame of 32 x 32 at most: the two tiny frames and the narrow ones still fit
    t = plan_all(sizes, order, 1024u, 0);
    CHECK(t.frames + t.oversized.size() == sizes.size() && t.oversized.size() == 9);

    // ---- routing by group: the two equal frames make the one group of 2 x 240 x 180 pixels
    AtlasRoute r = atlas_route(sizes, 2ull * 240 * 180, false);
    CHECK(r.own.size() == 1 && r.own[0].size() == 2 && r.own[0][0] == 0 && r.own[0][1] == 8 && r.packed.size() == sizes.size() - 2);
    for (size_t i = 1; i < r.packed.size(); ++i) CHECK(r.packed[i - 1] < r.packed[i]);
    r = atlas_route(sizes, 1, false);                                          // everything per group
    CHECK(r.packed.empty() && r.own.size() == sizes.size() - 1);
    r = atlas_route(sizes, UINT64_MAX, false);                                 // never
    CHECK(r.own.empty() && r.packed.size() == sizes.size());
    r = atlas_route(sizes, UINT64_MAX, true);                                  // a flag that needs the image alone
    CHECK(r.packed.empty() && r.own.size() == sizes.size() - 1);
    size_t n = 0;
    for (const auto& g : r.own) {
        for (int i : g) CHECK(sizes[(size_t)i].w == sizes[(size_t)g[0]].w && sizes[(size_t)i].h == sizes[(size_t)g[0]].h && sizes[(size_t)i].ch == sizes[(size_t)g[0]].ch);
        n += g.size();
    }
    CHECK(n == sizes.size());
    // the packed part of a route, planned
    r = atlas_route(sizes, 2ull * 240 * 180, false);
    t = plan_all(sizes, r.packed, ATLAS_DEFAULT_PX, 0);
    CHECK(t.atlases == 1 && t.frames == r.packed.size());

    // ---- the frame checks: the first bad frame is named
    static const uint8_t px[64] = {0};
    std::vector<vj_image> im = {{px, 4, 4, 4, 0, 1}, {px, 5, 3, 15, 0, 3}, {px, 2, 2, 8, 0, 4}, {px, 3, 3, 3, 0, 0}};
    std::vector<AtlasSize> got;
    CHECK(atlas_check_frames(im.data(), (int)im.size(), &got) == VJ_OK && got.size() == 4 && got[1].ch == 3 && got[3].ch == 1);
    CHECK(atlas_check_frames(nullptr, 0, &got) == VJ_OK && got.empty());
    CHECK(atlas_check_frames(nullptr, 1, &got) == VJ_ERR_ARG);
    const vj_image bad[] = {{nullptr, 4, 4, 4, 0, 1}, {px, 0, 4, 4, 0, 1}, {px, 4, -1, 4, 0, 1}, {px, 4, 4, 3, 0, 1}, {px, 4, 4, 11, 0, 3}, {px, 4, 4, 8, 0, 2}};
    for (const vj_image& b : bad) {
        std::vector<vj_image> v = {im[0], im[1], b};
        CHECK(atlas_check_frames(v.data(), 3, &got) == VJ_ERR_ARG);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr);
    }
    printf("atlas_asan_driver: OK\n");
    return 0;
}
