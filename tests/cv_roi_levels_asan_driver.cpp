// Sanitizer driver of the host planner of CV_HAAR_SCALE_IMAGE inside regions (csrc/vj_cv_roi_levels_host.cpp): built by
// tests/test_sanitizers_cv_roi_levels.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/cv_roi_levels_asan_driver.cpp csrc/vj_cv_roi_levels_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  The REGIONS geometry of tests/cv_rois_cases.py in three frames, planned with the library's canvas budget and
// with one so small that the canvases split and one region fits none: every level image inside its canvas, no two overlapping, row
// units covering every grid row once, taps inside the crop, the oversized region reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_cv_roi_levels_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static const int FRAME_W = 240, FRAME_H = 180, N_FRAMES = 3;
static const int REGIONS[][4] = {
    {0, 0, FRAME_W, FRAME_H}, {0, 0, 131, 97}, {FRAME_W - 141, 0, 141, 111}, {0, FRAME_H - 103, 127, 103},
    {FRAME_W - 150, FRAME_H - 120, 150, 120}, {37, 21, 155, 133}, {51, 33, 101, 99}, {13, 7, 211, 61}, {101, 5, 67, 171},
    {5, 3, 29, 29}, {199, 150, 31, 22}, {63, 41, 88, 88}, {17, 59, 120, 110},
};

struct Totals { size_t canvases = 0, levels = 0, regions = 0; uint64_t windows = 0; std::vector<int> oversized; };

// every canvas of the list, checked; the level loop restated for the expected counts
static Totals plan_all(const std::vector<CvRoiHost>& regs, int win_w, int win_h, double sf, int min_w, int min_h, uint64_t budget) {
    Totals t;
    CvTapCache taps;
    CvRegionCanvas cv;
    for (size_t pos = 0; pos < regs.size();) {
        CHECK(cv_roi_plan_canvas(regs, pos, win_w, win_h, sf, min_w, min_h, budget, &taps, &cv) == VJ_OK);
        CHECK(cv.n_regions >= 1 && pos + cv.n_regions <= regs.size());
        if (cv.oversized) {
            CHECK(cv.n_regions == 1 && cv.levels.empty() && cv.dev.empty());
            t.oversized.push_back(regs[pos].id);
            pos += 1;
            continue;
        }
        CHECK(cv.dev.size() == cv.levels.size());
        CHECK((uint64_t)cv.w * cv.h <= budget && cv.pitch >= cv.w && cv.pitch % 4u == 0u);
        CHECK(cv.h < 65535u && (uint64_t)(cv.w + 1u) * (cv.h + 3ull) < (1ull << 30));
        std::vector<uint8_t> covered((size_t)cv.pitch * cv.h, 0);
        std::vector<uint8_t> row_seen(cv.n_rows, 0);
        uint64_t windows = 0, unit = 0;
        size_t expect_levels = 0;
        std::vector<CvLevelHost> own;
        for (size_t r = pos; r < pos + cv.n_regions; ++r) {
            int n_empty = 0;
            CHECK(cv_scale_image_levels(win_w, win_h, regs[r].w, regs[r].h, sf, min_w, min_h, regs[r].w, regs[r].h, &own, &n_empty) == VJ_OK);
            expect_levels += own.size();
        }
        CHECK(expect_levels == cv.levels.size());
        for (size_t k = 0; k < cv.levels.size(); ++k) {
            const CvRegionLevel& L = cv.levels[k];
            const PyrRegionLevelDev& d = cv.dev[k];
            CHECK(L.region >= (int)pos && L.region < (int)(pos + cv.n_regions));
            const CvRoiHost& g = regs[(size_t)L.region];
            CHECK(d.frame == (uint32_t)g.frame && d.cx == (uint32_t)g.x && d.cy == (uint32_t)g.y && d.cw == (uint32_t)g.w && d.ch == (uint32_t)g.h);
            CHECK(d.cx + d.cw <= (uint32_t)FRAME_W && d.cy + d.ch <= (uint32_t)FRAME_H);
            CHECK(d.w == (uint32_t)L.lv.lw && d.h == (uint32_t)L.lv.lh && d.w >= (uint32_t)win_w && d.h >= (uint32_t)win_h);
            // inside the canvas, at a dword-aligned column, overlapping nothing
            CHECK(d.ox % 4u == 0u && d.ox + d.w <= cv.w && d.oy + d.h <= cv.h);
            for (uint32_t y = 0; y < d.h; ++y)
                for (uint32_t x = 0; x < d.w; ++x) {
                    uint8_t& c = covered[(size_t)(d.oy + y) * cv.pitch + d.ox + x];
                    CHECK(c == 0);
                    c = 1;
                }
            // the taps index the crop
            CHECK((size_t)d.xtab + d.w <= taps.taps.size() && (size_t)d.ytab + d.h <= taps.taps.size());
            for (uint32_t x = 0; x < d.w; ++x) CHECK(taps.taps[d.xtab + x].i0 < d.cw && taps.taps[d.xtab + x].i1 < d.cw);
            for (uint32_t y = 0; y < d.h; ++y) CHECK(taps.taps[d.ytab + y].i0 < d.ch && taps.taps[d.ytab + y].i1 < d.ch);
            CHECK((d.area != 0u) == (d.cw == 2u * d.w && d.ch == 2u * d.h));
            // work units of the pyramid kernel: a prefix
            CHECK(d.unit_first == unit);
            unit += (uint64_t)((d.w + PYR_REGION_TW - 1u) / PYR_REGION_TW) * ((d.h + PYR_REGION_TH - 1u) / PYR_REGION_TH);
            // the grid: x, y = 0, step, ... < size - window; its rows are units [row_first, + end_y), each once
            CHECK(L.lv.step == (L.lv.factor > 2 ? 1 : 2));
            int nx = 0, ny = 0;
            for (int x = 0; x < L.lv.lw - win_w; x += L.lv.step) ++nx;
            for (int y = 0; y < L.lv.lh - win_h; y += L.lv.step) ++ny;
            CHECK(nx == L.lv.end_x && ny == L.lv.end_y && nx > 0 && ny > 0);
            CHECK((L.lv.end_x - 1) * L.lv.step + win_w <= L.lv.lw && (L.lv.end_y - 1) * L.lv.step + win_h <= L.lv.lh);
            CHECK((uint64_t)L.row_first + (uint64_t)L.lv.end_y <= cv.n_rows);
            for (int iy = 0; iy < L.lv.end_y; ++iy) {
                CHECK(row_seen[L.row_first + (uint32_t)iy] == 0);
                row_seen[L.row_first + (uint32_t)iy] = 1;
            }
            CHECK(L.lv.win_w >= min_w && L.lv.win_h >= min_h && L.lv.win_w <= g.w && L.lv.win_h <= g.h);
            windows += (uint64_t)nx * ny;
        }
        for (uint8_t s : row_seen) CHECK(s == 1);
        CHECK(unit == cv.n_pyr_units && windows == cv.windows);
        t.canvases += cv.levels.empty() ? 0 : 1;
        t.levels += cv.levels.size();
        t.windows += cv.windows;
        t.regions += cv.n_regions;
        pos += cv.n_regions;
    }
    return t;
}

int main() {
    std::vector<CvRoiHost> regs;
    for (int f = 0; f < N_FRAMES; ++f)
        for (const auto& r : REGIONS) regs.push_back(CvRoiHost{f, r[0], r[1], r[2], r[3], (int)regs.size()});
    // the library's budget: one canvas holds everything
    const Totals whole = plan_all(regs, 20, 20, 1.1, 0, 0, 1ull << 24);
    CHECK(whole.canvases == 1 && whole.oversized.empty() && whole.levels >= 300 && whole.regions == regs.size());
    // a budget that holds a few regions: the canvases split, the whole frame (ids 0, 13, 26) fits none
    const Totals split = plan_all(regs, 20, 20, 1.1, 0, 0, 150000);
    CHECK(split.canvases >= 2 && split.oversized.size() == 3 && split.oversized[0] == 0 && split.oversized[1] == 13 && split.oversized[2] == 26);
    CHECK(split.regions == regs.size() - 3);
    // what the canvases hold does not depend on how they split
    const Totals rest = plan_all(std::vector<CvRoiHost>(regs.begin() + 1, regs.begin() + 13), 20, 20, 1.1, 0, 0, 1ull << 24);
    CHECK(split.levels == whole.levels - 3 * (whole.levels / 3 - rest.levels) && split.windows == whole.windows - 3 * (whole.windows / 3 - rest.windows));
    // scale factor 2: levels at exactly half their crop take the 2 x 2 mean's taps
    const Totals half = plan_all(regs, 20, 20, 2.0, 0, 0, 1ull << 24);
    CHECK(half.levels >= 12 && half.canvases == 1);
    // a minimum size, another window, a budget nothing fits
    const Totals mins = plan_all(regs, 24, 20, 1.25, 30, 30, 1ull << 24);
    CHECK(mins.levels >= 10 && mins.levels < whole.levels);
    const Totals none = plan_all(regs, 20, 20, 1.1, 0, 0, 16);
    CHECK(none.canvases == 0 && none.levels == 0 && none.oversized.size() == regs.size());
    // regions smaller than the window have no level: they are taken and leave nothing, whatever the budget
    const std::vector<CvRoiHost> tiny = {CvRoiHost{0, 3, 3, 19, 40, 0}, CvRoiHost{1, 200, 150, 40, 18, 1}};
    const Totals t0 = plan_all(tiny, 20, 20, 1.1, 0, 0, 16), t1 = plan_all(tiny, 20, 20, 1.1, 0, 0, 1ull << 24);
    CHECK(t0.levels == 0 && t0.oversized.empty() && t0.regions == 2 && t1.levels == 0 && t1.oversized.empty() && t1.regions == 2);
    // regions that are no image rectangles are refused
    CvTapCache taps;
    CvRegionCanvas cv;
    CHECK(cv_roi_plan_canvas({CvRoiHost{0, 0, 0, 0, 50, 0}}, 0, 20, 20, 1.1, 0, 0, 1ull << 24, &taps, &cv) == VJ_ERR_ARG);
    CHECK(cv_roi_plan_canvas({CvRoiHost{0, -1, 0, 50, 50, 0}}, 0, 20, 20, 1.1, 0, 0, 1ull << 24, &taps, &cv) == VJ_ERR_ARG);
    CHECK(cv_roi_plan_canvas(regs, regs.size(), 20, 20, 1.1, 0, 0, 1ull << 24, &taps, &cv) == VJ_OK && cv.n_regions == 0);
    // the routing rule: at most CV_ROI_LEVELS_MAX_REGIONS_PER_SIZE regions per distinct size on average
    {
        std::vector<vj_roi> rr;
        for (const CvRoiHost& g : regs) rr.push_back(vj_roi{g.frame, g.x, g.y, g.w, g.h});
        CHECK(cv_rois_levels_pay(rr.data(), (int)rr.size()) && cv_rois_levels_pay(rr.data(), 0));      // 39 regions of 13 sizes
        std::vector<vj_roi> same((size_t)CV_ROI_LEVELS_MAX_REGIONS_PER_SIZE, vj_roi{0, 0, 0, 50, 60});
        CHECK(cv_rois_levels_pay(same.data(), (int)same.size()));
        same.push_back(vj_roi{1, 3, 3, 50, 60});
        CHECK(!cv_rois_levels_pay(same.data(), (int)same.size()));
        same.push_back(vj_roi{1, 3, 3, 60, 50});                                                          // a second size
        CHECK(cv_rois_levels_pay(same.data(), (int)same.size()));
    }
    // a scale factor that gives more than 65536 levels
    std::vector<CvLevelHost> lv;
    CHECK(cv_scale_image_levels(20, 20, 240, 180, 1.0 + 1e-9, 0, 0, 240, 180, &lv) == VJ_ERR_LIMIT);
    printf("cv_roi_levels_asan_driver: OK (%zu level images, %zu + %zu canvases)\n", whole.levels, whole.canvases, split.canvases);
    return 0;
}
