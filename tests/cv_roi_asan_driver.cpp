// Sanitizer driver of the host side of vj_detect_opencv_rois / vj_detect_opencv_chain (csrc/vj_cv_roi_host.cpp): built by
// tests/test_sanitizers_cv_rois.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/cv_roi_asan_driver.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Degenerate region lists — edge-touching, too small, unsorted, outside, huge scale counts — must come back
// as empty lists or error codes; every memory error or undefined behaviour aborts the process.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_cv_roi_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint32_t rng_state = 7;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static const int WIN = 20;

static std::vector<CvRoiFactor> factors_for(int n, double sf, uint64_t reach) {
    std::vector<CvRoiFactor> f;
    double factor = 1;
    for (int k = 0; k < n; ++k, factor *= sf) {
        f.push_back(cv_roi_factor(WIN, WIN, factor));
        f.back().max_reach = reach;
    }
    return f;
}

// the unit list of a region list: every unit names a region, a factor and a row inside the region's own grid
static int units_of(const std::vector<CvRoiHost>& regs, double sf, int W, int H, int min_w, size_t* n_units, uint64_t* windows, int slack = 0) {
    int n_factors = 0;
    for (const CvRoiHost& r : regs) {
        const int n = cv_count_factors(WIN, WIN, r.w, r.h, sf, 4096);
        if (n > 4096) return VJ_ERR_LIMIT;
        n_factors = n > n_factors ? n : n_factors;
    }
    const std::vector<CvRoiFactor> factors = factors_for(n_factors + slack, sf, 0);
    std::vector<CvRoiDev> rois;
    std::vector<CvRoiUnit> units;
    const uint32_t stride = (uint32_t)W + 1u, frame_elems = stride * ((uint32_t)H + 3u);
    const int rc = cv_roi_build_units(regs, WIN, WIN, sf, factors, stride, frame_elems, min_w, min_w, &rois, &units, windows);
    if (rc) return rc;
    CHECK(rois.size() == regs.size());
    uint64_t sum = 0;
    for (const CvRoiUnit& u : units) {
        CHECK(u.roi < regs.size() && u.slot < factors.size());
        const CvRoiHost& r = regs[u.roi];
        const CvRoiFactor& f = factors[u.slot];
        CHECK(f.win_w >= min_w && u.end_x > 0);
        CHECK(u.end_x == (uint32_t)cv_round((r.w - f.win_w) / f.ystep) && u.iy < (uint32_t)cv_round((r.h - f.win_h) / f.ystep));
        // a window the border rule lets through lies inside the region, the region inside the frame
        CHECK(r.x >= 0 && r.y >= 0 && r.x + r.w <= W && r.y + r.h <= H);
        sum += u.end_x;
    }
    CHECK(sum == *windows);
    *n_units = units.size();
    return VJ_OK;
}

static void test_factors() {
    CHECK(cv_count_factors(WIN, WIN, 30, 30, 1.1, 100) == 0);              // 20 < 20 is false: too small for any scale
    CHECK(cv_count_factors(WIN, WIN, 31, 31, 1.1, 100) == 1);
    CHECK(cv_count_factors(WIN, WIN, 31, 1000, 1.1, 100) == 1);
    CHECK(cv_count_factors(WIN, WIN, 0, 0, 1.1, 100) == 0);
    CHECK(cv_count_factors(WIN, WIN, INT_MIN, INT_MAX, 1.1, 100) == 0);
    CHECK(cv_count_factors(WIN, WIN, INT_MAX, INT_MAX, 1.1, 1000) > 100);
    // huge scale counts: a factor step just above 1 stops at the cap
    CHECK(cv_count_factors(WIN, WIN, 65000, 65000, 1.0 + 1e-12, 1000) == 1001);
    CHECK(cv_count_factors(WIN, WIN, 65000, 65000, 1.0000001, 1 << 20) == (1 << 20) + 1);
    CHECK(cv_count_factors(WIN, WIN, 200, 200, 1e300, 100) == 1);
    const CvRoiFactor f = cv_roi_factor(WIN, WIN, 1.0);
    CHECK(f.ystep == 2. && f.win_w == WIN && f.win_h == WIN);
    CHECK(cv_roi_factor(WIN, WIN, 2.5).ystep == 2.5 && cv_roi_factor(WIN, WIN, 2.5).win_w == 50);
}

static void test_arguments() {
    std::vector<uint8_t> px(64 * 48 * 3, 0);
    vj_image frames[3] = {{px.data(), 64, 48, 64, 0, 1}, {px.data(), 64, 48, 64 * 3, 0, 3}, {nullptr, 64, 48, 64, 0, 1}};
    const vj_roi ok[] = {{0, 0, 0, 64, 48}, {0, 63, 47, 1, 1}, {1, 1, 1, 63, 47}, {0, 0, 47, 64, 1}};
    for (const vj_roi& r : ok) CHECK(cv_roi_inside(r, frames, 3));
    const vj_roi bad[] = {{0, 0, 0, 65, 48}, {0, 1, 0, 64, 48}, {0, -1, 0, 10, 10}, {0, 0, 0, 0, 10}, {0, 0, 0, 10, -3}, {3, 0, 0, 10, 10},
                          {-1, 0, 0, 10, 10}, {2, 0, 0, 10, 10}, {0, INT_MAX, 0, 10, 10}, {0, 0, 0, INT_MAX, INT_MAX},
                          {0, INT_MAX, INT_MAX, INT_MAX, INT_MAX}, {0, INT_MIN, INT_MIN, 1, 1}, {0, 0, 0, INT_MIN, 1}};
    for (const vj_roi& r : bad) CHECK(!cv_roi_inside(r, frames, 3));
    int W, H, CH;
    CHECK(cv_frames_uniform(frames, 1, &W, &H, &CH) && W == 64 && H == 48 && CH == 1);
    CHECK(!cv_frames_uniform(frames, 2, &W, &H, &CH));     // channel counts differ
    CHECK(!cv_frames_uniform(frames, 0, &W, &H, &CH));
    vj_image odd[2] = {{px.data(), 64, 48, 64, 0, 1}, {px.data(), 32, 48, 64, 0, 1}};
    CHECK(!cv_frames_uniform(odd, 2, &W, &H, &CH));        // sizes differ
    vj_image thin = {px.data(), 64, 48, 63, 0, 1};
    CHECK(!cv_frames_uniform(&thin, 1, &W, &H, &CH));      // stride below the width
    vj_image big = {px.data(), 65535, 65535, 65535, 0, 1};
    CHECK(!cv_frames_uniform(&big, 1, &W, &H, &CH));
    vj_image two = {px.data(), 64, 48, 128, 0, 2};
    CHECK(!cv_frames_uniform(&two, 1, &W, &H, &CH));
}

static void test_units() {
    const int W = 200, H = 150;
    size_t n = 0;
    uint64_t windows = 0;
    // edge-touching, overlapping, the whole frame, too small (a side of at most win + 10), one pixel
    std::vector<CvRoiHost> regs = {{0, 0, 0, W, H, 0}, {0, W - 40, H - 40, 40, 40, 1}, {1, 0, H - 31, 31, 31, 2}, {0, 3, 5, 30, 120, 3},
                                   {2, 7, 9, 1, 1, 4}, {0, 0, 0, W, 31, 5}, {1, W - 31, 0, 31, H, 6}, {0, 10, 10, 100, 100, 7}};
    CHECK(units_of(regs, 1.1, W, H, 0, &n, &windows) == VJ_OK && n > 0 && windows > 0);
    const size_t n_all = n;
    CHECK(units_of(regs, 1.1, W, H, 40, &n, &windows) == VJ_OK && n < n_all);   // min_size drops the small factors
    CHECK(units_of(regs, 1.1, W, H, 0, &n, &windows, 5) == VJ_OK && n == n_all);   // a longer table than the regions need
    CHECK(units_of(regs, 1.1, W, H, 100000, &n, &windows) == VJ_OK && n == 0 && windows == 0);
    std::vector<CvRoiHost> small = {{0, 0, 0, 30, 30, 0}, {0, 5, 5, 1, 1, 1}, {0, 0, 0, 30, H, 2}};
    CHECK(units_of(small, 1.1, W, H, 0, &n, &windows) == VJ_OK && n == 0 && windows == 0);
    CHECK(units_of(std::vector<CvRoiHost>(), 1.1, W, H, 0, &n, &windows) == VJ_OK && n == 0);
    // a factor step that gives thousands of scales in a small region, and one past the cap
    CHECK(units_of({{0, 0, 0, 60, 60, 0}}, 1.0005, W, H, 0, &n, &windows) == VJ_OK && n > 1000);
    CHECK(units_of({{0, 0, 0, 60, 60, 0}}, 1.0 + 1e-9, W, H, 0, &n, &windows) == VJ_ERR_LIMIT);
    // a table shorter than a region's factors, a region that is no rectangle, a feature that reaches past the frame's allocation
    std::vector<CvRoiDev> rois;
    std::vector<CvRoiUnit> units;
    const uint32_t stride = W + 1, frame_elems = stride * (H + 3);
    CHECK(cv_roi_build_units(regs, WIN, WIN, 1.1, factors_for(2, 1.1, 0), stride, frame_elems, 0, 0, &rois, &units, &windows) == VJ_ERR_LIMIT);
    CHECK(cv_roi_build_units({{0, -1, 0, 50, 50, 0}}, WIN, WIN, 1.1, factors_for(30, 1.1, 0), stride, frame_elems, 0, 0, &rois, &units, &windows) == VJ_ERR_ARG);
    CHECK(cv_roi_build_units({{0, 0, 0, 50, 0, 0}}, WIN, WIN, 1.1, factors_for(30, 1.1, 0), stride, frame_elems, 0, 0, &rois, &units, &windows) == VJ_ERR_ARG);
    CHECK(cv_roi_build_units(regs, WIN, WIN, 1.1, factors_for(30, 1.1, (uint64_t)stride * 30), stride, frame_elems, 0, 0, &rois, &units, &windows) == VJ_ERR_LIMIT);
    CHECK(cv_roi_build_units({{0, INT_MAX - 50, INT_MAX - 50, 50, 50, 0}}, WIN, WIN, 1.1, factors_for(30, 1.1, 0), stride, frame_elems, 0, 0, &rois, &units, &windows) == VJ_ERR_LIMIT);
    // random regions inside the frame
    for (int round = 0; round < 50; ++round) {
        std::vector<CvRoiHost> rr;
        for (int i = 0, m = (int)(rnd() % 12); i < m; ++i) {
            const int w = 1 + (int)(rnd() % W), h = 1 + (int)(rnd() % H);
            rr.push_back(CvRoiHost{(int)(rnd() % 4), (int)(rnd() % (uint32_t)(W - w + 1)), (int)(rnd() % (uint32_t)(H - h + 1)), w, h, i});
        }
        CHECK(units_of(rr, 1.05 + (rnd() % 100) / 100., W, H, (int)(rnd() % 60), &n, &windows) == VJ_OK);
    }
}

static void test_rects_and_results() {
    const std::vector<CvRoiFactor> factors = factors_for(4, 1.2, 0);
    const std::vector<CvRoiHost> regs = {{0, 0, 0, 80, 80, 5}, {1, 3, 3, 90, 70, 2}};
    const CvDet raw[] = {{4, 6, 1, 1}, {0, 0, 0, 0}, {2, 2, 3, 1}, {2, 2, 3, 0}};
    std::vector<vj_rect> all;
    CHECK(cv_roi_rects_of(raw, 4, factors, regs, &all) == VJ_OK && all.size() == 4);
    CHECK(all[0].frame == 2 && all[0].scale_idx == 1 && all[0].w == factors[1].win_w && all[1].frame == 5);
    const CvDet off_slot = {0, 0, 4, 0}, off_roi = {0, 0, 0, 2}, wild = {0, 0, 0xffffffffu, 0xffffffffu};
    CHECK(cv_roi_rects_of(&off_slot, 1, factors, regs, &all) != VJ_OK);
    CHECK(cv_roi_rects_of(&off_roi, 1, factors, regs, &all) != VJ_OK);
    CHECK(cv_roi_rects_of(&wild, 1, factors, regs, &all) != VJ_OK);
    CHECK(cv_roi_rects_of(nullptr, 0, factors, regs, &all) == VJ_OK && all.size() == 4);

    StageProgram prog;
    prog.n_nodes = {3, 9};
    prog.n_rects = {6, 20};
    vj_cv_params p;
    memset(&p, 0, sizeof(p));
    p.scale_factor = 1.2;
    p.flags = VJ_FLAG_COUNTERS;
    vj_result out;
    memset(&out, 0, sizeof(out));
    out.counters.stage_entered[0] = 10;
    out.counters.stage_entered[1] = 4;
    CHECK(finish_cv_roi_result(all, &prog, &p, &out) == VJ_OK && out.count == 4);
    for (uint32_t i = 1; i < out.count; ++i) CHECK(out.rects[i - 1].frame <= out.rects[i].frame);   // unsorted in, sorted out
    CHECK(out.counters.stump_evals == 10 * 3 + 4 * 9 && out.counters.gather_bytes == 48 * 10 + 16 * (10 * 6 + 4 * 20));
    free(out.rects);   // (vj_result_free lives with the device code)
    // grouped per region; no pass ran (no program); nothing at all
    std::vector<vj_rect> many;
    for (int i = 0; i < 40; ++i) many.push_back(vj_rect{10 + i % 3, 12 + i % 2, 24, 24, 0.f, i % 2 ? 7 : 0, 1});
    p.min_neighbors = 3;
    memset(&out, 0, sizeof(out));
    CHECK(finish_cv_roi_result(many, nullptr, &p, &out) == VJ_OK && out.count == 2 && out.rects[0].frame == 0 && out.rects[1].frame == 7);
    free(out.rects);   // (vj_result_free lives with the device code)
    std::vector<vj_rect> none;
    memset(&out, 0, sizeof(out));
    CHECK(finish_cv_roi_result(none, &prog, &p, &out) == VJ_OK && out.count == 0 && out.rects == nullptr);
}

static void test_fallback_grouping() {
    std::vector<uint8_t> gray(100 * 80, 0), bgr(100 * 80 * 3, 0);
    const vj_image frames[2] = {{gray.data(), 100, 80, 100, 0, 0}, {bgr.data(), 100, 80, 300, 0, 3}};
    // unsorted, repeated sizes, the same size on frames of different channel counts, edge-touching
    const vj_roi rois[] = {{1, 60, 40, 40, 40}, {0, 0, 0, 40, 40}, {0, 60, 40, 40, 40}, {1, 0, 0, 100, 80}, {0, 0, 0, 100, 80}, {0, 99, 79, 1, 1},
                           {1, 10, 10, 40, 40}};
    const int n_rois = (int)(sizeof(rois) / sizeof(rois[0]));
    const std::vector<CvRoiSizeGroup> groups = cv_roi_size_groups(frames, rois, n_rois);
    CHECK(groups.size() == 5);
    std::vector<int> seen((size_t)n_rois, 0);
    std::vector<vj_rect> all;
    vj_result out;
    memset(&out, 0, sizeof(out));
    for (const CvRoiSizeGroup& g : groups) {
        CHECK(g.idx.size() == g.views.size() && !g.idx.empty());
        std::vector<vj_rect> rects;
        for (size_t k = 0; k < g.idx.size(); ++k) {
            const vj_roi& r = rois[g.idx[k]];
            const vj_image& f = frames[r.frame];
            const vj_image& v = g.views[k];
            seen[(size_t)g.idx[k]]++;
            CHECK(v.width == r.w && v.height == r.h && v.stride == f.stride && v.channels == f.channels);
            CHECK(v.width == g.views[0].width && v.height == g.views[0].height && v.channels == g.views[0].channels);
            // the view's last byte lies inside the frame's pixels
            const int ch = f.channels <= 1 ? 1 : f.channels;
            const uint8_t* last = v.data + (size_t)(v.height - 1) * (size_t)v.stride + (size_t)v.width * (size_t)ch - 1;
            CHECK(v.data >= f.data && last < f.data + (size_t)f.height * (size_t)f.stride);
            CHECK(*last == 0);
            rects.push_back(vj_rect{1, 2, 20, 20, 0.f, (int32_t)k, 0});
        }
        vj_result part;
        memset(&part, 0, sizeof(part));
        part.rects = rects.data();
        part.count = (uint32_t)rects.size();
        part.counters.windows = 5;
        part.timing.n_cascade_launches = 1;
        CHECK(cv_roi_take_part(part, g.idx, &all, &out) == VJ_OK);
        // a result that names a frame the group does not have
        vj_rect stray = {0, 0, 20, 20, 0.f, (int32_t)g.idx.size(), 0};
        part.rects = &stray;
        part.count = 1;
        std::vector<vj_rect> sink;
        vj_result scratch;
        memset(&scratch, 0, sizeof(scratch));
        CHECK(cv_roi_take_part(part, g.idx, &sink, &scratch) == VJ_ERR_ARG);
        stray.frame = -1;
        CHECK(cv_roi_take_part(part, g.idx, &sink, &scratch) == VJ_ERR_ARG);
    }
    for (int s : seen) CHECK(s == 1);
    CHECK(out.counters.windows == 5 * groups.size() && out.timing.n_cascade_launches == groups.size());
    CHECK(cv_roi_emit_parts(all, &out) == VJ_OK && out.count == (uint32_t)n_rois);
    for (uint32_t i = 0; i < out.count; ++i) CHECK(out.rects[i].frame == (int32_t)i);
    free(out.rects);   // (vj_result_free lives with the device code)
    CHECK(cv_roi_size_groups(frames, rois, 0).empty());

    // regions by frame, sub-batch by sub-batch: every region once, relative to its sub-batch
    const std::vector<int> by_frame = cv_rois_by_frame(rois, n_rois);
    CHECK(by_frame.size() == (size_t)n_rois && cv_rois_by_frame(rois, 0).empty());
    for (size_t i = 1; i < by_frame.size(); ++i) CHECK(rois[by_frame[i - 1]].frame <= rois[by_frame[i]].frame);
    size_t next = 0, total = 0;
    std::vector<CvRoiHost> regs;
    for (int f0 = 0; f0 < 2; ++f0) {
        cv_rois_of_subbatch(rois, by_frame, &next, f0, 1, &regs);
        for (const CvRoiHost& r : regs) CHECK(r.frame == 0 && rois[r.id].frame == f0 && r.w == rois[r.id].w);
        total += regs.size();
    }
    CHECK(total == (size_t)n_rois && next == by_frame.size());
    cv_rois_of_subbatch(rois, by_frame, &next, 2, 5, &regs);
    CHECK(regs.empty());
}

static void test_chain_regions() {
    const int W = 120, H = 90;
    std::vector<vj_rect> raw;
    for (int i = 0; i < 30; ++i) raw.push_back(vj_rect{40 - i % 3, 30 + i % 2, 24, 24, 0.f, 2 + i % 2, i % 4});   // unsorted, two frames
    std::vector<CvRoiHost> regs;
    std::vector<vj_rect> regions;
    CHECK(cv_chain_regions(raw.data(), raw.size(), 0, W, H, 2, 2, &regs, &regions) == VJ_OK && regs.size() == 30 && regions.size() == 30);
    for (size_t i = 0; i < regs.size(); ++i) CHECK(regs[i].id == (int)i && regs[i].frame == regions[i].frame - 2 && regs[i].frame >= 0 && regs[i].frame < 2);
    vj_result first;
    memset(&first, 0, sizeof(first));
    first.rects = regions.data();
    first.count = (uint32_t)regions.size();
    CHECK(cv_chain_regions_match(regions, first));
    first.count -= 1;
    CHECK(!cv_chain_regions_match(regions, first));
    std::vector<vj_rect> moved = regions;
    moved[7].x += 1;
    first.rects = moved.data();
    first.count = (uint32_t)moved.size();
    CHECK(!cv_chain_regions_match(regions, first));
    // grouped: ids go on from the regions already there
    CHECK(cv_chain_regions(raw.data(), raw.size(), 3, W, H, 2, 2, &regs, &regions) == VJ_OK && regs.size() == 2 && regions.size() == 32);
    CHECK(regs[0].id == 30 && regs[1].id == 31);
    CHECK(cv_chain_regions(nullptr, 0, 3, W, H, 0, 1, &regs, &regions) == VJ_OK && regs.empty() && regions.size() == 32);
    // a candidate of another sub-batch, or outside the frame
    CHECK(cv_chain_regions(raw.data(), raw.size(), 0, W, H, 0, 2, &regs, &regions) == VJ_ERR_ARG);
    const vj_rect outside[] = {{W - 10, 0, 24, 24, 0.f, 0, 0}, {0, 0, 0, 24, 0.f, 0, 0}, {-1, 0, 24, 24, 0.f, 0, 0}, {0, 0, INT_MAX, INT_MAX, 0.f, 0, 0},
                               {INT_MAX, INT_MAX, 24, 24, 0.f, 0, 0}, {0, 0, 24, 24, 0.f, INT_MIN, 0}};
    for (const vj_rect& r : outside) CHECK(cv_chain_regions(&r, 1, 0, W, H, 0, 1, &regs, &regions) == VJ_ERR_ARG);
    const vj_rect edge = {W - 24, H - 24, 24, 24, 0.f, 0, 0};
    CHECK(cv_chain_regions(&edge, 1, 0, W, H, 0, 1, &regs, &regions) == VJ_OK && regs.size() == 1);
}

int main() {
    test_factors();
    test_arguments();
    test_units();
    test_rects_and_results();
    test_fallback_grouping();
    test_chain_regions();
    printf("cv_roi_asan_driver: OK\n");
    return 0;
}
