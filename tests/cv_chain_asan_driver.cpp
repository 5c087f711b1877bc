// Sanitizer driver of the device-free host code of vj_detect_opencv_chain's device hand-off (csrc/vj_cv_roi_host.cpp: the route a call
// takes, the rank of a sub-batch's candidates, the region -> out_first index remap, the grouped regions, the second cascade's
// rectangles, the info record, the state block's errors) and of the unit builder's restatement shared with the device
// (csrc/vj_cv_roi_units.hpp), built by tests/test_sanitizers_cv_chain.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/cv_chain_asan_driver.cpp csrc/vj_cv_roi_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  Every memory error or undefined behaviour aborts the process.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>
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

static uint32_t rng_state = 11;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static void route() {
    const uint32_t D = VJ_FLAG_CV_CHAIN_DEVICE, C = VJ_FLAG_COUNTERS;
    CvChainRoute r = cv_chain_route(0, 0);
    CHECK(r.handoff == 2 && r.flags_first == 0 && r.flags_second == 0);
    r = cv_chain_route(D, 0);
    CHECK(r.handoff == 1 && r.flags_first == 0 && r.flags_second == 0);
    r = cv_chain_route(D | C, C);
    CHECK(r.handoff == 1 && r.flags_first == C && r.flags_second == C);
    r = cv_chain_route(C, D);                                     // only the first word is read for the bit; it is stripped from both
    CHECK(r.handoff == 2 && r.flags_first == C && r.flags_second == 0);
    for (uint32_t other : {(uint32_t)VJ_FLAG_CV_CANNY_PRUNING, (uint32_t)VJ_FLAG_CV_SCALE_IMAGE, (uint32_t)VJ_FLAG_CV_FIND_BIGGEST, 1u << 20}) {
        r = cv_chain_route(D | other, 0);
        CHECK(r.handoff == 3 && r.flags_first == other);
        r = cv_chain_route(D, other);
        CHECK(r.handoff == 3 && r.flags_second == other && r.flags_first == 0);
        r = cv_chain_route(other, D | other);
        CHECK(r.handoff == 3 && r.flags_second == other);
    }
}

// candidates as the first cascade reports them: in no order
static std::vector<vj_rect> candidates(size_t n, int f0, int nf, bool duplicates) {
    std::vector<vj_rect> raw;
    for (size_t i = 0; i < n; ++i) {
        const int k = (int)(rnd() % 5u);
        vj_rect r{(int32_t)(rnd() % 300u), (int32_t)(rnd() % 200u), 20 + 4 * k, 20 + 4 * k, 0.0f, f0 + (int32_t)(rnd() % (uint32_t)nf), k};
        if (duplicates && i != 0 && rnd() % 3u == 0u) r = raw[rnd() % raw.size()];
        raw.push_back(r);
    }
    return raw;
}

static void rank_and_remap(bool duplicates) {
    CHECK(cv_chain_rank(nullptr, 0).empty());
    const int f0 = 3, nf = 4;
    const std::vector<vj_rect> raw = candidates(257, f0, nf, duplicates);
    const std::vector<uint32_t> rank = cv_chain_rank(raw.data(), raw.size());
    CHECK(rank.size() == raw.size());
    std::vector<vj_rect> sorted = raw;
    std::sort(sorted.begin(), sorted.end(), [](const vj_rect& a, const vj_rect& b) {
        return std::tie(a.frame, a.scale_idx, a.y, a.x) < std::tie(b.frame, b.scale_idx, b.y, b.x);
    });
    std::vector<bool> used(raw.size(), false);
    for (size_t i = 0; i < raw.size(); ++i) {   // a permutation, and the rectangle at its rank in the sorted list is the candidate's
        CHECK(rank[i] < raw.size() && !used[rank[i]]);
        used[rank[i]] = true;
        const vj_rect &a = sorted[rank[i]], &b = raw[i];
        CHECK(a.x == b.x && a.y == b.y && a.w == b.w && a.frame == b.frame && a.scale_idx == b.scale_idx);
    }
    // the device's regions: the candidates bucketed by frame, in any order inside a frame
    std::vector<CvRoiDev> rois;
    for (int f = 0; f < nf; ++f)
        for (size_t i = raw.size(); i-- > 0;)
            if (raw[i].frame == f0 + f)
                rois.push_back(CvRoiDev{(uint32_t)f, (uint32_t)raw[i].x, (uint32_t)raw[i].y, (uint32_t)raw[i].w, (uint32_t)raw[i].h, {(uint32_t)i, 0, 0}});
    std::vector<int> ids;
    const size_t base = 1000;
    CHECK(cv_chain_region_ids(rois.data(), rois.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_OK && ids.size() == rois.size());
    for (size_t r = 0; r < rois.size(); ++r) {
        CHECK(ids[r] >= (int)base && ids[r] < (int)(base + raw.size()));
        const vj_rect& a = sorted[(size_t)ids[r] - base];
        CHECK((uint32_t)a.x == rois[r].x && (uint32_t)a.y == rois[r].y && (uint32_t)a.w == rois[r].w && a.frame == f0 + (int)rois[r].frame);
    }
    // the second cascade's detections through the ids; a region index or slot out of range is refused
    const std::vector<CvRoiFactor> factors = {cv_roi_factor(20, 20, 1.0), cv_roi_factor(20, 20, 1.1)};
    std::vector<CvDet> det = {{1, 2, 0, 0}, {3, 4, 1, (uint32_t)rois.size() - 1u}};
    std::vector<vj_rect> all;
    CHECK(cv_chain_rects_of(det.data(), det.size(), factors, ids, &all) == VJ_OK && all.size() == 2);
    CHECK(all[0].frame == ids[0] && all[1].frame == ids.back() && all[1].w == factors[1].win_w && all[1].scale_idx == 1);
    det.push_back(CvDet{0, 0, 0, (uint32_t)rois.size()});
    CHECK(cv_chain_rects_of(det.data(), det.size(), factors, ids, &all) == VJ_ERR_HIP);
    det.back() = CvDet{0, 0, 2, 0};
    CHECK(cv_chain_rects_of(det.data(), det.size(), factors, ids, &all) == VJ_ERR_HIP);
    CHECK(cv_chain_rects_of(nullptr, 0, factors, {}, &all) == VJ_OK);
    // refused: a source index out of range, one used twice, a missing region, a region that is not its candidate
    std::vector<CvRoiDev> bad = rois;
    bad[5].pad[0] = (uint32_t)raw.size();
    CHECK(cv_chain_region_ids(bad.data(), bad.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    bad[5].pad[0] = 0xffffffffu;
    CHECK(cv_chain_region_ids(bad.data(), bad.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    bad = rois;
    bad[7].pad[0] = bad[8].pad[0];
    CHECK(cv_chain_region_ids(bad.data(), bad.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    CHECK(cv_chain_region_ids(rois.data(), rois.size() - 1, raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    bad = rois;
    bad[9].x += 1u;
    CHECK(cv_chain_region_ids(bad.data(), bad.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    bad = rois;
    bad[0].frame = 0x80000000u;
    CHECK(cv_chain_region_ids(bad.data(), bad.size(), raw.data(), raw.size(), f0, base, &ids) == VJ_ERR_HIP);
    CHECK(cv_chain_region_ids(nullptr, 0, nullptr, 0, f0, base, &ids) == VJ_OK && ids.empty());
}

static void grouped_regions() {
    std::vector<vj_rect> regions(3, vj_rect{1, 1, 30, 30, 4.0f, 0, -1});
    std::vector<int> ids;
    const std::vector<CvRoiDev> rois = {{0, 5, 6, 40, 41, {3, 0, 0}}, {0, 50, 60, 24, 24, {7, 0, 0}}, {2, 9, 9, 100, 100, {4, 0, 0}}};
    CHECK(cv_chain_grouped_regions(rois.data(), rois.size(), 10, 3, &regions, &ids) == VJ_OK);
    CHECK(regions.size() == 6 && ids == (std::vector<int>{3, 4, 5}));
    CHECK(regions[5].frame == 12 && regions[5].x == 9 && regions[5].w == 100 && regions[5].weight == 4.0f && regions[5].scale_idx == -1);
    CHECK(regions[3].frame == 10 && regions[3].y == 6 && regions[3].h == 41 && regions[3].weight == 3.0f);
    CHECK(cv_chain_grouped_regions(nullptr, 0, 0, 1, &regions, &ids) == VJ_OK && ids.empty() && regions.size() == 6);
    std::vector<CvRoiDev> bad = rois;
    bad[2].frame = 3;                                             // beyond the sub-batch
    CHECK(cv_chain_grouped_regions(bad.data(), bad.size(), 10, 3, &regions, &ids) == VJ_ERR_HIP);
    bad = rois;
    bad[0].frame = 1;                                             // frames out of order
    CHECK(cv_chain_grouped_regions(bad.data(), bad.size(), 10, 3, &regions, &ids) == VJ_ERR_HIP);
    CHECK(cv_chain_grouped_regions(rois.data(), 1, 10, 0, &regions, &ids) == VJ_ERR_HIP);
}

static void info_and_state() {
    vj_cv_chain_info info{};
    cv_chain_info_add(&info, true, 5, 100, 1000);
    cv_chain_info_add(&info, false, 0, 0, 0);
    cv_chain_info_add(&info, true, 2, 0xffffffffull, 1ull << 40);
    CHECK(info.sub_batches == 3 && info.sub_batches_device == 2 && info.regions == 7 && info.units == 100 + 0xffffffffull &&
          info.windows == 1000 + (1ull << 40));
    CvChainState s{};
    CHECK(cv_chain_state_error(s) == VJ_OK);
    s.windows = 0xffffffffull;
    s.n_units = 0x7fffffffull;
    CHECK(cv_chain_state_error(s) == VJ_OK);
    s.windows += 1;
    CHECK(cv_chain_state_error(s) == VJ_ERR_LIMIT);
    s.windows = 0;
    s.n_units += 1;
    CHECK(cv_chain_state_error(s) == VJ_ERR_LIMIT);
    s = CvChainState{};
    s.err_reach = 1;
    CHECK(cv_chain_state_error(s) == VJ_ERR_LIMIT);
    s.err_factors = 1;
    CHECK(cv_chain_state_error(s) == VJ_ERR_LIMIT);
    s.err_outside = 1;                                            // the host refuses a region outside its frame first
    CHECK(cv_chain_state_error(s) == VJ_ERR_ARG);
}

// The restatement the device's unit builder runs (cv_chain_count_factors / cv_chain_slot, compiled here for the host) against
// cv_roi_build_units: every region size 1..640 x every slot, two scale factors, with and without a minimum size, a reach that
// refuses regions near the frame's end.
static void unit_restatement() {
    const int WIN_W = 20, WIN_H = 22, W = 640, H = 640;
    const uint32_t stride = (uint32_t)W + 1u, frame_elems = stride * ((uint32_t)H + 3u);
    for (const double sf : {1.1, 1.25}) {
        const int n_factors = cv_count_factors(WIN_W, WIN_H, W, H, sf, 4096);
        std::vector<CvRoiFactor> factors;
        std::vector<CvChainFactor> table;
        double factor = 1;
        for (int k = 0; k < n_factors; ++k, factor *= sf) {
            factors.push_back(cv_roi_factor(WIN_W, WIN_H, factor));
            factors.back().max_reach = 7;
            table.push_back(CvChainFactor{factor, factors.back().ystep, factors.back().win_w, factors.back().win_h, factors.back().max_reach});
        }
        for (const int min_size : {0, 45})
            for (int size = 1; size <= 640; ++size) {
                const int w = size, h = 1 + (size * 7) % 640;       // every width with some height, and the square
                for (const CvRoiHost& r : {CvRoiHost{0, 0, 0, w, h, 0}, CvRoiHost{0, W - size, H - size, size, size, 0}, CvRoiHost{0, 3, 5, h, w, 0}}) {
                    if (r.x + r.w > W || r.y + r.h > H) continue;
                    std::vector<CvRoiDev> rois;
                    std::vector<CvRoiUnit> units;
                    uint64_t windows = 0;
                    const int rc = cv_roi_build_units({r}, WIN_W, WIN_H, sf, factors, stride, frame_elems, min_size, min_size, &rois, &units, &windows);
                    const uint32_t nk = cv_chain_count_factors(table.data(), (uint32_t)table.size(), WIN_W, WIN_H, r.w, r.h);
                    CHECK((int)nk == std::min(cv_count_factors(WIN_W, WIN_H, r.w, r.h, sf, 4096), n_factors));
                    std::vector<CvRoiUnit> mine;
                    uint64_t my_windows = 0;
                    bool reach = false;
                    for (uint32_t k = 0; k < nk; ++k) {
                        int end_x, end_y;
                        const int what = cv_chain_slot(table[k], r.x, r.y, r.w, r.h, min_size, min_size, stride, frame_elems, &end_x, &end_y);
                        if (what == CV_CHAIN_SLOT_REACH) reach = true;
                        if (what != CV_CHAIN_SLOT_OK) continue;
                        for (int iy = 0; iy < end_y; ++iy) mine.push_back(CvRoiUnit{0, k, (uint32_t)iy, (uint32_t)end_x});
                        my_windows += (uint64_t)end_x * (uint64_t)end_y;
                    }
                    CHECK(reach == (rc == VJ_ERR_LIMIT) && (rc == VJ_OK || rc == VJ_ERR_LIMIT));
                    if (rc != VJ_OK) continue;
                    CHECK(my_windows == windows && mine.size() == units.size());
                    CHECK(mine.empty() || memcmp(mine.data(), units.data(), mine.size() * sizeof(CvRoiUnit)) == 0);
                }
            }
    }
    // halves: the grid end rounds to even, as cvRound does
    CHECK(cv_chain_grid_end(25, 20, 2.0) == 2 && cv_chain_grid_end(27, 20, 2.0) == 4 && cv_chain_grid_end(20, 21, 2.0) == 0 && cv_chain_grid_end(20, 23, 2.0) == -2);
}

int main() {
    route();
    rank_and_remap(false);
    rank_and_remap(true);
    grouped_regions();
    info_and_state();
    unit_restatement();
    printf("cv_chain_asan_driver: OK\n");
    return 0;
}
