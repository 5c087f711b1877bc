// Sanitizer driver of the host code vj_run_windows_opencv adds (csrc/vj_cv_points_host.cpp: argument checks, what a scale gives, the
// grouping by (sub-batch, scale slot), the unit list, the scatter of the verdicts): built by tests/test_sanitizers_run_windows.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/run_windows_asan_driver.cpp csrc/vj_cv_points_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_group.cpp csrc/vj_cascade.cpp
// (no HIP involved).  Degenerate lists — empty, null, one window, 2^20 windows of one scale, every window its own scale, extreme
// coordinates, indices out of range — must come back as lists or error codes; every memory error or undefined behaviour aborts.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_cv_points_host.hpp"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

using namespace vj;

static uint32_t rng_state = 7;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// the whole host pipeline of a call on `windows`, the device replaced by a function of the point: the verdicts come back in the
// caller's order, every window exactly once, every unit within one slot and 64 windows
static void pipeline(const std::vector<vj_window>& windows, int n_frames, int n_scales, int max_frames) {
    const uint32_t n = (uint32_t)windows.size();
    std::vector<uint32_t> order;
    std::vector<size_t> sub_first;
    cv_points_order(windows.data(), n, n_frames, max_frames, &order, &sub_first);
    CHECK(order.size() == n && sub_first.back() == n && sub_first.front() == 0);
    std::vector<vj_window_result> out(n, vj_window_result{77, 78, 79.0});
    std::vector<CvPointDev> points;
    std::vector<CvPointUnit> units;
    std::vector<CvPointResult> res;
    size_t seen = 0;
    for (size_t b = 0; b + 1 < sub_first.size(); ++b) {
        CHECK(sub_first[b] <= sub_first[b + 1]);
        const size_t m = sub_first[b + 1] - sub_first[b];
        if (m == 0) continue;
        const int f0 = (int)b * max_frames;
        const uint32_t* ord = order.data() + sub_first[b];
        cv_points_build(windows.data(), ord, m, f0, &points, &units);
        CHECK(points.size() == m);
        size_t covered = 0;
        uint32_t last_slot = 0;
        for (size_t u = 0; u < units.size(); ++u) {
            const CvPointUnit& un = units[u];
            CHECK(un.first == covered && un.count >= 1 && un.count <= CV_POINT_UNIT && (int)un.slot < n_scales);
            CHECK(u == 0 || un.slot >= last_slot);                              // ordered by slot
            last_slot = un.slot;
            for (uint32_t k = 0; k < un.count; ++k) {
                const CvPointDev& p = points[un.first + k];
                const vj_window& w = windows[ord[un.first + k]];
                CHECK(p.index == un.first + k && (uint32_t)w.scale == un.slot && p.x == w.x && p.y == w.y);
                CHECK((int)p.frame == w.frame - f0 && (int)p.frame < max_frames);
            }
            covered += un.count;
        }
        CHECK(covered == m);
        // stable within a slot: the caller's indices rise
        for (size_t k = 1; k < m; ++k)
            if (windows[ord[k]].scale == windows[ord[k - 1]].scale) CHECK(ord[k] > ord[k - 1]);
        res.resize(m);
        for (size_t k = 0; k < m; ++k) res[k] = CvPointResult{(int32_t)ord[k], 5, (double)points[k].x};
        cv_points_scatter(res.data(), ord, m, out.data());
        seen += m;
    }
    CHECK(seen == n);
    for (uint32_t i = 0; i < n; ++i) CHECK(out[i].result == (int32_t)i && out[i].reserved == 0 && out[i].stage_sum == (double)windows[i].x);
}

int main() {
    vj_cascade c;
    c.win_w = 20;
    c.win_h = 20;
    c.stages.resize(3);
    for (auto& s : c.stages) s.next = -1;
    vj_cascade tree = c;
    tree.stages[1].next = 2;
    std::vector<uint8_t> pix(64 * 48, 0);
    const vj_image frames[2] = {vj_image{pix.data(), 64, 48, 64, 0, 1}, vj_image{pix.data(), 64, 48, 64, 0, 1}};
    const double scales[3] = {1.0, 1.5, 2.5};
    vj_window_result out[4];
    int W = 0, H = 0, CH = 0;
    const vj_window one[1] = {{0, 3, 4, 1}};

    // empty and null lists
    CHECK(cv_points_check(&c, nullptr, 0, nullptr, 0, nullptr, 0, 0, nullptr, &W, &H, &CH) == VJ_OK);
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 0, 0, out, &W, &H, &CH) == VJ_OK);
    CHECK(cv_points_check(nullptr, frames, 2, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, nullptr, 2, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, nullptr, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, scales, 3, nullptr, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 1, 0, nullptr, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 0, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, scales, 0, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    // one window
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_OK && W == 64 && H == 48 && CH == 1);
    // start_stage
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 1, -1, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 1, INT_MIN, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&c, frames, 2, scales, 3, one, 1, INT_MAX, out, &W, &H, &CH) == VJ_OK);
    CHECK(cv_points_check(&tree, frames, 2, scales, 3, one, 1, 1, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&tree, frames, 2, scales, 3, one, 0, 1, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(cv_points_check(&tree, frames, 2, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_OK);
    // indices out of range, extreme coordinates (which are no error)
    for (int frame : {-1, 2, INT_MAX, INT_MIN}) {
        const vj_window w[2] = {{0, 0, 0, 0}, {frame, 0, 0, 0}};
        CHECK(cv_points_check(&c, frames, 2, scales, 3, w, 2, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    for (int scale : {-1, 3, INT_MAX, INT_MIN}) {
        const vj_window w[2] = {{0, 0, 0, 0}, {1, 0, 0, scale}};
        CHECK(cv_points_check(&c, frames, 2, scales, 3, w, 2, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    {
        const vj_window w[4] = {{0, INT_MAX, INT_MIN, 0}, {1, INT_MIN, INT_MAX, 2}, {1, -1, -1, 1}, {0, INT_MAX, INT_MAX, 2}};
        CHECK(cv_points_check(&c, frames, 2, scales, 3, w, 4, 0, out, &W, &H, &CH) == VJ_OK);
        pipeline(std::vector<vj_window>(w, w + 4), 2, 3, 1);
        pipeline(std::vector<vj_window>(w, w + 4), 2, 3, 2);
    }
    // scales that are none
    for (double bad : {0.0, -1.0, -0.0, std::nan(""), (double)INFINITY, -(double)INFINITY}) {
        const double s[2] = {1.0, bad};
        CHECK(cv_points_check(&c, frames, 2, s, 2, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    // what a scale gives: tiny, ties, huge (clamped: no int overflows)
    for (double s : {std::numeric_limits<double>::denorm_min(), 1e-9, 0.01, 0.5, 1.0, 1.37, 2.5, 3.2, 1e6, 1e300, std::numeric_limits<double>::max()}) {
        const CvPointScale k = cv_point_scale(20, 20, s, 64, 48);
        CHECK(k.win_w >= 0 && k.win_w <= (int)CV_POINT_WIN_MAX && k.win_h >= 0 && k.win_h <= (int)CV_POINT_WIN_MAX);
        CHECK(k.fits == (k.win_w <= 64 && k.win_h <= 48));
    }
    CHECK(cv_point_scale(20, 20, 2.5, 64, 48).win_w == 50 && cv_point_scale(20, 20, 2.5, 64, 48).ew == 45 && !cv_point_scale(20, 20, 2.5, 64, 48).fits);
    CHECK(cv_point_scale(20, 20, 2.4, 64, 48).fits && cv_point_scale(20, 20, 2.4, 64, 48).win_h == 48);
    CHECK(cv_point_scale(5, 5, 2.5, 640, 480).win_w == 12);                    // 12.5: half to even
    // frames that are not uniform
    {
        const vj_image mixed[2] = {frames[0], vj_image{pix.data(), 32, 48, 32, 0, 1}};
        CHECK(cv_points_check(&c, mixed, 2, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
        const vj_image empty[1] = {vj_image{nullptr, 64, 48, 64, 0, 1}};
        CHECK(cv_points_check(&c, empty, 1, scales, 3, one, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    // the pipeline: empty, one window, 2^20 windows of one scale, every window its own scale, a shuffled mix over sub-batches
    pipeline({}, 2, 3, 1);
    pipeline({{1, 3, 4, 2}}, 2, 3, 1);
    pipeline({{1, 3, 4, 2}}, 2, 3, 64);
    {
        std::vector<vj_window> w(1u << 20);
        for (size_t i = 0; i < w.size(); ++i) w[i] = vj_window{(int32_t)(rnd() % 9), (int32_t)rnd(), (int32_t)rnd(), 5};
        pipeline(w, 9, 6, 2);
        pipeline(w, 9, 6, 9);
    }
    {
        std::vector<vj_window> w(1u << 16);
        for (size_t i = 0; i < w.size(); ++i) w[i] = vj_window{(int32_t)(rnd() % 3), (int32_t)i, -(int32_t)i, (int32_t)(w.size() - 1 - i)};
        pipeline(w, 3, (int)w.size(), 1);
        pipeline(w, 3, (int)w.size(), 3);
    }
    {
        std::vector<vj_window> w(5000);
        for (size_t i = 0; i < w.size(); ++i) w[i] = vj_window{(int32_t)(rnd() % 7), (int32_t)(rnd() % 200) - 20, (int32_t)(rnd() % 200) - 20, (int32_t)(rnd() % 11)};
        for (int mf : {1, 2, 3, 7, 100}) pipeline(w, 7, 11, mf);
        for (size_t n : {(size_t)63, (size_t)64, (size_t)65, (size_t)129}) pipeline(std::vector<vj_window>(w.begin(), w.begin() + (long)n), 7, 11, 7);
    }
    printf("run_windows_asan_driver: OK\n");
    return 0;
}
