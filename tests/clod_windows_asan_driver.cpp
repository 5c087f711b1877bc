// Sanitizer driver of the host code vj_run_windows adds (csrc/vj_points_host.cpp: argument checks, what a scale gives, the scatter
// of the verdicts) together with the grouping it reuses (csrc/vj_cv_points_host.cpp): built by tests/test_sanitizers_clod_windows.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/clod_windows_asan_driver.cpp csrc/vj_points_host.cpp csrc/vj_cv_points_host.cpp csrc/vj_cv_roi_host.cpp csrc/vj_group.cpp
//       csrc/vj_cascade.cpp
// (no HIP involved).  Degenerate lists — empty, null, one window, 2^20 windows of one scale, every window its own scale, extreme
// coordinates, indices out of range — must come back as lists or error codes; every memory error or undefined behaviour aborts.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_points_host.hpp"

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
    std::vector<vj_clod_window_result> out(n, vj_clod_window_result{77, 78.0f, 79.0f, 80});
    std::vector<CvPointDev> points;
    std::vector<CvPointUnit> units;
    std::vector<ClodPointResult> res;
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
        for (size_t u = 0; u < units.size(); ++u) {
            const CvPointUnit& un = units[u];
            CHECK(un.first == covered && un.count >= 1 && un.count <= CV_POINT_UNIT && (int)un.slot < n_scales);
            CHECK(u == 0 || un.slot >= units[u - 1].slot);                     // ordered by slot
            for (uint32_t k = 0; k < un.count; ++k) {
                const CvPointDev& p = points[un.first + k];
                const vj_window& w = windows[ord[un.first + k]];
                CHECK(p.index == un.first + k && (uint32_t)w.scale == un.slot && p.x == w.x && p.y == w.y);
                CHECK((int)p.frame == w.frame - f0 && (int)p.frame < max_frames);
            }
            covered += un.count;
        }
        CHECK(covered == m);
        res.resize(m);
        for (size_t k = 0; k < m; ++k) res[k] = ClodPointResult{(int32_t)ord[k], (float)points[k].y, (float)points[k].x, 5};
        clod_points_scatter(res.data(), ord, m, out.data());
        seen += m;
    }
    CHECK(seen == n);
    for (uint32_t i = 0; i < n; ++i)
        CHECK(out[i].result == (int32_t)i && out[i].reserved == 0 && out[i].stage_sum == (float)windows[i].x && out[i].variance == (float)windows[i].y);
}

int main() {
    vj_cascade c;
    c.win_w = 20;
    c.win_h = 20;
    c.stages.resize(3);
    for (auto& s : c.stages) s.next = -1;
    c.nodes.resize(2);
    for (auto& nd : c.nodes) nd.tilted = 0;
    vj_cascade tree = c;
    tree.stages[1].next = 2;
    vj_cascade tilted = c;
    tilted.nodes[1].tilted = 1;
    std::vector<uint8_t> pix(64 * 48, 0);
    const vj_image frames[2] = {vj_image{pix.data(), 64, 48, 64, 0, 1}, vj_image{pix.data(), 64, 48, 64, 0, 1}};
    const float scales[3] = {1.0f, 1.5f, 2.5f};
    vj_clod_window_result out[4];
    int W = 0, H = 0, CH = 0;
    const vj_window one[1] = {{0, 3, 4, 1}};
    const uint32_t SM = VJ_FLAG_SIGNED_MEAN, TU = VJ_FLAG_TILTED_AS_UPRIGHT;

    // empty and null lists
    CHECK(clod_points_check(&c, nullptr, 0, nullptr, 0, nullptr, 0, 0, 0, nullptr, &W, &H, &CH) == VJ_OK);
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 0, 0, 0, out, &W, &H, &CH) == VJ_OK);
    CHECK(clod_points_check(nullptr, frames, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, nullptr, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, nullptr, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, scales, 3, nullptr, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, 0, 0, nullptr, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 0, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, scales, 0, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    // one window
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_OK && W == 64 && H == 48 && CH == 1);
    // start_stage
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, -1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, INT_MIN, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, INT_MAX, 0, out, &W, &H, &CH) == VJ_OK);
    CHECK(clod_points_check(&tree, frames, 2, scales, 3, one, 1, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&tree, frames, 2, scales, 3, one, 0, 1, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    CHECK(clod_points_check(&tree, frames, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_OK);
    // flags: the two that are honoured, every other bit, tilted features with and without the flag (checked before the empty list)
    CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, 0, SM | TU, out, &W, &H, &CH) == VJ_OK);
    for (int bit = 0; bit < 32; ++bit) {
        const uint32_t f = 1u << bit;
        const int want = (f == SM || f == TU) ? VJ_OK : VJ_ERR_ARG;
        CHECK(clod_points_check(&c, frames, 2, scales, 3, one, 1, 0, f, out, &W, &H, &CH) == want);
        CHECK(clod_points_check(&c, nullptr, 0, nullptr, 0, nullptr, 0, 0, f, nullptr, &W, &H, &CH) == want);
    }
    CHECK(clod_points_check(&tilted, frames, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_UNSUPPORTED);
    CHECK(clod_points_check(&tilted, frames, 2, scales, 3, one, 1, 0, SM, out, &W, &H, &CH) == VJ_ERR_UNSUPPORTED);
    CHECK(clod_points_check(&tilted, frames, 2, scales, 3, one, 1, 0, TU, out, &W, &H, &CH) == VJ_OK);
    // indices out of range, extreme coordinates (which are no error)
    for (int frame : {-1, 2, INT_MAX, INT_MIN}) {
        const vj_window w[2] = {{0, 0, 0, 0}, {frame, 0, 0, 0}};
        CHECK(clod_points_check(&c, frames, 2, scales, 3, w, 2, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    for (int scale : {-1, 3, INT_MAX, INT_MIN}) {
        const vj_window w[2] = {{0, 0, 0, 0}, {1, 0, 0, scale}};
        CHECK(clod_points_check(&c, frames, 2, scales, 3, w, 2, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    {
        const vj_window w[4] = {{0, INT_MAX, INT_MIN, 0}, {1, INT_MIN, INT_MAX, 2}, {1, -1, -1, 1}, {0, INT_MAX, INT_MAX, 2}};
        CHECK(clod_points_check(&c, frames, 2, scales, 3, w, 4, 0, 0, out, &W, &H, &CH) == VJ_OK);
        pipeline(std::vector<vj_window>(w, w + 4), 2, 3, 1);
        pipeline(std::vector<vj_window>(w, w + 4), 2, 3, 2);
    }
    // scales that are none, and scales whose window or variance rectangle is empty
    for (float bad : {0.0f, -1.0f, -0.0f, std::nanf(""), INFINITY, -INFINITY, std::numeric_limits<float>::denorm_min(), 1e-9f, 0.02f, 0.026f}) {
        const float s[2] = {1.0f, bad};
        CHECK(clod_points_check(&c, frames, 2, s, 2, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
    }
    // what a scale gives: small, ties, huge (clamped: no int overflows)
    for (float s : {0.03f, 0.5f, 1.0f, 1.37f, 2.5f, 3.2f, 1e6f, 1e30f, std::numeric_limits<float>::max()}) {
        ClodPointScale k;
        CHECK(clod_point_scale(20, 20, s, 64, 48, &k) == VJ_OK);
        CHECK(k.win_w >= 1 && k.win_w <= (int)CV_POINT_WIN_MAX && k.win_h >= 1 && k.win_h <= (int)CV_POINT_WIN_MAX && k.area >= 1u);
        CHECK(k.ew <= k.win_w && k.eh <= k.win_h && k.fits == (k.win_w <= 64 && k.win_h <= 48));
    }
    {
        ClodPointScale k;
        CHECK(clod_point_scale(20, 20, 2.5f, 64, 48, &k) == VJ_OK && k.win_w == 50 && k.ex == 3 && k.ew == 45 && k.area == 2025u && !k.fits);
        CHECK(clod_point_scale(20, 20, 2.4f, 64, 48, &k) == VJ_OK && k.fits && k.win_h == 48);
        CHECK(clod_point_scale(5, 5, 2.5f, 640, 480, &k) == VJ_OK && k.win_w == 13);   // 12.5: half away from zero
        CHECK(clod_point_scale(20, 20, 0.026f, 64, 48, &k) == VJ_ERR_ARG && k.win_w == 1 && k.area == 0u);
        CHECK(clod_point_scale(20, 20, 1e30f, 64, 48, &k) == VJ_OK && k.win_w == (int)CV_POINT_WIN_MAX && k.area == 0xffffffffu);
    }
    // frames that are not uniform
    {
        const vj_image mixed[2] = {frames[0], vj_image{pix.data(), 32, 48, 32, 0, 1}};
        CHECK(clod_points_check(&c, mixed, 2, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
        const vj_image empty[1] = {vj_image{nullptr, 64, 48, 64, 0, 1}};
        CHECK(clod_points_check(&c, empty, 1, scales, 3, one, 1, 0, 0, out, &W, &H, &CH) == VJ_ERR_ARG);
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
    printf("clod_windows_asan_driver: OK\n");
    return 0;
}
