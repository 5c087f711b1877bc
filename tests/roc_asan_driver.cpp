// Sanitizer driver of the host code vj_detect_opencv_roc adds (csrc/vj_group.cpp: vj_group_rectangles_levels and the level branch of
// group_rectangles): built by tests/test_sanitizers_roc.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/roc_asan_driver.cpp csrc/vj_group.cpp csrc/vj_cascade.cpp
// (no HIP involved).  Degenerate lists — empty, one rectangle, null pointers, rectangles outside an image, every rectangle its own
// class, one class of thousands, frames of one rectangle each, extreme levels and weights — must come back as counts or error codes;
// every memory error or undefined behaviour aborts the process.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/vj.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint32_t rng_state = 11;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

struct Lists {
    std::vector<vj_rect> r;
    std::vector<int32_t> lv;
    std::vector<double> lw;
    void add(int x, int y, int w, int h, int frame, int level, double weight) {
        r.push_back(vj_rect{x, y, w, h, 0.0f, frame, 0});
        lv.push_back(level);
        lw.push_back(weight);
    }
    int group(int thr, double eps = 0.2) { return vj_group_rectangles_levels(r.data(), lv.data(), lw.data(), (int)r.size(), thr, eps); }
};

int main() {
    // empty, null, negative
    CHECK(vj_group_rectangles_levels(nullptr, nullptr, nullptr, 0, 3, 0.2) == 0);
    CHECK(vj_group_rectangles_levels(nullptr, nullptr, nullptr, 0, 0, 0.2) == 0);
    CHECK(vj_group_rectangles_levels(nullptr, nullptr, nullptr, 5, 3, 0.2) == -VJ_ERR_ARG);
    CHECK(vj_group_rectangles_levels(nullptr, nullptr, nullptr, -1, 3, 0.2) == -VJ_ERR_ARG);
    {
        Lists l;
        l.add(0, 0, 20, 20, 0, 22, 1.0);
        CHECK(vj_group_rectangles_levels(l.r.data(), nullptr, l.lw.data(), 1, 3, 0.2) == -VJ_ERR_ARG);
        CHECK(vj_group_rectangles_levels(l.r.data(), l.lv.data(), nullptr, 1, 3, 0.2) == -VJ_ERR_ARG);
        CHECK(vj_group_rectangles_levels(l.r.data(), l.lv.data(), l.lw.data(), 1, 3, -1.0) == -VJ_ERR_ARG);
        CHECK(vj_group_rectangles_levels(l.r.data(), l.lv.data(), l.lw.data(), 1, 3, NAN) == -VJ_ERR_ARG);
        CHECK(l.group(3) == 1 && l.lv[0] == 22 && l.lw[0] == 1.0 && l.r[0].scale_idx == -1);   // one rectangle: its level decides
        CHECK(l.group(22) == 0);
    }
    {   // not image rectangles
        Lists l;
        l.add(INT_MAX, 0, 20, 20, 0, 5, 0.0);
        CHECK(l.group(1) == -VJ_ERR_ARG);
        l.r[0] = vj_rect{0, 0, -1, 20, 0.0f, 0, 0};
        CHECK(l.group(1) == -VJ_ERR_ARG);
    }
    {   // threshold <= 0: levels become 1, nothing else moves
        Lists l;
        for (int k = 0; k < 7; ++k) l.add(k, k, 20, 20, k / 3, 10 + k, -1.0 * k);
        CHECK(l.group(0) == 7 && l.group(-5) == 7 && l.group(INT_MIN) == 7);
        for (int k = 0; k < 7; ++k) CHECK(l.lv[k] == 1 && l.lw[k] == -1.0 * k && l.r[k].x == k);
    }
    {   // extreme levels and weights: INT_MAX / INT_MIN / 0 levels, infinities, NaN, DBL_MIN's neighbours
        Lists l;
        const double ws[] = {INFINITY, -INFINITY, NAN, DBL_MIN, -DBL_MIN, 0.0, -0.0, DBL_MAX, -DBL_MAX};
        const int ls[] = {INT_MAX, INT_MIN, 0, -1, 1, INT_MAX, 0, INT_MIN, 2};
        for (int k = 0; k < 9; ++k) l.add(100 + (k & 1), 100, 30, 30, 0, ls[k], ws[k]);
        const int n = l.group(INT_MAX - 1);
        CHECK(n == 1 && l.lv[0] == INT_MAX && l.lw[0] == INFINITY);
        Lists z;   // no member above level 0: the class keeps level 0 and DBL_MIN, and is dropped by any positive threshold
        for (int k = 0; k < 4; ++k) z.add(5, 5, 20, 20, 0, -k, -3.0);
        CHECK(z.group(1) == 0);
    }
    {   // every rectangle its own class; one class of thousands; frames of one rectangle each
        Lists l;
        for (int k = 0; k < 500; ++k) l.add(k * 100, 0, 20, 20, 0, 1 + k % 30, (double)k);
        CHECK(l.group(15) == 245);   // levels 16..30 of 1 + k % 30
        Lists m;
        for (int k = 0; k < 3000; ++k) m.add(50 + (int)(rnd() % 3), 50 + (int)(rnd() % 3), 40, 40, 0, 19 + (int)(rnd() % 4), (double)(rnd() % 1000) - 500.0);
        CHECK(m.group(20) == 1 && m.lv[0] == 22);
        Lists f;
        for (int k = 0; k < 300; ++k) f.add(0, 0, 20, 20, k, k % 5, 0.5);
        const int n = f.group(2);
        CHECK(n == 120);
        for (int k = 0; k < n; ++k) CHECK(f.lv[k] > 2 && f.r[k].frame % 5 == f.lv[k]);
    }
    {   // random lists, random thresholds: counts stay within the input, levels come from the input
        for (int it = 0; it < 200; ++it) {
            Lists l;
            const int n = (int)(rnd() % 60);
            for (int k = 0; k < n; ++k)
                l.add((int)(rnd() % 200), (int)(rnd() % 200), 20 + (int)(rnd() % 40), 20 + (int)(rnd() % 40), k * 3 / (n + 1), (int)(rnd() % 25), (double)(rnd() % 2000) / 100.0 - 10.0);
            const int m = l.group(1 + (int)(rnd() % 23));
            CHECK(m >= 0 && m <= n);
            for (int k = 0; k < m; ++k) CHECK(l.lv[k] >= 0 && l.lv[k] < 25 && l.r[k].scale_idx == -1 && l.r[k].weight == 0.0f);
        }
    }
    printf("roc_asan_driver: OK\n");
    return 0;
}
