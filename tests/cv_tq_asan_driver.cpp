// Sanitizer driver of the tree queue's sizing (csrc/vj_cv_tq_host.hpp: cv_tq_sizing, what vj_detect_opencv's stage-tree tile path
// asks before it launches): built by tests/test_sanitizers_cv_tq.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cv_tq_asan_driver.cpp
// (no HIP involved; cv_tq_first / cv_tq_cap and CV_TQ_MAX are vj_device.hpp's own).  Against brute force, for shifts 0..4, 1..64
// tile scales of random grids whose windows put want(nf) next to CV_TQ_MAX for some nf in 1..200:
//   "queue of N"   comes out exactly when want(nf) <= CV_TQ_MAX; every scale's sub-queue [first, first + cap) lies inside [0, N) and
//                  no two overlap, with tq_win_first / tq_slot as the planner builds them (prefix sums in scale order);
//   "resplit to M" M frames fit, M + 1 do not, 1 <= M <= max_frames;
//   "rows only"    comes out exactly when not even one frame fits.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_cv_tq_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

struct Scale { uint32_t end_x, end_y, tq_win_first, tq_slot; };

// n scales whose grid windows add up to about `target` (< 2^32: a frame's windows fit the 32-bit detection count)
static std::vector<Scale> make_scales(std::mt19937_64& rng, uint32_t n, uint64_t target, uint64_t* tile_windows) {
    std::vector<Scale> s(n);
    uint64_t left = target, first = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t room = std::max<uint64_t>(1, left / (n - k));
        const uint64_t share = k + 1 == n ? std::max<uint64_t>(1, left) : 1 + rng() % std::min<uint64_t>(2 * room, std::max<uint64_t>(1, left));
        const uint64_t lo = share / 65535u + 1u, hi = std::min<uint64_t>(65535u, share);
        const uint64_t ex = lo >= hi ? hi : lo + rng() % (hi - lo + 1);
        const uint64_t ey = std::max<uint64_t>(1, std::min<uint64_t>(65535u, share / ex));
        s[k] = Scale{(uint32_t)ex, (uint32_t)ey, (uint32_t)first, k};
        first += ex * ey;
        left -= std::min(left, ex * ey);
    }
    CHECK(first <= 0xffffffffull);
    *tile_windows = first;
    return s;
}

static uint64_t want_of(uint64_t tile_windows, uint32_t n_scales, uint64_t nf, uint32_t shift, bool chain_pass) {
    return ((tile_windows * nf) >> shift) + (chain_pass ? (uint64_t)n_scales * 4096u + 4096u : 4096u);
}

int main() {
    std::mt19937_64 rng(20240607);
    size_t n_queue = 0, n_rows = 0, n_resplit = 0, n_edge = 0;
    for (uint32_t shift = 0; shift <= 4; ++shift)
        for (uint32_t n = 1; n <= 64; ++n)
            for (int rep = 0; rep < 12; ++rep) {
                const bool chain_pass = rep % 4 != 3;
                const uint64_t fixed = chain_pass ? (uint64_t)n * 4096u + 4096u : 4096u;
                // the frame count at which the queue is to reach CV_TQ_MAX, and a plan whose windows put it there
                const uint64_t n_star = rep % 6 == 5 ? 1 : 1 + rng() % 200;   // (1: "not even one frame" on one side of it)
                const uint64_t at = ((CV_TQ_MAX - fixed + 1u) << shift) / n_star;
                const uint64_t target = std::min<uint64_t>(0xffff0000ull, rep % 3 == 0 ? at : at - std::min<uint64_t>(at - 1, 70000u) + rng() % 140000u);
                uint64_t tw = 0;
                const std::vector<Scale> scales = make_scales(rng, n, target, &tw);
                const uint64_t probes[] = {1, 200, n_star > 1 ? n_star - 1 : 1, n_star, std::min<uint64_t>(200, n_star + 1), 1 + rng() % 200};
                for (const uint64_t nf : probes) {
                    const int max_frames = (int)(nf + rng() % 3);   // (a sub-batch never has more frames than max_frames)
                    const CvTqSizing sz = cv_tq_sizing(tw, n, (uint32_t)nf, shift, 0, chain_pass, max_frames);
                    const bool fits = want_of(tw, n, nf, shift, chain_pass) <= CV_TQ_MAX;
                    const bool one_fits = want_of(tw, n, 1, shift, chain_pass) <= CV_TQ_MAX;
                    if (fits ? want_of(tw, n, nf + 1, shift, chain_pass) > CV_TQ_MAX : nf == 1 || want_of(tw, n, nf - 1, shift, chain_pass) <= CV_TQ_MAX)
                        ++n_edge;   // nf is the last count that fits, or the first that does not
                    CHECK((sz.kind == CvTqSizing::QUEUE) == fits);
                    CHECK((sz.kind == CvTqSizing::ROWS_ONLY) == !one_fits);
                    if (sz.kind == CvTqSizing::QUEUE) {
                        ++n_queue;
                        const uint64_t N = sz.n;
                        CHECK(N == want_of(tw, n, nf, shift, chain_pass) && N <= CV_TQ_MAX);
                        if (!chain_pass) continue;   // (one flat queue of N entries)
                        uint64_t end_before = 0;
                        for (const Scale& s : scales) {   // in scale order: sorted by first, so disjoint when each starts at or after the last one's end
                            const uint64_t first = cv_tq_first(s.tq_win_first, s.tq_slot, (uint32_t)nf, shift);
                            const uint64_t cap = cv_tq_cap(s.end_x, s.end_y, (uint32_t)nf, shift);
                            CHECK(cap >= 4096u && first >= end_before && first + cap <= N);
                            end_before = first + cap;
                        }
                    } else if (sz.kind == CvTqSizing::RESPLIT) {
                        ++n_resplit;
                        const uint64_t M = sz.n;
                        CHECK(M >= 1 && M <= (uint64_t)max_frames && M < nf);
                        uint64_t brute = 0;
                        for (uint64_t m = 1; m <= (uint64_t)max_frames; ++m)
                            if (want_of(tw, n, m, shift, chain_pass) <= CV_TQ_MAX) brute = m;
                        CHECK(M == brute);
                        CHECK(want_of(tw, n, M, shift, chain_pass) <= CV_TQ_MAX && want_of(tw, n, M + 1, shift, chain_pass) > CV_TQ_MAX);
                    } else {
                        ++n_rows;
                    }
                    // a forced capacity is the queue, whatever the batch
                    const CvTqSizing forced = cv_tq_sizing(tw, n, (uint32_t)nf, shift, 16, chain_pass, max_frames);
                    CHECK(forced.kind == CvTqSizing::QUEUE && forced.n == 16u);
                }
            }
    // a plan without tile windows: the fixed part alone
    CHECK(cv_tq_sizing(0, 3, 200, 4, 0, true, 200).kind == CvTqSizing::QUEUE && cv_tq_sizing(0, 3, 200, 4, 0, true, 200).n == 4u * 4096u);
    CHECK(n_queue > 1000 && n_rows > 100 && n_resplit > 1000 && n_edge > 1000);   // (every outcome and the boundary were reached)
    printf("cv_tq_asan_driver: OK (%zu queue, %zu resplit, %zu rows only, %zu at the boundary)\n", n_queue, n_resplit, n_rows, n_edge);
    return 0;
}
