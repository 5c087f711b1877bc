// CPU check of the strip rule the kernels and the host share (csrc/vj_sq_strips.hpp), a program of its own:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clfacedetection_amd/csrc tests/sq_strips_driver.cpp -o sq_strips && ./sq_strips < cases
// Reads "w h" lines.  For every window it (1) prints "w h rows k b0 ... bk": the strip height and the row boundaries at which
// sq_window_strips reads its corners (recorded through the loader; tests/test_sq_strips.py checks them and redoes the sums
// with numpy), and (2) checks the function's own arithmetic: the window sits at (x, y) = (1, 2) inside an image with a margin,
// all 255 and random {0, 255}, whose exact squared integral (u64) is reduced mod 2^32; the strips' sum from the reduced
// image must equal the true sum from the exact one.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vj_sq_strips.hpp"

using namespace vj;

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rng() {   // xorshift32
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static int check_window(uint32_t w, uint32_t h) {
    const uint32_t rows = sq_strip_rows(w);
    if (rows == 0u || (uint64_t)rows * w > SQ32_MAX_AREA || (uint64_t)(rows + 1u) * w <= SQ32_MAX_AREA) {
        printf("window %u x %u: strip height %u\n", w, h, rows);
        return 1;
    }
    const uint32_t X = 1u, Y = 2u, W = w + 2u, H = h + 3u, pitch = W + 1u;
    // (1) the boundaries, through a loader that records where it is asked to read
    std::vector<uint32_t> seen;
    const uint32_t c0 = Y * pitch + X;
    (void)sq_window_strips([&](uint32_t i) { seen.push_back(i); return 0u; }, c0, w, h * pitch, rows * pitch);
    if (seen.size() < 4u || seen.size() % 2u != 0u) {
        printf("window %u x %u: %zu reads\n", w, h, seen.size());
        return 1;
    }
    const size_t k = seen.size() / 2u - 1u;
    if (k != sq_strip_count(h, rows)) {
        printf("window %u x %u: %zu strips walked, sq_strip_count says %u\n", w, h, k, sq_strip_count(h, rows));
        return 1;
    }
    printf("%u %u %u %zu", w, h, rows, k);
    for (size_t j = 0; j < seen.size(); j += 2u) {
        const uint32_t l = seen[j], r = seen[j + 1u];
        if (r != l + w || l < c0 || (l - c0) % pitch != 0u) {
            printf("\nwindow %u x %u: corner pair %zu reads %u and %u\n", w, h, j / 2u, l, r);
            return 1;
        }
        printf(" %u", (l - c0) / pitch);
    }
    printf("\n");
    // (2) the arithmetic
    for (int content = 0; content < 2; ++content) {
        std::vector<uint64_t> sq((size_t)(H + 1u) * pitch, 0ull);
        for (uint32_t y = 0; y < H; ++y) {
            uint64_t row = 0;
            for (uint32_t x = 0; x < W; ++x) {
                const uint64_t p = content == 0 ? 255u : ((rng() >> 7) & 1u) * 255u;
                row += p * p;
                sq[(size_t)(y + 1u) * pitch + x + 1u] = sq[(size_t)y * pitch + x + 1u] + row;
            }
        }
        std::vector<uint32_t> lo(sq.size());
        for (size_t i = 0; i < sq.size(); ++i) lo[i] = (uint32_t)sq[i];
        const uint64_t want = sq[c0 + (size_t)h * pitch + w] - sq[c0 + (size_t)h * pitch] - sq[c0 + w] + sq[c0];
        const uint64_t got = sq_window_strips([&](uint32_t i) { return lo.at(i); }, c0, w, h * pitch, rows * pitch);
        if (got != want) {
            printf("window %u x %u, content %d: strips give %" PRIu64 ", the exact integral %" PRIu64 "\n", w, h, content, got, want);
            return 1;
        }
    }
    return 0;
}

int main() {
    static_assert(sq_strip_rows(257u) == 257u && sq_strip_rows(258u) == 256u && sq_strip_rows(1u) == SQ32_MAX_AREA &&
                      sq_strip_rows(SQ32_MAX_AREA) == 1u && sq_strip_rows(SQ32_MAX_AREA + 1u) == 0u && sq_strip_rows(0u) == 0u,
                  "strip heights at the edges");
    static_assert(sq_strip_count(257u, 257u) == 1u && sq_strip_count(258u, 256u) == 2u && sq_strip_count(SQ32_MAX_AREA + 1u, SQ32_MAX_AREA) == 2u,
                  "strip counts at the edges");
    unsigned w, h;
    int n = 0;
    while (scanf("%u %u", &w, &h) == 2) {
        if (check_window(w, h)) return 1;
        ++n;
    }
    printf("sq_strips_driver: OK %d\n", n);
    return 0;
}
