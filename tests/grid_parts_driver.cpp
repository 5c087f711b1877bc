// CPU check of the part-range arithmetic the grid pass and the host share (csrc/vj_grid_parts.hpp), a program of its own:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clfacedetection_amd/csrc tests/grid_parts_driver.cpp -o grid_parts && ./grid_parts
// For every total in [0, 4100] — and a few near 2^32, where the product total * x needs 64 bits — the GRID_PARTS ranges must be
// disjoint, ascending and cover [0, total); the sizes differ by at most one; home / next visit every part exactly once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vj_grid_parts.hpp"

using namespace vj;

static int check_total(uint32_t total) {
    if (grid_part_begin(total, 0) != 0u || grid_part_begin(total, GRID_PARTS) != total) {
        printf("total %u: parts span [%u, %u)\n", total, grid_part_begin(total, 0), grid_part_begin(total, GRID_PARTS));
        return 1;
    }
    uint32_t covered = 0, lo_size = UINT32_MAX, hi_size = 0;
    for (uint32_t x = 0; x < GRID_PARTS; ++x) {
        const uint32_t b = grid_part_begin(total, x), e = grid_part_begin(total, x + 1u);
        if (b != covered || e < b || e > total || grid_part_size(total, x) != e - b) {   // ascending, disjoint, without gaps
            printf("total %u part %u: [%u, %u) after %u covered\n", total, x, b, e, covered);
            return 1;
        }
        covered = e;
        lo_size = e - b < lo_size ? e - b : lo_size;
        hi_size = e - b > hi_size ? e - b : hi_size;
    }
    if (covered != total || hi_size - lo_size > 1u) {
        printf("total %u: covered %u, part sizes %u .. %u\n", total, covered, lo_size, hi_size);
        return 1;
    }
    if (total <= 4100u) {   // every item in exactly one part
        std::vector<uint8_t> seen(total, 0);
        for (uint32_t x = 0; x < GRID_PARTS; ++x)
            for (uint32_t i = grid_part_begin(total, x); i < grid_part_begin(total, x + 1u); ++i) ++seen[i];
        for (uint32_t i = 0; i < total; ++i)
            if (seen[i] != 1) {
                printf("total %u: item %u in %u parts\n", total, i, (unsigned)seen[i]);
                return 1;
            }
    }
    return 0;
}

int main() {
    for (uint32_t total = 0; total <= 4100u; ++total)
        if (check_total(total)) return 1;
    for (uint32_t total : {65535u, 65536u, 114560u, 0x1fffffffu, 0x20000000u, 0x7fffffffu, 0x80000001u, 0xfffffff7u, 0xffffffffu})
        if (check_total(total)) return 1;
    // the steal walk: from every home part, GRID_PARTS steps visit every part once and return home
    for (uint32_t block = 0; block < 64u; ++block) {
        uint32_t x = grid_part_home(block), mask = 0;
        if (x >= GRID_PARTS || x != block % GRID_PARTS) {
            printf("block %u: home part %u\n", block, x);
            return 1;
        }
        for (uint32_t k = 0; k < GRID_PARTS; ++k) {
            mask |= 1u << x;
            x = grid_part_next(x);
        }
        if (mask != (1u << GRID_PARTS) - 1u || x != grid_part_home(block)) {
            printf("block %u: walk visits %#x, ends on %u\n", block, mask, x);
            return 1;
        }
    }
    printf("grid_parts_driver: OK\n");
    return 0;
}
