// CPU check of the gather chain's queue arithmetic and first-pass unit cutting (csrc/vj_gather_queue.hpp, shared by the kernel and
// the host), a program of its own:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clfacedetection_amd/csrc tests/gather_queue_driver.cpp -o gather_queue
//   ./gather_queue grids.txt        (grids.txt: one "nx ny row0" per line — the grids of a plan's scales)
// 1. For 1 ... 8 waves (and the values a caller may pass beyond): the capacity is a multiple of 64, waves * cap fits the
//    workgroup's array, the stump-parallel tail's scratch fits a wave's queue at the clamp and not one step of 8 above it.
//    Prints "cap <waves> <cap> <tail>" per wave count for the caller to compare.
// 2. For every grid of the file, every wave count and a set of block widths: every unit holds at most cap windows; walked as the
//    grid pass walks them (clipped to the grid), the units cover every window of the rows from row0 on exactly once and no other.
//    Prints "units <waves> <count>": the units of all the file's grids from their row0 on at the shipped block width, which the
//    caller compares with the plan's own count.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vj_gather_queue.hpp"

using namespace vj;

struct Unit { uint32_t first, count, bw; };

static int check_grid(uint32_t nx, uint32_t ny, uint32_t row0, uint32_t block_w, uint32_t cap) {
    std::vector<Unit> units;
    gather_cut_units(nx, ny, row0, block_w, cap, [&](uint32_t first, uint32_t count, uint32_t bw) { units.push_back(Unit{first, count, bw}); });
    std::vector<uint8_t> seen((size_t)nx * ny, 0);
    for (const Unit& u : units) {
        if (u.count == 0u || u.count > cap || (u.bw != 0u && u.count % u.bw != 0u)) {
            printf("grid %u x %u from row %u, block_w %u, cap %u: unit of %u windows, width %u\n", nx, ny, row0, block_w, cap, u.count, u.bw);
            return 1;
        }
        for (uint32_t i = 0; i < u.count; ++i) {   // cascade_pass<FROM_GRID>'s walk
            uint32_t ix, iy;
            if (u.bw != 0u) {
                const uint32_t ty = i / u.bw;
                ix = (u.first & 0xffffu) + (i - ty * u.bw);
                iy = (u.first >> 16) + ty;
            } else {
                iy = (u.first + i) / nx;
                ix = u.first + i - iy * nx;
            }
            if (ix < nx && iy < ny) ++seen[(size_t)iy * nx + ix];
        }
    }
    for (uint32_t iy = 0; iy < ny; ++iy)
        for (uint32_t ix = 0; ix < nx; ++ix)
            if (seen[(size_t)iy * nx + ix] != (iy >= row0 ? 1 : 0)) {
                printf("grid %u x %u from row %u, block_w %u, cap %u: window (%u, %u) in %u units\n", nx, ny, row0, block_w, cap, ix, iy,
                       (unsigned)seen[(size_t)iy * nx + ix]);
                return 1;
            }
    if (row0 >= ny && !units.empty()) {
        printf("grid %u x %u from row %u: %zu units for no rows\n", nx, ny, row0, units.size());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv) {
    for (uint32_t w = 0; w <= 12u; ++w) {
        const uint32_t eff = w < 1u ? 1u : (w > GATHER_WAVES_LIMIT ? GATHER_WAVES_LIMIT : w);
        const uint32_t cap = gather_queue_cap(w), tail = gather_tail_max(cap);
        if (cap == 0u || cap % 64u != 0u || cap > GATHER_QUEUE_CAP_MAX || eff * cap > GATHER_LDS_ENTRIES) {
            printf("%u waves: capacity %u\n", w, cap);
            return 1;
        }
        // (the largest such capacity, unless the 512 of the other gather kernels bounds it)
        if (cap < GATHER_QUEUE_CAP_MAX && eff * (cap + 64u) <= GATHER_LDS_ENTRIES) {
            printf("%u waves: capacity %u leaves room for 64 more per wave\n", w, cap);
            return 1;
        }
        if (tail == 0u || tail % 8u != 0u || tail > 48u || gather_tail_bytes(tail) > 8u * cap || gather_tail_bytes(tail + 8u) <= 8u * cap) {
            printf("%u waves: capacity %u, tail clamp %u (%u bytes of %u)\n", w, cap, tail, gather_tail_bytes(tail), 8u * cap);
            return 1;
        }
        if (gather_waves_fitting(w, cap) != eff || gather_queue_cap(gather_waves_fitting(GATHER_WAVES_LIMIT, cap)) < cap) {
            printf("%u waves: %u waves fit units of %u\n", w, gather_waves_fitting(w, cap), cap);
            return 1;
        }
        if (w >= 1u && w <= GATHER_WAVES_LIMIT) printf("cap %u %u %u\n", w, cap, tail);
    }
    int n_grids = 0;
    uint64_t n_units[GATHER_WAVES_LIMIT + 1] = {};   // units of the file's grids from their row0 on, blocks 32 wide (the shipped width)
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) {
            printf("cannot open %s\n", argv[1]);
            return 1;
        }
        unsigned nx, ny, row0;
        while (fscanf(f, "%u %u %u", &nx, &ny, &row0) == 3) {
            if (nx == 0u || ny == 0u || nx > 8192u || ny > 8192u) {
                printf("grid %u x %u: outside what this driver walks\n", nx, ny);
                fclose(f);
                return 1;
            }
            for (uint32_t w = 1; w <= GATHER_WAVES_LIMIT; ++w)
                for (uint32_t block_w : {0u, 1u, 16u, 32u, 48u, 64u, 300u, 512u})
                    for (uint32_t r : {0u, (uint32_t)row0})
                        if (check_grid(nx, ny, r, block_w, gather_queue_cap(w))) {
                            fclose(f);
                            return 1;
                        }
            for (uint32_t w = 1; w <= GATHER_WAVES_LIMIT; ++w)
                gather_cut_units(nx, ny, row0, 32u, gather_queue_cap(w), [&](uint32_t, uint32_t, uint32_t) { ++n_units[w]; });
            ++n_grids;
        }
        fclose(f);
        for (uint32_t w = 1; w <= GATHER_WAVES_LIMIT; ++w) printf("units %u %llu\n", w, (unsigned long long)n_units[w]);
    }
    printf("gather_queue_driver: OK (%d grids)\n", n_grids);
    return 0;
}
