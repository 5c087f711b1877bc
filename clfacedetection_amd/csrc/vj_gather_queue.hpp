// The LDS queues of the gather chain's linear kernels (cascade_pass without stage trees, vj_kernels.hip): one
// array of GATHER_LDS_ENTRIES entries per workgroup — the 16 KiB the tile classes leave free — divided among the waves the
// launch runs.  More waves get shorter queues out of the same array.  Plain integer arithmetic without HIP, shared by the kernel,
// the host code that cuts the first-pass units and clamps the tunables (vj_clod_plan.cpp, vj_detect.cpp) and a CPU test of its own
// (tests/gather_queue_driver.cpp); constexpr, so the same functions serve host and device code.
#pragma once
#include <stdint.h>

namespace vj {

constexpr uint32_t GATHER_LDS_ENTRIES = 2048;     // 8-byte entries: 16 KiB
constexpr uint32_t GATHER_QUEUE_CAP_MAX = 512;    // == UNIT_WINDOWS: what a wave's queue holds in every other gather kernel
constexpr uint32_t GATHER_WAVES_LIMIT = 8;        // == GATHER_WAVES_MAX

// Entries per wave of a launch with `waves` waves per workgroup: whole 64-lane groups, 512 for up to 4 waves, 384 for 5, 320 for
// 6, 256 for 7 and 8.  waves * cap <= GATHER_LDS_ENTRIES.
constexpr uint32_t gather_queue_cap(uint32_t waves) {
    const uint32_t w = waves < 1u ? 1u : (waves > GATHER_WAVES_LIMIT ? GATHER_WAVES_LIMIT : waves);
    const uint32_t cap = 64u * (GATHER_LDS_ENTRIES / (64u * w));
    return cap < GATHER_QUEUE_CAP_MAX ? cap : GATHER_QUEUE_CAP_MAX;
}

// The stump-parallel tail (sweep_tail_stump_parallel) keeps its scratch inside the wave's own queue: T entries, and behind
// them T x GATHER_TAIL_BLOCKS verdict words of 8 bytes — 80 T bytes.  The most windows it may take at a capacity, in steps of
// 8 and at most 48: 48 at 512 entries, 32 at 384 and 320, 24 at 256.  The verdict words start behind that many entries.
constexpr uint32_t GATHER_TAIL_BLOCKS = 9;        // blocks of 64 stumps per stage at most (== SP_TAIL_MAX_BLOCKS)
constexpr uint32_t gather_tail_bytes(uint32_t windows) { return windows * (8u + GATHER_TAIL_BLOCKS * 8u); }
constexpr uint32_t gather_tail_max(uint32_t cap) {
    const uint32_t t = cap * 8u / gather_tail_bytes(8u) * 8u;
    return t < 48u ? t : 48u;
}
static_assert(gather_queue_cap(1) == 512 && gather_queue_cap(4) == 512 && gather_queue_cap(5) == 384 && gather_queue_cap(6) == 320 &&
                  gather_queue_cap(7) == 256 && gather_queue_cap(8) == 256, "the capacities DESIGN.md §4.2 lists");
static_assert(gather_tail_max(512) == 48 && gather_tail_max(384) == 32 && gather_tail_max(320) == 32 && gather_tail_max(256) == 24,
              "the tail clamps DESIGN.md §7 lists");
static_assert(gather_tail_bytes(gather_tail_max(512)) <= 512 * 8 && gather_tail_bytes(gather_tail_max(384)) <= 384 * 8 &&
                  gather_tail_bytes(gather_tail_max(320)) <= 320 * 8 && gather_tail_bytes(gather_tail_max(256)) <= 256 * 8,
              "the tail's entries and verdict words fit the wave's queue at every capacity");

// The most waves per workgroup whose queues still hold a unit of `unit_cap` windows (a plan cut for more waves may be run by
// fewer, never the other way round).
constexpr uint32_t gather_waves_fitting(uint32_t waves, uint32_t unit_cap) {
    uint32_t w = waves < 1u ? 1u : (waves > GATHER_WAVES_LIMIT ? GATHER_WAVES_LIMIT : waves);
    while (w > 1u && gather_queue_cap(w) < unit_cap) --w;
    return w;
}

// First-pass units of one scale's grid (nx x ny windows, rows from row0 on: the tiles keep the rows above): 2-D blocks of
// block_w x floor(cap / block_w) windows when block_w > 0 and the grid's indices fit 16 bits — emit(ix0 | iy0 << 16, bw * bh, bw);
// blocks at the right and lower edges reach past the grid, the grid pass clips them — else row-major runs of cap windows,
// emit(first, count, 0).  Every unit holds at most `cap` windows.
template <typename Emit>
inline void gather_cut_units(uint32_t nx, uint32_t ny, uint32_t row0, uint32_t block_w, uint32_t cap, Emit emit) {
    if (row0 >= ny) return;
    if (block_w > 0u && nx < 65536u && ny < 65536u) {
        uint32_t bw = block_w < nx ? block_w : nx;
        if (bw > cap) bw = cap;
        uint32_t bh = cap / bw < ny ? cap / bw : ny;
        if (bh < 1u) bh = 1u;
        for (uint32_t iy0 = row0; iy0 < ny; iy0 += bh)
            for (uint32_t ix0 = 0; ix0 < nx; ix0 += bw) emit(ix0 | (iy0 << 16), bw * bh, bw);
    } else {
        const uint32_t nwin = nx * ny;
        for (uint32_t f = row0 * nx; f < nwin; f += cap) emit(f, cap < nwin - f ? cap : nwin - f, 0u);
    }
}

}  // namespace vj
