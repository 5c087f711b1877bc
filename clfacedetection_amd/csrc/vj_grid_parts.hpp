// The parts of the grid pass's (frame, unit) list (cascade_pass<FROM_GRID>, vj_kernels.hip): GRID_PARTS contiguous
// ranges, one ticket counter each, that the pass's waves draw their units from.  Plain integer arithmetic without HIP, shared by
// the kernel, the host code that lays the counters out (vj_detect_host.hpp) and a CPU test of its own (tests/grid_parts_driver.cpp);
// constexpr, so the same functions serve host and device code.
#pragma once
#include <stdint.h>

namespace vj {

constexpr uint32_t GRID_PARTS = 8;   // one per XCD: the waves of an XCD start on "their" part (its frames share that XCD's L2)

// Part x of a list of `total` items is [grid_part_begin(total, x), grid_part_begin(total, x + 1)), x in [0, GRID_PARTS): the
// parts are disjoint, ascending and cover [0, total) for every total (parts of a short list may be empty).
constexpr uint32_t grid_part_begin(uint32_t total, uint32_t x) {
    return (uint32_t)((unsigned long long)total * x / GRID_PARTS);
}
constexpr uint32_t grid_part_size(uint32_t total, uint32_t x) { return grid_part_begin(total, x + 1u) - grid_part_begin(total, x); }

// The part a workgroup starts on, and the part tried after part x is used up (all GRID_PARTS are visited in turn).
constexpr uint32_t grid_part_home(uint32_t block) { return block & (GRID_PARTS - 1u); }
constexpr uint32_t grid_part_next(uint32_t x) { return (x + 1u) & (GRID_PARTS - 1u); }
static_assert((GRID_PARTS & (GRID_PARTS - 1u)) == 0u, "GRID_PARTS is a power of two");

}  // namespace vj
