// The squared sum of a window from the squared integral held MOD 2^32 (the u32 layout of the detect path).
// Four corners combined mod 2^32 give a rectangle's squared sum exactly as long as the true value is below 2^32, i.e. for
// rectangles of up to SQ32_MAX_AREA pixels.  A larger window of w <= SQ32_MAX_AREA columns is cut into horizontal strips of
// floor(SQ32_MAX_AREA / w) rows: each strip's sum is exact from the mod-2^32 image, and the strips add up in 64 bits to the exact
// value.  A strip's bottom corners are the next strip's top corners, so k strips cost 2 + 2 k loads.  Plain integer arithmetic
// without HIP, shared by the kernels (vj_kernels.hip), the host that gives every scale its strip height (vj_clod_plan.cpp) and a CPU
// test of its own (tests/sq_strips_driver.cpp).
#pragma once
#include <stdint.h>

namespace vj {

// 255^2 * 66051 < 2^32 <= 255^2 * 66052: the largest window area whose squared sum always fits a dword
constexpr uint32_t SQ32_MAX_AREA = 66051;
static_assert(65025ull * SQ32_MAX_AREA < (1ull << 32) && 65025ull * (SQ32_MAX_AREA + 1ull) >= (1ull << 32), "SQ32_MAX_AREA");

// Rows per strip of a window `w` columns wide, 1 <= w <= SQ32_MAX_AREA (0 for any other width: no strip height exists).
constexpr uint32_t sq_strip_rows(uint32_t w) { return w == 0u || w > SQ32_MAX_AREA ? 0u : SQ32_MAX_AREA / w; }
// Strips of a window of h rows: strip i is rows [i * rows, min((i + 1) * rows, h)).
constexpr uint32_t sq_strip_count(uint32_t h, uint32_t rows) { return (h + rows - 1u) / rows; }

// The exact squared sum of the window whose top-left corner is element `c0` of the mod-2^32 image, `dw` elements wide and
// `dh` = rows * pitch elements high, in strips of `strip` = sq_strip_rows(dw) * pitch elements; ld(i) returns element i.
// (constexpr like the functions above, so that the same template serves host and device code)
template <typename Ld>
constexpr uint64_t sq_window_strips(Ld ld, uint32_t c0, uint32_t dw, uint32_t dh, uint32_t strip) {
    uint64_t q = 0;
    if (strip == 0u) strip = dh;   // (never from the host's plans; keeps the walk finite whatever it is given)
    uint32_t top_l = ld(c0), top_r = ld(c0 + dw);
    for (uint32_t off = 0; off < dh;) {
        off += strip < dh - off ? strip : dh - off;
        const uint32_t bot_l = ld(c0 + off), bot_r = ld(c0 + off + dw);
        q += (uint32_t)(bot_r - bot_l - top_r + top_l);   // this strip: below 2^32, so exact mod 2^32
        top_l = bot_l;
        top_r = bot_r;
    }
    return q;
}

}  // namespace vj
