// The byte-moving half of the frame-processing calls: where the pieces of the block a slice uploads lie, the rows of
// host frames gathered into it at a 4-byte pitch, and — for the calls that paint in place — the spans copied back into the caller's
// memory.  No HIP and no vj_env: tests/stage_asan_driver.cpp runs all of it under AddressSanitizer.  vj_slice.hpp is the HIP half.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace vj {

inline size_t align4(size_t v) { return (v + 3u) & ~(size_t)3; }
inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

// The layout of a block, piece by piece; every call returns where its piece begins, `bytes` is the total so far.
struct StageBlock {
    size_t bytes = 0;
    // records, taps, lists: the next piece begins at a multiple of 16
    size_t section(size_t n) {
        const size_t at = bytes;
        bytes = at + align16(n);
        return at;
    }
    // n_rows rows at the pitch align4(row_bytes), the next piece right behind them (preprocess, extract, affine, yuv, atlas)
    size_t rows(size_t row_bytes, size_t n_rows) {
        const size_t at = bytes;
        bytes = at + align4(row_bytes) * n_rows;
        return at;
    }
    // ... the next piece at a multiple of 16 (paint, paint_yuv)
    size_t rows16(size_t row_bytes, size_t n_rows) {
        const size_t at = bytes;
        bytes = align16(at + align4(row_bytes) * n_rows);
        return at;
    }
};

// `rows` rows of row_bytes bytes, `stride` apart, to dst at `pitch`: no byte outside a row is read, no pad byte written
inline void gather_rows(uint8_t* dst, size_t pitch, const uint8_t* src, size_t stride, size_t rows, size_t row_bytes) {
    for (size_t y = 0; y < rows; ++y) memcpy(dst + y * pitch, src + y * stride, row_bytes);
}

// ... appended to the block `b` that begins at hs; returns where they lie
inline size_t stage_rows(uint8_t* hs, StageBlock* b, const uint8_t* src, size_t stride, size_t rows, size_t row_bytes) {
    const size_t at = b->rows(row_bytes, rows);
    gather_rows(hs + at, align4(row_bytes), src, stride, rows, row_bytes);
    return at;
}

// The inverse, for what was painted: bytes [x0, x0 + span) of rows [y0, y1) from a staged piece whose first row is row0 to the plane
// they came from.  Nothing outside those spans is written: never a row's padding, never a row outside the rectangle.
inline void scatter_span(uint8_t* dst, size_t stride, const uint8_t* src, size_t pitch, int32_t row0, int32_t y0, int32_t y1, size_t x0, size_t span) {
    for (int32_t y = y0; y < y1; ++y) memcpy(dst + (size_t)y * stride + x0, src + (size_t)(y - row0) * pitch + x0, span);
}

// A plane of a host frame (a gray / BGR frame is one plane, id 0) and, once touch_rows has run, the rows [y0, y1) the slice's
// records touch, where they lie in the block and at which pitch.
struct TouchedRows {
    int frame;
    uint32_t id;
    const uint8_t* p;
    size_t stride, row_bytes;
    int32_t rows;
    int32_t y0, y1;
    size_t at, pitch;
};
inline TouchedRows touched_plane(int frame, uint32_t id, const uint8_t* p, size_t stride, size_t row_bytes, int32_t rows) {
    return TouchedRows{frame, id, p, stride, row_bytes, rows, rows, 0, 0, align4(row_bytes)};
}

// What a record touches: bytes [x0, x0 + span) of rows [y0, y1) of plane (frame, id); piece: that plane's place in the list touch_rows
// leaves, -1 when it is not there (a device-resident plane)
struct RowSpan {
    int frame;
    uint32_t id;
    int32_t y0, y1;
    size_t x0, span;
    int piece;
};

// Of `planes`, those a span names stay, in their order, each with the rows its spans touch appended to `b`; the spans learn their piece.
inline void touch_rows(std::vector<TouchedRows>* planes, std::vector<RowSpan>* spans, StageBlock* b) {
    size_t kept = 0;
    for (RowSpan& r : *spans) r.piece = -1;
    for (TouchedRows s : *planes) {
        for (const RowSpan& r : *spans)
            if (r.frame == s.frame && r.id == s.id) {
                s.y0 = std::min(s.y0, r.y0);
                s.y1 = std::max(s.y1, r.y1);
            }
        if (s.y1 <= s.y0) continue;
        s.at = b->rows16(s.row_bytes, (size_t)(s.y1 - s.y0));
        for (RowSpan& r : *spans)
            if (r.frame == s.frame && r.id == s.id) r.piece = (int)kept;
        (*planes)[kept++] = s;
    }
    planes->resize(kept);
}

inline void gather_touched(uint8_t* hs, const std::vector<TouchedRows>& planes) {
    for (const TouchedRows& s : planes) gather_rows(hs + s.at, s.pitch, s.p + (size_t)s.y0 * s.stride, s.stride, (size_t)(s.y1 - s.y0), s.row_bytes);
}

inline void scatter_touched(const uint8_t* hs, const std::vector<TouchedRows>& planes, const std::vector<RowSpan>& spans) {
    for (const RowSpan& r : spans) {
        if (r.piece < 0) continue;
        const TouchedRows& s = planes[(size_t)r.piece];
        scatter_span(const_cast<uint8_t*>(s.p), s.stride, hs + s.at, s.pitch, s.y0, r.y0, r.y1, r.x0, r.span);
    }
}

}  // namespace vj
