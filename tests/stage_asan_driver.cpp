// Sanitizer driver of the byte-moving half of the frame-processing calls (csrc/vj_stage_host.hpp): built by
// tests/test_sanitizers_stage.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/stage_asan_driver.cpp
// (no HIP involved; the header is all there is to link).  Every source and destination lies in a heap block of its exact size, so
// that ASan sees a byte read or written outside it.  Against restatements written out here:
//  - the block layout: record counts 0, 1 and 5, pieces of 1, 3, 4, 5 and 131 row bytes with 1, 2 and 7 rows, packed and with every
//    piece's end rounded up to 16: the offsets are the formulas the drivers spelled out before the builder, pieces never overlap,
//    the total is the last end;
//  - gather_rows: strides equal to, one above and 13 above the row bytes, sources at every address mod 4: the rows arrive, the
//    destination's pad bytes keep their canary;
//  - scatter_span: only [x0, x0 + span) x [y0, y1) of a canary-filled strided destination changes;
//  - touch_rows, gather_touched, scatter_touched on frames of one plane and of three: the touched rows are the brute-force min / max
//    over the records, a plane no record names is not staged, overlapping records of one plane write their union and nothing else.
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../clfacedetection_amd/csrc/vj_stage_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static const size_t ROW_BYTES[] = {1, 3, 4, 5, 131};
static const size_t ROWS[] = {1, 2, 7};
static const uint8_t CANARY = 0xA5;

// a heap block of exactly `bytes` bytes
struct Block {
    std::unique_ptr<uint8_t[]> mem;
    size_t bytes;
    explicit Block(size_t n, int fill = -1) : mem(new uint8_t[n ? n : 1]), bytes(n) {
        for (size_t i = 0; i < n; ++i) mem[i] = fill >= 0 ? (uint8_t)fill : (uint8_t)(i * 7u + 1u);
    }
    uint8_t* p() { return mem.get(); }
};

static void test_layout() {
    const size_t rec_size = 40, tap_size = 12;
    for (size_t n_recs : {(size_t)0, (size_t)1, (size_t)5})
        for (int round16 = 0; round16 < 2; ++round16) {
            StageBlock b;
            // the head as the drivers wrote it: rec_bytes = align16(n * sizeof(record)), then the taps
            const size_t rec_bytes = (n_recs * rec_size + 15u) / 16u * 16u, tap_bytes = (3u * tap_size + 15u) / 16u * 16u;
            CHECK(b.section(n_recs * rec_size) == 0);
            CHECK(b.section(3u * tap_size) == rec_bytes);
            CHECK(b.bytes == rec_bytes + tap_bytes);
            size_t running = rec_bytes + tap_bytes, last_end = running;
            for (size_t rb : ROW_BYTES)
                for (size_t rows : ROWS) {
                    const size_t pitch = (rb + 3u) / 4u * 4u;
                    const size_t at = round16 ? b.rows16(rb, rows) : b.rows(rb, rows);
                    CHECK(at == running);         // (a piece begins where the one before it ended: never inside it)
                    CHECK(at >= last_end);
                    last_end = at + pitch * rows;
                    running = round16 ? (last_end + 15u) / 16u * 16u : last_end;
                    CHECK(b.bytes == running);
                    if (round16) CHECK(at % 16u == 0 && b.bytes % 16u == 0);
                    else CHECK(at % 4u == 0);
                }
            CHECK(b.bytes >= last_end && b.bytes - last_end < 16u);
            if (!round16) CHECK(b.bytes == last_end);
        }
    CHECK(align4(0) == 0 && align4(1) == 4 && align4(4) == 4 && align4(5) == 8 && align16(0) == 0 && align16(1) == 16 && align16(16) == 16 && align16(17) == 32);
}

static void test_gather() {
    for (size_t rb : ROW_BYTES)
        for (size_t rows : ROWS)
            for (size_t extra : {(size_t)0, (size_t)1, (size_t)13})
                for (size_t off = 0; off < 4; ++off)
                    for (size_t pitch : {align4(rb), align4(rb) + 4u}) {
                        const size_t stride = rb + extra;
                        Block src(off + (rows - 1) * stride + rb);                 // ends with the last row's last byte
                        Block dst(rows * pitch - (pitch - rb), CANARY);           // ... and so does the destination
                        gather_rows(dst.p(), pitch, src.p() + off, stride, rows, rb);
                        for (size_t y = 0; y < rows; ++y)
                            for (size_t x = 0; x < pitch && y * pitch + x < dst.bytes; ++x)
                                CHECK(dst.p()[y * pitch + x] == (x < rb ? src.p()[off + y * stride + x] : CANARY));
                        // stage_rows: the same rows at the pitch align4(rb), where the builder says
                        StageBlock b;
                        b.section(5);
                        Block hs(16 + rows * align4(rb), CANARY);
                        const size_t at = stage_rows(hs.p(), &b, src.p() + off, stride, rows, rb);
                        CHECK(at == 16 && b.bytes == hs.bytes);
                        for (size_t i = 0; i < hs.bytes; ++i) {
                            const size_t y = i < 16 ? rows : (i - 16) / align4(rb), x = i < 16 ? 0 : (i - 16) % align4(rb);
                            CHECK(hs.p()[i] == (y < rows && x < rb ? src.p()[off + y * stride + x] : CANARY));
                        }
                    }
}

// scatter_span of one span; the destination is rows x row_bytes at `stride`, the staged piece begins with row `row0`
static void one_scatter(size_t rb, int32_t rows, size_t stride, int32_t row0, int32_t y0, int32_t y1, size_t x0, size_t span) {
    const size_t pitch = align4(rb);
    Block dst((size_t)(rows - 1) * stride + rb, CANARY);
    Block staged((size_t)(rows - row0) * pitch - (pitch - rb));
    scatter_span(dst.p(), stride, staged.p(), pitch, row0, y0, y1, x0, span);
    for (size_t i = 0; i < dst.bytes; ++i) {
        const size_t y = i / stride, x = i % stride;
        const bool in = (int32_t)y >= y0 && (int32_t)y < y1 && x >= x0 && x < x0 + span;
        CHECK(dst.p()[i] == (in ? staged.p()[(y - (size_t)row0) * pitch + x] : CANARY));
    }
}

static void test_scatter() {
    for (size_t rb : {(size_t)5, (size_t)131})
        for (size_t extra : {(size_t)0, (size_t)1, (size_t)13}) {
            const size_t stride = rb + extra;
            one_scatter(rb, 7, stride, 0, 0, 7, 0, rb);             // the whole plane
            one_scatter(rb, 7, stride, 2, 2, 5, 0, 3);              // a span at column 0
            one_scatter(rb, 7, stride, 2, 2, 7, rb - 2, 2);         // ... ending at the last column, in the last row
            one_scatter(rb, 7, stride, 6, 6, 7, rb - 1, 1);         // one row, one byte, the block's last
            one_scatter(rb, 7, stride, 0, 0, 1, 0, 1);              // ... its first
            one_scatter(rb, 7, stride, 1, 3, 4, 1, rb - 2);         // row0 < y0: the piece begins above the span
            one_scatter(rb, 7, stride, 0, 5, 6, 2, 1);
            one_scatter(rb, 7, stride, 3, 4, 4, 0, rb);             // no row
        }
}

// frames of `n_planes` planes each; plane q of frame f is rows[q] x rb[q]
struct Rec { int frame; uint32_t id; int32_t x0, x1, y0, y1; };

static void one_touch(int n_frames, uint32_t n_planes, const std::vector<Rec>& recs, int device_frame) {
    const size_t rb[3] = {37 * (n_planes == 1 ? 3u : 1u), 19, 18}, rows[3] = {23, 11, 11};
    std::vector<Block> mem, orig;
    std::vector<size_t> strides;
    std::vector<TouchedRows> planes;
    for (int f = 0; f < n_frames; ++f)
        for (uint32_t q = 0; q < n_planes; ++q) {
            const size_t stride = rb[q] + (size_t)((f + (int)q) % 3) * 5u, off = (size_t)((f + (int)q) % 4);
            mem.emplace_back(off + (rows[q] - 1) * stride + rb[q]);
            orig.emplace_back(mem.back().bytes);
            strides.push_back(stride);
            if (f != device_frame) planes.push_back(touched_plane(f, q, mem.back().p() + off, stride, rb[q], (int32_t)rows[q]));
        }
    std::vector<RowSpan> spans;
    for (const Rec& r : recs) spans.push_back(RowSpan{r.frame, r.id, r.y0, r.y1, (size_t)r.x0, (size_t)(r.x1 - r.x0), 7});
    StageBlock b;
    b.section(recs.size() * 40u);
    const size_t head = b.bytes;
    touch_rows(&planes, &spans, &b);
    // the brute-force statement: per plane of a host frame, min / max over the records that name it; in the planes' order
    size_t at = head, k = 0;
    for (int f = 0; f < n_frames; ++f)
        for (uint32_t q = 0; q < n_planes; ++q) {
            int32_t y0 = (int32_t)rows[q], y1 = 0;
            for (const Rec& r : recs)
                if (r.frame == f && r.id == q) y0 = std::min(y0, r.y0), y1 = std::max(y1, r.y1);
            if (f == device_frame || y1 <= y0) {
                for (size_t i = 0; i < recs.size(); ++i)
                    if (recs[i].frame == f && recs[i].id == q) CHECK(spans[i].piece == -1);
                continue;
            }
            CHECK(k < planes.size());
            const TouchedRows& s = planes[k];
            CHECK(s.frame == f && s.id == q && s.y0 == y0 && s.y1 == y1 && s.at == at && s.pitch == (rb[q] + 3u) / 4u * 4u && s.row_bytes == rb[q]);
            at = (at + s.pitch * (size_t)(y1 - y0) + 15u) / 16u * 16u;
            for (size_t i = 0; i < recs.size(); ++i)
                if (recs[i].frame == f && recs[i].id == q) CHECK(spans[i].piece == (int)k);
            ++k;
        }
    CHECK(k == planes.size() && b.bytes == at);
    // the round trip: what was gathered is the touched rows; painted in the block, only the records' spans come back
    Block hs(b.bytes, CANARY);
    gather_touched(hs.p(), planes);
    for (const TouchedRows& s : planes)
        for (int32_t y = s.y0; y < s.y1; ++y)
            for (size_t x = 0; x < s.pitch; ++x)
                CHECK(hs.p()[s.at + (size_t)(y - s.y0) * s.pitch + x] == (x < s.row_bytes ? s.p[(size_t)y * s.stride + x] : CANARY));
    for (size_t i = head; i < hs.bytes; ++i) hs.p()[i] = (uint8_t)~hs.p()[i];
    scatter_touched(hs.p(), planes, spans);
    for (int f = 0; f < n_frames; ++f)
        for (uint32_t q = 0; q < n_planes; ++q) {
            const size_t m = (size_t)f * n_planes + q, stride = strides[m], off = (size_t)((f + (int)q) % 4);
            for (size_t i = 0; i < mem[m].bytes; ++i) {
                bool in = false;
                if (i >= off && f != device_frame) {
                    const size_t y = (i - off) / stride, x = (i - off) % stride;
                    for (const Rec& r : recs)
                        in = in || (r.frame == f && r.id == q && (int32_t)y >= r.y0 && (int32_t)y < r.y1 && (int32_t)x >= r.x0 && (int32_t)x < r.x1);
                }
                CHECK(mem[m].p()[i] == (in ? (uint8_t)~orig[m].p()[i] : orig[m].p()[i]));
            }
        }
}

static void test_touch() {
    // one plane per frame (BGR: 37 x 23 x 3): frame 1 named by no record, frame 2 by overlapping ones, frame 3 device-resident
    one_touch(4, 1, {{0, 0, 0, 111, 0, 23}, {2, 0, 3, 30, 4, 9}, {2, 0, 12, 60, 6, 15}, {2, 0, 110, 111, 22, 23}, {3, 0, 0, 9, 0, 3}}, 3);
    one_touch(1, 1, {{0, 0, 0, 1, 0, 1}}, -1);
    one_touch(2, 1, {}, -1);
    // three planes per frame: a chroma plane no record names, records of several planes in any order, an empty record
    one_touch(3, 3, {{0, 0, 2, 20, 3, 12}, {0, 1, 1, 10, 1, 6}, {0, 2, 1, 10, 1, 6}, {2, 1, 0, 19, 0, 11}, {2, 0, 0, 37, 0, 23}, {2, 0, 5, 9, 20, 23},
                     {1, 2, 4, 4, 5, 5}},
              -1);
    one_touch(2, 3, {{1, 0, 36, 37, 22, 23}, {1, 1, 18, 19, 10, 11}, {0, 0, 0, 37, 11, 12}}, 0);
}

int main() {
    test_layout();
    test_gather();
    test_scatter();
    test_touch();
    printf("stage_asan_driver: OK\n");
    return 0;
}
