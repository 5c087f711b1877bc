// Sanitizer driver of the host planner of vj_yuv_to_bgr / vj_bgr_to_yuv (csrc/vj_yuv_host.cpp: the argument checks, the layouts, the
// frame records of a slice): built by tests/test_sanitizers_yuv.py with
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -DVJ_BUILDING
//       tests/yuv_asan_driver.cpp csrc/vj_yuv_host.cpp csrc/vj_cascade.cpp csrc/vj_group.cpp
// (no HIP involved).  All layouts, both channel counts, widths 2 .. 10 and 254 .. 258, heights 2, 4, 6, whole calls and slices of 1, 2
// and 3 frames: the work units — decoded as the kernels of csrc/vj_yuv.hip decode them: a binary search of the unit prefix, then
// block, wave, lane and row pair -> the stores of a lane — cover every byte of every output plane and every pad byte exactly once,
// nothing outside them, and read only inside the source planes; then the error cases.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../clfacedetection_amd/csrc/vj_yuv_host.hpp"

using namespace vj;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static uint8_t px[64];

struct Size { int w, h; };
static std::vector<Size> sizes_of_the_cases() {
    std::vector<Size> s;
    for (int h : {2, 4, 6}) {
        for (int w = 2; w <= 10; w += 2) s.push_back(Size{w, h});
        for (int w = 254; w <= 258; w += 2) s.push_back(Size{w, h});
    }
    s.push_back(Size{514, 66});   // more than one block each way
    return s;
}

// what a lane touches: [at, at + len) of the destination, or of a source plane
struct Cover {
    std::vector<uint8_t> hit;
    explicit Cover(uint64_t bytes) : hit((size_t)bytes, 0) {}
    void store(uint64_t at, uint64_t len, uint64_t align) {
        CHECK(at % align == 0u && at + len <= hit.size());
        for (uint64_t k = 0; k < len; ++k) {
            CHECK(hit[(size_t)(at + k)] == 0);   // no byte twice
            hit[(size_t)(at + k)] = 1;
        }
    }
};
// a load of bytes [x0, x0 + len) of row `row` of a plane of `rows` rows of row_bytes bytes
static void load(uint64_t row, uint64_t rows, uint64_t x0, uint64_t len, uint64_t row_bytes) { CHECK(row < rows && x0 + len <= row_bytes); }

template <typename Visit>
static void for_each_lane(const YuvSlice& sl, size_t m, Visit visit) {
    for (uint32_t u0 = 0; u0 < sl.n_units; ++u0) {
        uint32_t lo = 0, hi = (uint32_t)m;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (sl.recs[mid].unit_first <= u0) lo = mid;
            else hi = mid;
        }
        const YuvFrameDev& d = sl.recs[lo];
        const uint32_t bpr = (d.width + YUV_BLOCK_W - 1u) / YUV_BLOCK_W, u = u0 - d.unit_first;
        const uint32_t by = u / bpr, bx = u - by * bpr;
        CHECK(by * YUV_BLOCK_H < d.height && bx * YUV_BLOCK_W < d.width);   // no empty unit
        for (uint32_t tid = 0; tid < 256u; ++tid) {
            const uint32_t x = bx * YUV_BLOCK_W + (tid & 63u) * YUV_LANE_W;
            if (x >= d.width) continue;
            const uint32_t n = std::min(YUV_LANE_W, d.width - x);
            CHECK(n == 4u || n == 2u);
            for (uint32_t y = by * YUV_BLOCK_H + 2u * (tid >> 6); y < std::min((by + 1u) * YUV_BLOCK_H, d.height); y += 2u * YUV_WAVES) visit(d, x, y, n);
        }
    }
}

// ---- decode: the layout through the C entry point and through the planner, then every slice of `per_slice` frames
static void plan_decode(const std::vector<vj_yuv_image>& frames, int channels, size_t per_slice) {
    const int n = (int)frames.size();
    vj_yuv_params p;
    memset(&p, 0xff, sizeof(p));
    vj_yuv_default(&p);
    CHECK(p.channels == 3 && p.flags == 0u && p.reserved == 0u);
    p.channels = channels;
    p.flags = VJ_YUV_RGB_ORDER;
    std::vector<vj_image> out((size_t)n);
    uint64_t bytes = 1;
    CHECK(vj_yuv_to_bgr_layout(frames.data(), n, &p, out.data(), &bytes) == VJ_OK);
    YuvLayout lay;
    CHECK(yuv_decode_layout(frames.data(), n, &p, &lay) == VJ_OK && lay.bytes == bytes && lay.slots.size() == (size_t)n && lay.swap_rb);
    uint64_t end = 0;
    for (int i = 0; i < n; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        const vj_image& o = out[(size_t)i];
        CHECK((uint64_t)(uintptr_t)o.data == t.off && o.width == frames[(size_t)i].width && o.height == frames[(size_t)i].height && o.stride == (int)t.pitch);
        CHECK(o.on_device == 1 && o.channels == channels && t.pitch == yuv_align4(t.w * (uint32_t)channels));
        CHECK(t.off % 256u == 0u && t.off >= end && t.off - end < 256u);
        end = t.off + (uint64_t)t.pitch * t.h;
    }
    CHECK(end == bytes);
    Cover dst(bytes);
    YuvSlice sl;
    const uint32_t CH = (uint32_t)channels;
    for (size_t first = 0; first < (size_t)n; first += per_slice) {
        const size_t m = std::min(per_slice, (size_t)n - first);
        CHECK(yuv_decode_plan_slice(frames.data(), lay, first, m, &sl) == VJ_OK && sl.recs.size() == m);
        uint64_t unit = 0;
        for (size_t i = 0; i < m; ++i) {
            const YuvFrameDev& d = sl.recs[i];
            const vj_yuv_image& f = frames[first + i];
            CHECK(d.y == f.y && d.c0 == f.c0 && d.y_stride == (uint32_t)f.y_stride && d.c_stride == (uint32_t)f.c_stride && d.layout == (uint32_t)f.layout);
            CHECK(d.width == (uint32_t)f.width && d.height == (uint32_t)f.height && d.channels == CH && d.unit_first == unit);
            CHECK(d.dst_off == lay.slots[first + i].off && d.pitch == lay.slots[first + i].pitch);
            unit += yuv_units(d.width, d.height);
        }
        CHECK(unit == sl.n_units);
        for_each_lane(sl, m, [&](const YuvFrameDev& d, uint32_t x, uint32_t y, uint32_t nn) {
            // loads: n bytes of Y rows y, y + 1; n bytes of the pair row y / 2, or n / 2 of each I420 plane
            load(y, d.height, x, nn, d.width);
            load(y + 1u, d.height, x, nn, d.width);
            if (d.layout == YUV_I420) load(y >> 1, d.height / 2u, x >> 1, nn / 2u, d.width / 2u);
            else load(y >> 1, d.height / 2u, x, nn, d.width);
            // stores: per row 12 or 16 bytes; the 2-pixel lane 8 bytes — BGR: its 6 bytes and the row's 2 pad bytes
            const uint64_t len = nn == 4u ? 4u * CH : 8u;
            for (uint32_t r = 0; r < 2u; ++r) dst.store(d.dst_off + (uint64_t)(y + r) * d.pitch + (uint64_t)x * CH, len, 4u);
        });
    }
    for (int i = 0; i < n; ++i) {   // every byte of every row of every image, pad bytes included, once; nothing between the images
        const YuvSlot& t = lay.slots[(size_t)i];
        for (uint64_t b = 0; b < (uint64_t)t.pitch * t.h; ++b) CHECK(dst.hit[(size_t)(t.off + b)] == 1);
        const uint64_t next = i + 1 < n ? lay.slots[(size_t)i + 1].off : bytes;
        for (uint64_t b = t.off + (uint64_t)t.pitch * t.h; b < next; ++b) CHECK(dst.hit[(size_t)b] == 0);
    }
}

// ---- encode
static void plan_encode(const std::vector<vj_image>& frames, int layout, size_t per_slice) {
    const int n = (int)frames.size();
    vj_yuv_params p;
    vj_yuv_default(&p);
    std::vector<vj_yuv_image> out((size_t)n);
    uint64_t bytes = 1;
    CHECK(vj_bgr_to_yuv_layout(frames.data(), n, &p, layout, out.data(), &bytes) == VJ_OK);
    YuvLayout lay;
    CHECK(yuv_encode_layout(frames.data(), n, &p, layout, &lay) == VJ_OK && lay.bytes == bytes && lay.slots.size() == (size_t)n && !lay.swap_rb);
    const uint32_t L = (uint32_t)layout;
    uint64_t end = 0;
    for (int i = 0; i < n; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        const vj_yuv_image& o = out[(size_t)i];
        CHECK((uint64_t)(uintptr_t)o.y == t.off && t.off % 256u == 0u && t.off >= end && t.off - end < 256u);
        CHECK(o.width == frames[(size_t)i].width && o.height == frames[(size_t)i].height && o.layout == layout && o.on_device == 1);
        CHECK(o.y_stride == (int)yuv_align4(t.w) && (uint64_t)(uintptr_t)o.c0 == t.off + (uint64_t)o.y_stride * t.h);
        CHECK(o.c_stride == (int)yuv_align4(L == YUV_I420 ? t.w / 2u : t.w));
        if (L == YUV_I420) CHECK((uint64_t)(uintptr_t)o.c1 == (uint64_t)(uintptr_t)o.c0 + (uint64_t)o.c_stride * (t.h / 2u));
        else CHECK(o.c1 == nullptr);
        end = t.off + yuv_frame_bytes(L, t.w, t.h);
        CHECK(end == (uint64_t)(uintptr_t)o.c0 + (uint64_t)o.c_stride * (t.h / 2u) * (L == YUV_I420 ? 2u : 1u));
    }
    CHECK(end == bytes);
    Cover dst(bytes);
    YuvSlice sl;
    for (size_t first = 0; first < (size_t)n; first += per_slice) {
        const size_t m = std::min(per_slice, (size_t)n - first);
        CHECK(yuv_encode_plan_slice(frames.data(), lay, first, m, &sl) == VJ_OK && sl.recs.size() == m);
        uint64_t unit = 0;
        for (size_t i = 0; i < m; ++i) {
            const YuvFrameDev& d = sl.recs[i];
            const vj_image& f = frames[first + i];
            CHECK(d.y == f.data && d.y_stride == (uint32_t)f.stride && d.channels == (uint32_t)f.channels && d.layout == L && d.unit_first == unit);
            CHECK(d.width == (uint32_t)f.width && d.height == (uint32_t)f.height && d.dst_off == lay.slots[first + i].off && d.pitch == yuv_align4(d.width));
            unit += yuv_units(d.width, d.height);
        }
        CHECK(unit == sl.n_units);
        for_each_lane(sl, m, [&](const YuvFrameDev& d, uint32_t x, uint32_t y, uint32_t nn) {
            load(y, d.height, (uint64_t)x * d.channels, (uint64_t)nn * d.channels, (uint64_t)d.width * d.channels);
            load(y + 1u, d.height, (uint64_t)x * d.channels, (uint64_t)nn * d.channels, (uint64_t)d.width * d.channels);
            // stores: a dword of Y per row (the 2-pixel lane: with the row's two pad bytes) ...
            for (uint32_t r = 0; r < 2u; ++r) dst.store(d.dst_off + (uint64_t)(y + r) * d.pitch + x, 4u, 4u);
            const uint32_t cp = yuv_plane_pitch(L, d.width, 1u);
            const uint64_t crow = (uint64_t)(y >> 1) * cp;
            if (L != YUV_I420) {   // ... a dword of pairs ...
                dst.store(d.dst_off + yuv_plane_off(L, d.width, d.height, 1u) + crow + x, 4u, 4u);
            } else {               // ... or two bytes per plane and, from the row's last lane, the pad bytes left before the pitch
                const bool row_end = x + YUV_LANE_W >= d.width && (x >> 1) + 2u < cp;
                for (uint32_t pl = 1; pl <= 2u; ++pl) {
                    const uint64_t at = d.dst_off + yuv_plane_off(L, d.width, d.height, pl) + crow + (x >> 1);
                    dst.store(at, 2u, 2u);
                    if (row_end) dst.store(at + 2u, 2u, 2u);
                }
            }
        });
    }
    for (int i = 0; i < n; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        const uint64_t fb = yuv_frame_bytes(L, t.w, t.h);
        for (uint64_t b = 0; b < fb; ++b) CHECK(dst.hit[(size_t)(t.off + b)] == 1);
        const uint64_t next = i + 1 < n ? lay.slots[(size_t)i + 1].off : bytes;
        for (uint64_t b = t.off + fb; b < next; ++b) CHECK(dst.hit[(size_t)b] == 0);
    }
}

int main() {
    const std::vector<Size> sizes = sizes_of_the_cases();
    // ---- every layout, both channel counts; whole calls and slices of 1, 2 and 3 frames; sources at padded strides
    for (int layout : {VJ_YUV_NV12, VJ_YUV_NV21, VJ_YUV_I420}) {
        std::vector<vj_yuv_image> yf;
        std::vector<vj_image> b3, b4, mixed;
        for (size_t i = 0; i < sizes.size(); ++i) {
            const int w = sizes[i].w, h = sizes[i].h, crow = layout == VJ_YUV_I420 ? w / 2 : w;
            yf.push_back(vj_yuv_image{px, px, px, w, h, w + (int)(i % 3), crow + (int)(i % 2) * 5, layout, (int)(i % 2)});
            b3.push_back(vj_image{px, w, h, w * 3 + (int)(i % 4), 0, 3});
            b4.push_back(vj_image{px, w, h, w * 4 + (int)(i % 3), (int)(i % 2), 4});
            mixed.push_back(i % 2 ? b3.back() : b4.back());
        }
        for (size_t per : {sizes.size(), (size_t)1, (size_t)2, (size_t)3}) {
            plan_decode(yf, 3, per);
            plan_decode(yf, 4, per);
            plan_encode(b3, layout, per);
            plan_encode(b4, layout, per);
            plan_encode(mixed, layout, per);
        }
    }
    {   // the layouts mixed in one call
        std::vector<vj_yuv_image> yf;
        for (size_t i = 0; i < sizes.size(); ++i) yf.push_back(vj_yuv_image{px, px, px, sizes[i].w, sizes[i].h, sizes[i].w, sizes[i].w, (int)(i % 3), 0});
        plan_decode(yf, 3, yf.size());
        plan_decode(yf, 4, 2);
    }
    {   // no frames
        vj_yuv_params p;
        vj_yuv_default(&p);
        uint64_t bytes = 5;
        CHECK(vj_yuv_to_bgr_layout(nullptr, 0, &p, nullptr, &bytes) == VJ_OK && bytes == 0);
        bytes = 5;
        CHECK(vj_bgr_to_yuv_layout(nullptr, 0, &p, VJ_YUV_I420, nullptr, &bytes) == VJ_OK && bytes == 0);
        vj_yuv_default(nullptr);
    }

    // ---- the error cases
    vj_yuv_params ok;
    vj_yuv_default(&ok);
    vj_image out[4];
    vj_yuv_image yout[4];
    uint64_t bytes = 0;
    const vj_yuv_image good = {px, px, px, 8, 4, 8, 8, VJ_YUV_NV12, 0};
    const vj_image goodb = {px, 8, 4, 24, 0, 3};
    CHECK(vj_yuv_to_bgr_layout(nullptr, 1, &ok, out, &bytes) == VJ_ERR_ARG);
    CHECK(vj_yuv_to_bgr_layout(&good, 1, nullptr, out, &bytes) == VJ_ERR_ARG);
    CHECK(vj_yuv_to_bgr_layout(&good, 1, &ok, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_yuv_to_bgr_layout(&good, 1, &ok, out, nullptr) == VJ_ERR_ARG);
    CHECK(vj_yuv_to_bgr_layout(&good, -1, &ok, out, &bytes) == VJ_ERR_ARG);
    CHECK(vj_bgr_to_yuv_layout(nullptr, 1, &ok, 0, yout, &bytes) == VJ_ERR_ARG);
    CHECK(vj_bgr_to_yuv_layout(&goodb, 1, nullptr, 0, yout, &bytes) == VJ_ERR_ARG);
    CHECK(vj_bgr_to_yuv_layout(&goodb, 1, &ok, 0, nullptr, &bytes) == VJ_ERR_ARG);
    CHECK(vj_bgr_to_yuv_layout(&goodb, 1, &ok, 0, yout, nullptr) == VJ_ERR_ARG);
    CHECK(vj_bgr_to_yuv_layout(&goodb, 1, &ok, 3, yout, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), "layout") != nullptr);
    struct { vj_yuv_image f; int rc; const char* word; } bad[] = {
        {{nullptr, px, px, 8, 4, 8, 8, 0, 0}, VJ_ERR_ARG, "null y"}, {{px, nullptr, px, 8, 4, 8, 8, 1, 0}, VJ_ERR_ARG, "null c0"},
        {{px, px, nullptr, 8, 4, 8, 4, 2, 0}, VJ_ERR_ARG, "null c1"}, {{px, px, px, 7, 4, 8, 8, 0, 0}, VJ_ERR_ARG, "even"},
        {{px, px, px, 8, 5, 8, 8, 0, 0}, VJ_ERR_ARG, "even"}, {{px, px, px, 0, 4, 8, 8, 0, 0}, VJ_ERR_ARG, "positive"},
        {{px, px, px, 8, 4, 7, 8, 0, 0}, VJ_ERR_ARG, "y_stride"}, {{px, px, px, 8, 4, 8, 7, 0, 0}, VJ_ERR_ARG, "c_stride"},
        {{px, px, px, 8, 4, 8, 3, 2, 0}, VJ_ERR_ARG, "c_stride"}, {{px, px, px, 8, 4, 8, 8, 3, 0}, VJ_ERR_ARG, "layout"},
        {{px, px, px, 65536, 4, 65536, 65536, 0, 0}, VJ_ERR_LIMIT, "65534"}, {{px, px, px, 8, 65535, 8, 8, 0, 0}, VJ_ERR_LIMIT, "65534"}};
    for (const auto& b : bad) {
        const vj_yuv_image v[3] = {good, good, b.f};
        bytes = 9;
        CHECK(vj_yuv_to_bgr_layout(v, 3, &ok, out, &bytes) == b.rc && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr && strstr(vj_last_error(), b.word) != nullptr);
    }
    struct { vj_image f; int rc; const char* word; } badb[] = {
        {{nullptr, 8, 4, 24, 0, 3}, VJ_ERR_ARG, "null data"}, {{px, 8, 4, 8, 0, 1}, VJ_ERR_ARG, "gray"}, {{px, 8, 4, 16, 0, 2}, VJ_ERR_ARG, "channels"},
        {{px, 7, 4, 24, 0, 3}, VJ_ERR_ARG, "even"}, {{px, 8, 3, 24, 0, 3}, VJ_ERR_ARG, "even"}, {{px, 8, 4, 23, 0, 3}, VJ_ERR_ARG, "stride"},
        {{px, 65536, 2, 65536 * 3, 0, 3}, VJ_ERR_LIMIT, "65534"}};
    for (const auto& b : badb) {
        const vj_image v[3] = {goodb, goodb, b.f};
        bytes = 9;
        CHECK(vj_bgr_to_yuv_layout(v, 3, &ok, VJ_YUV_I420, yout, &bytes) == b.rc && bytes == 0);
        CHECK(strstr(vj_last_error(), "frame 2") != nullptr && strstr(vj_last_error(), b.word) != nullptr);
    }
    for (int k = 0; k < 4; ++k) {
        vj_yuv_params p = ok;
        const char* word = k == 0 ? "flags" : k == 1 ? "reserved" : "channels";
        if (k == 0) p.flags = 2u;
        if (k == 1) p.reserved = 1u;
        if (k == 2) p.channels = 1;
        if (k == 3) p.channels = 5;
        CHECK(vj_yuv_to_bgr_layout(&good, 1, &p, out, &bytes) == VJ_ERR_ARG && strstr(vj_last_error(), word) != nullptr);
        CHECK(vj_bgr_to_yuv_layout(&goodb, 1, &p, 0, yout, &bytes) == (k < 2 ? VJ_ERR_ARG : VJ_OK));   // the encoder's sources say their own
    }
    {   // the limits: a side of 65534 passes; 4095 such frames pass, 4096 hold more work units than a 32-bit index
        std::vector<vj_yuv_image> many(4096, vj_yuv_image{px, px, px, 65534, 65534, 65534, 65534, 0, 0});
        std::vector<vj_image> out_many(many.size());
        CHECK(vj_yuv_to_bgr_layout(many.data(), 4095, &ok, out_many.data(), &bytes) == VJ_OK);
        CHECK(vj_yuv_to_bgr_layout(many.data(), 4096, &ok, out_many.data(), &bytes) == VJ_ERR_LIMIT && strstr(vj_last_error(), "work units") != nullptr);
    }
    {   // a device-resident source plane that overlaps the destination (addresses only: nothing is read)
        uint8_t* const base = (uint8_t*)(uintptr_t)0x10000;
        const vj_yuv_image f[2] = {{base + 4096, base + 8192, base + 12288, 16, 4, 16, 8, VJ_YUV_I420, 1}, {base, base, base, 16, 4, 16, 16, VJ_YUV_NV12, 0}};
        CHECK(yuv_decode_check_overlap(f, 2, base, 4096) == VJ_OK);             // ends where the Y plane begins; the host frame is not looked at
        CHECK(yuv_decode_check_overlap(f, 2, base, 4097) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr && strstr(vj_last_error(), "y plane") != nullptr);
        CHECK(yuv_decode_check_overlap(f, 2, base + 4096 + 64, 4032) == VJ_OK);  // between the Y and the U plane
        CHECK(yuv_decode_check_overlap(f, 2, base + 4096 + 64, 4033) == VJ_ERR_ARG && strstr(vj_last_error(), "c0 plane") != nullptr);
        CHECK(yuv_decode_check_overlap(f, 2, base + 12288 + 15, 1) == VJ_ERR_ARG && strstr(vj_last_error(), "c1 plane") != nullptr);   // its last byte
        CHECK(yuv_decode_check_overlap(f, 2, base + 12288 + 16, 1) == VJ_OK);
        const vj_yuv_image nv = {base + 4096, base + 8192, base + 12288, 16, 4, 16, 16, VJ_YUV_NV12, 1};
        CHECK(yuv_decode_check_overlap(&nv, 1, base + 12288, 64) == VJ_OK);     // NV12 has no c1 plane
        const vj_image b[2] = {{base + 4096, 5, 4, 20, 1, 3}, {base, 16, 4, 48, 0, 3}};
        CHECK(yuv_encode_check_overlap(b, 2, base, 4096) == VJ_OK);
        CHECK(yuv_encode_check_overlap(b, 2, base, 4097) == VJ_ERR_ARG && strstr(vj_last_error(), "frame 0") != nullptr);
        CHECK(yuv_encode_check_overlap(b, 2, base + 4096 + 3 * 20 + 14, 1) == VJ_ERR_ARG);
        CHECK(yuv_encode_check_overlap(b, 2, base + 4096 + 3 * 20 + 15, 1) == VJ_OK);
    }
    {   // vj_yuv_luma
        vj_image g;
        const vj_yuv_image f = {px, nullptr, nullptr, 9, 5, 12, 0, 7, 1};
        CHECK(vj_yuv_luma(&f, &g) == VJ_OK && g.data == px && g.width == 9 && g.height == 5 && g.stride == 12 && g.on_device == 1 && g.channels == 1);
        CHECK(vj_yuv_luma(nullptr, &g) == VJ_ERR_ARG && vj_yuv_luma(&f, nullptr) == VJ_ERR_ARG);
    }
    printf("yuv_asan_driver: OK\n");
    return 0;
}
