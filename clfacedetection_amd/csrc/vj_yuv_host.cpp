// Host planner of vj_yuv_to_bgr / vj_bgr_to_yuv that needs no device: see vj_yuv_host.hpp.
#include "vj_yuv_host.hpp"

#include <cstring>

namespace vj {

namespace {

constexpr uint32_t YUV_MAX_SIDE = 65534;

int check_params(const vj_yuv_params* p, bool decode) {
    if (!p) {
        set_error("vj_yuv_params: null parameters");
        return VJ_ERR_ARG;
    }
    if ((p->flags & ~(uint32_t)VJ_YUV_RGB_ORDER) != 0u || p->reserved != 0u) {
        set_error("vj_yuv_params: %s", p->reserved != 0u ? "reserved must be 0" : "unknown bits in flags");
        return VJ_ERR_ARG;
    }
    if (decode && p->channels != 3 && p->channels != 4) {
        set_error("vj_yuv_params: channels must be 3 (BGR) or 4 (BGRA), not %d", p->channels);
        return VJ_ERR_ARG;
    }
    return VJ_OK;
}

// the sizes every 4:2:0 frame obeys
int check_size(int i, int32_t w, int32_t h) {
    if (w <= 0 || h <= 0) {
        set_error("frame %d: width and height must be positive", i);
        return VJ_ERR_ARG;
    }
    if ((uint32_t)w > YUV_MAX_SIDE || (uint32_t)h > YUV_MAX_SIDE) {
        set_error("frame %d: %d x %d: sides up to 65534", i, w, h);
        return VJ_ERR_LIMIT;
    }
    if (((w | h) & 1) != 0) {
        set_error("frame %d: %d x %d: width and height must be even (4:2:0 chroma)", i, w, h);
        return VJ_ERR_ARG;
    }
    return VJ_OK;
}

bool overlaps(const uint8_t* p, uint64_t rows, uint64_t stride, uint64_t row_bytes, uintptr_t d0, uintptr_t d1) {
    const uintptr_t s0 = (uintptr_t)p, s1 = s0 + (rows - 1u) * stride + row_bytes;
    return s0 < d1 && d0 < s1;
}

int too_many_units() {
    set_error("vj_yuv: the frames hold more work units than a 32-bit index holds");
    return VJ_ERR_LIMIT;
}

}  // namespace

int yuv_decode_layout(const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, YuvLayout* out) {
    *out = YuvLayout{};
    int rc = check_params(p, true);
    if (rc) return rc;
    if (n_frames < 0 || (n_frames > 0 && !frames)) {
        set_error("vj_yuv_to_bgr: null frames");
        return VJ_ERR_ARG;
    }
    out->channels = (uint32_t)p->channels;
    out->swap_rb = (p->flags & VJ_YUV_RGB_ORDER) != 0u;
    out->slots.reserve((size_t)n_frames);
    uint64_t off = 0, units = 0;
    for (int i = 0; i < n_frames; ++i) {
        const vj_yuv_image& f = frames[i];
        if (f.layout != VJ_YUV_NV12 && f.layout != VJ_YUV_NV21 && f.layout != VJ_YUV_I420) {
            set_error("frame %d: unknown layout %d", i, f.layout);
            return VJ_ERR_ARG;
        }
        if (!f.y || !f.c0 || (f.layout == VJ_YUV_I420 && !f.c1)) {
            set_error("frame %d: null %s plane", i, !f.y ? "y" : !f.c0 ? "c0" : "c1");
            return VJ_ERR_ARG;
        }
        if ((rc = check_size(i, f.width, f.height))) return rc;
        if (f.y_stride < f.width || (int64_t)f.c_stride < (int64_t)yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width)) {
            set_error("frame %d: %s is below the plane's row bytes", i, f.y_stride < f.width ? "y_stride" : "c_stride");
            return VJ_ERR_ARG;
        }
        YuvSlot t;
        t.w = (uint32_t)f.width;
        t.h = (uint32_t)f.height;
        t.ch = out->channels;
        t.pitch = yuv_align4(t.w * t.ch);
        t.off = (off + 255u) & ~(uint64_t)255;
        off = t.off + (uint64_t)t.pitch * t.h;
        units += yuv_units(t.w, t.h);
        out->slots.push_back(t);
    }
    if (units > 0x7fffffffull) return too_many_units();
    out->bytes = off;
    return VJ_OK;
}

int yuv_encode_layout(const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, YuvLayout* out) {
    *out = YuvLayout{};
    int rc = check_params(p, false);
    if (rc) return rc;
    if (layout != VJ_YUV_NV12 && layout != VJ_YUV_NV21 && layout != VJ_YUV_I420) {
        set_error("vj_bgr_to_yuv: unknown layout %d", layout);
        return VJ_ERR_ARG;
    }
    if (n_frames < 0 || (n_frames > 0 && !frames)) {
        set_error("vj_bgr_to_yuv: null frames");
        return VJ_ERR_ARG;
    }
    out->layout = (uint32_t)layout;
    out->swap_rb = (p->flags & VJ_YUV_RGB_ORDER) != 0u;
    out->slots.reserve((size_t)n_frames);
    uint64_t off = 0, units = 0;
    for (int i = 0; i < n_frames; ++i) {
        const vj_image& f = frames[i];
        if (!f.data) {
            set_error("frame %d: null data", i);
            return VJ_ERR_ARG;
        }
        if (f.channels != 3 && f.channels != 4) {
            set_error("frame %d: a source must have 3 (BGR) or 4 (BGRA) channels%s", i, f.channels <= 1 ? ": a gray frame has no colour to encode" : "");
            return VJ_ERR_ARG;
        }
        if ((rc = check_size(i, f.width, f.height))) return rc;
        if ((int64_t)f.stride < (int64_t)f.width * f.channels) {
            set_error("frame %d: stride is below width * channels", i);
            return VJ_ERR_ARG;
        }
        YuvSlot t;
        t.w = (uint32_t)f.width;
        t.h = (uint32_t)f.height;
        t.ch = (uint32_t)f.channels;
        t.pitch = yuv_align4(t.w);
        t.off = (off + 255u) & ~(uint64_t)255;
        off = t.off + yuv_frame_bytes(out->layout, t.w, t.h);
        units += yuv_units(t.w, t.h);
        out->slots.push_back(t);
    }
    if (units > 0x7fffffffull) return too_many_units();
    out->bytes = off;
    return VJ_OK;
}

int yuv_decode_check_overlap(const vj_yuv_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes) {
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + bytes;
    for (int i = 0; i < n_frames; ++i) {
        const vj_yuv_image& f = frames[i];
        if (!f.on_device) continue;
        const uint64_t ch_rows = (uint64_t)f.height / 2u, ch_bytes = yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width);
        const char* which = overlaps(f.y, (uint64_t)f.height, (uint64_t)f.y_stride, (uint64_t)f.width, d0, d1) ? "y"
                            : overlaps(f.c0, ch_rows, (uint64_t)f.c_stride, ch_bytes, d0, d1)                 ? "c0"
                            : f.layout == VJ_YUV_I420 && overlaps(f.c1, ch_rows, (uint64_t)f.c_stride, ch_bytes, d0, d1) ? "c1" : nullptr;
        if (which) {
            set_error("frame %d: the device-resident %s plane overlaps the destination buffer", i, which);
            return VJ_ERR_ARG;
        }
    }
    return VJ_OK;
}

int yuv_encode_check_overlap(const vj_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes) {
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + bytes;
    for (int i = 0; i < n_frames; ++i) {
        const vj_image& f = frames[i];
        if (!f.on_device) continue;
        if (overlaps(f.data, (uint64_t)f.height, (uint64_t)f.stride, (uint64_t)f.width * (uint64_t)f.channels, d0, d1)) {
            set_error("frame %d: a device-resident source overlaps the destination buffer", i);
            return VJ_ERR_ARG;
        }
    }
    return VJ_OK;
}

int yuv_decode_plan_slice(const vj_yuv_image* frames, const YuvLayout& lay, size_t first, size_t n, YuvSlice* out) {
    out->recs.clear();
    out->n_units = 0;
    if (first + n > lay.slots.size()) {
        set_error("internal error: a slice beyond the call's frames");
        return VJ_ERR_ARG;
    }
    uint64_t unit = 0;
    for (size_t i = 0; i < n; ++i) {
        const YuvSlot& t = lay.slots[first + i];
        const vj_yuv_image& f = frames[first + i];
        YuvFrameDev d;
        memset(&d, 0, sizeof(d));
        d.y = f.y;
        d.c0 = f.c0;
        d.c1 = f.layout == VJ_YUV_I420 ? f.c1 : nullptr;
        d.dst_off = t.off;
        d.y_stride = (uint32_t)f.y_stride;
        d.c_stride = (uint32_t)f.c_stride;
        d.width = t.w;
        d.height = t.h;
        d.pitch = t.pitch;
        d.channels = t.ch;
        d.layout = (uint32_t)f.layout;
        d.unit_first = (uint32_t)unit;
        unit += yuv_units(t.w, t.h);
        if (unit > 0x7fffffffull) return too_many_units();
        out->recs.push_back(d);
    }
    out->n_units = (uint32_t)unit;
    return VJ_OK;
}

int yuv_encode_plan_slice(const vj_image* frames, const YuvLayout& lay, size_t first, size_t n, YuvSlice* out) {
    out->recs.clear();
    out->n_units = 0;
    if (first + n > lay.slots.size()) {
        set_error("internal error: a slice beyond the call's frames");
        return VJ_ERR_ARG;
    }
    uint64_t unit = 0;
    for (size_t i = 0; i < n; ++i) {
        const YuvSlot& t = lay.slots[first + i];
        const vj_image& f = frames[first + i];
        YuvFrameDev d;
        memset(&d, 0, sizeof(d));
        d.y = f.data;
        d.layout = lay.layout;
        d.dst_off = t.off;
        d.y_stride = (uint32_t)f.stride;
        d.width = t.w;
        d.height = t.h;
        d.pitch = t.pitch;
        d.channels = t.ch;
        d.unit_first = (uint32_t)unit;
        unit += yuv_units(t.w, t.h);
        if (unit > 0x7fffffffull) return too_many_units();
        out->recs.push_back(d);
    }
    out->n_units = (uint32_t)unit;
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

void vj_yuv_default(vj_yuv_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->channels = 3;
}

int vj_yuv_to_bgr_layout(const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, vj_image* out, uint64_t* bytes) {
    if (bytes) *bytes = 0;
    if (!p || !bytes || n_frames < 0 || (n_frames > 0 && (!frames || !out))) {
        set_error("vj_yuv_to_bgr_layout: null argument");
        return VJ_ERR_ARG;
    }
    YuvLayout lay;
    const int rc = yuv_decode_layout(frames, n_frames, p, &lay);
    if (rc) return rc;
    for (int i = 0; i < n_frames; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        out[i] = vj_image{(const uint8_t*)(uintptr_t)t.off, (int32_t)t.w, (int32_t)t.h, (int32_t)t.pitch, 1, (int32_t)t.ch};
    }
    *bytes = lay.bytes;
    return VJ_OK;
}

int vj_bgr_to_yuv_layout(const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, vj_yuv_image* out, uint64_t* bytes) {
    if (bytes) *bytes = 0;
    if (!p || !bytes || n_frames < 0 || (n_frames > 0 && (!frames || !out))) {
        set_error("vj_bgr_to_yuv_layout: null argument");
        return VJ_ERR_ARG;
    }
    YuvLayout lay;
    const int rc = yuv_encode_layout(frames, n_frames, p, layout, &lay);
    if (rc) return rc;
    for (int i = 0; i < n_frames; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        const uint32_t L = lay.layout;
        out[i] = vj_yuv_image{(const uint8_t*)(uintptr_t)t.off,
                              (const uint8_t*)(uintptr_t)(t.off + yuv_plane_off(L, t.w, t.h, 1u)),
                              L == YUV_I420 ? (const uint8_t*)(uintptr_t)(t.off + yuv_plane_off(L, t.w, t.h, 2u)) : nullptr,
                              (int32_t)t.w, (int32_t)t.h, (int32_t)t.pitch, (int32_t)yuv_plane_pitch(L, t.w, 1u), (int32_t)L, 1};
    }
    *bytes = lay.bytes;
    return VJ_OK;
}

int vj_yuv_luma(const vj_yuv_image* f, vj_image* out) {
    if (!f || !out) {
        set_error("vj_yuv_luma: null argument");
        return VJ_ERR_ARG;
    }
    if (!f->y || f->width <= 0 || f->height <= 0 || f->y_stride < f->width) {
        set_error("vj_yuv_luma: %s", !f->y ? "null y plane" : f->y_stride < f->width ? "y_stride is below width" : "width and height must be positive");
        return VJ_ERR_ARG;
    }
    *out = vj_image{f->y, f->width, f->height, f->y_stride, f->on_device, 1};
    return VJ_OK;
}

}  // extern "C"
