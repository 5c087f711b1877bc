// vj_yuv_to_bgr / vj_bgr_to_yuv: a decoder's 4:2:0 frames to BGR / BGRA in a device buffer of the caller's, and
// back.  The planner (vj_yuv_host.cpp) checks the call and lays the outputs out; here a slice of the call — all of it unless
// "max_subbatch" is set — is one copy (its frame records and its host frames, every plane gathered at a 4-byte pitch in the lane's
// page-locked staging buffer as vj_preprocess stages its sources) and one launch per layout (decode) or channel count (encode) the
// slice holds.  The block lives in d_yuv: [records | staged planes].
#include "vj_env_internal.hpp"
#include "vj_yuv_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }
inline size_t align4(size_t v) { return (v + 3u) & ~(size_t)3; }

int stage_reserve(vj_env* e, size_t bytes) {
    Lane* L = &e->lane0;
    if (L->h_stage_bytes < bytes) {
        if (L->h_stage) (void)hipHostFree(L->h_stage);
        L->h_stage = nullptr;
        L->h_stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&L->h_stage, bytes, hipHostMallocDefault));
        L->h_stage_bytes = bytes;
    }
    return e->d_yuv.ensure(bytes);
}

// rows of row_bytes bytes, `stride` apart, to hs + at at a 4-byte pitch; returns the bytes taken
size_t stage_plane(uint8_t* hs, size_t at, const uint8_t* src, size_t rows, size_t stride, size_t row_bytes) {
    const size_t pitch = align4(row_bytes);
    for (size_t y = 0; y < rows; ++y) memcpy(hs + at + y * pitch, src + y * stride, row_bytes);
    return pitch * rows;
}

int enqueue_decode_slice(vj_env* e, const vj_yuv_image* frames, const YuvLayout& lay, size_t first, size_t n, uint8_t* d_dst, YuvSlice* sl) {
    int rc;
    if ((rc = yuv_decode_plan_slice(frames, lay, first, n, sl))) return rc;
    const size_t rec_bytes = align16(n * sizeof(YuvFrameDev));
    size_t bytes = rec_bytes;
    bool has[3] = {false, false, false};
    for (size_t i = 0; i < n; ++i) {
        const vj_yuv_image& f = frames[first + i];
        has[f.layout] = true;
        if (f.on_device) continue;
        const size_t cb = align4(yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width)), planes = f.layout == VJ_YUV_I420 ? 2u : 1u;
        bytes += align4((size_t)f.width) * (size_t)f.height + planes * cb * ((size_t)f.height / 2u);
    }
    if ((rc = stage_reserve(e, bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_yuv.p;
    size_t at = rec_bytes;
    for (size_t i = 0; i < n; ++i) {
        const vj_yuv_image& f = frames[first + i];
        if (f.on_device) continue;
        YuvFrameDev& d = sl->recs[i];
        const size_t crow = yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width), crows = (size_t)f.height / 2u;
        d.y = dev + at;
        d.y_stride = (uint32_t)align4((size_t)f.width);
        at += stage_plane(hs, at, f.y, (size_t)f.height, (size_t)f.y_stride, (size_t)f.width);
        d.c0 = dev + at;
        d.c_stride = (uint32_t)align4(crow);
        at += stage_plane(hs, at, f.c0, crows, (size_t)f.c_stride, crow);
        if (f.layout == VJ_YUV_I420) {
            d.c1 = dev + at;
            at += stage_plane(hs, at, f.c1, crows, (size_t)f.c_stride, crow);
        }
    }
    memcpy(hs, sl->recs.data(), n * sizeof(YuvFrameDev));
    HIP_TRY(hipMemcpyAsync(e->d_yuv.p, hs, bytes, hipMemcpyHostToDevice, e->stream));
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const YuvFrameDev*)dev;
    a.n_frames = (uint32_t)n;
    a.n_units = sl->n_units;
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    a.channels = lay.channels;
    a.swap_rb = lay.swap_rb ? 1u : 0u;
    for (uint32_t L = 0; L < 3u; ++L) {
        if (!has[L]) continue;
        a.layout = L;
        const int hrc = launch_yuv_to_bgr(a, e->stream);
        if (hrc) {
            set_error("yuv_to_bgr launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
    }
    return VJ_OK;
}

int enqueue_encode_slice(vj_env* e, const vj_image* frames, const YuvLayout& lay, size_t first, size_t n, uint8_t* d_dst, YuvSlice* sl) {
    int rc;
    if ((rc = yuv_encode_plan_slice(frames, lay, first, n, sl))) return rc;
    const size_t rec_bytes = align16(n * sizeof(YuvFrameDev));
    size_t bytes = rec_bytes;
    bool has[5] = {false, false, false, false, false};
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        has[f.channels] = true;
        if (!f.on_device) bytes += align4((size_t)f.width * (size_t)f.channels) * (size_t)f.height;
    }
    if ((rc = stage_reserve(e, bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_yuv.p;
    size_t at = rec_bytes;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)f.channels;
        sl->recs[i].y = dev + at;
        sl->recs[i].y_stride = (uint32_t)align4(row_bytes);
        at += stage_plane(hs, at, f.data, (size_t)f.height, (size_t)f.stride, row_bytes);
    }
    memcpy(hs, sl->recs.data(), n * sizeof(YuvFrameDev));
    HIP_TRY(hipMemcpyAsync(e->d_yuv.p, hs, bytes, hipMemcpyHostToDevice, e->stream));
    YuvArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const YuvFrameDev*)dev;
    a.n_frames = (uint32_t)n;
    a.n_units = sl->n_units;
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    a.layout = lay.layout;
    a.swap_rb = lay.swap_rb ? 1u : 0u;
    for (uint32_t ch = 3; ch <= 4u; ++ch) {
        if (!has[ch]) continue;
        a.channels = ch;
        const int hrc = launch_bgr_to_yuv(a, e->stream);
        if (hrc) {
            set_error("bgr_to_yuv launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
    }
    return VJ_OK;
}

// What both directions share once the layout stands: the checks on the destination, then the slices between the events
template <typename Frame, typename Overlap, typename Enqueue>
int run_yuv(vj_env* e, const char* who, const Frame* frames, int n_frames, const YuvLayout& lay, uint8_t* d_dst, uint64_t dst_bytes, Overlap overlap,
            Enqueue enqueue) {
    if (dst_bytes < lay.bytes) {
        set_error("%s: dst_bytes %llu is below the %llu bytes the layout needs", who, (unsigned long long)dst_bytes, (unsigned long long)lay.bytes);
        return VJ_ERR_ARG;
    }
    if (((uintptr_t)d_dst & 3u) != 0u) {
        set_error("%s: d_dst must be a multiple of 4", who);
        return VJ_ERR_ARG;
    }
    int rc;
    if ((rc = overlap(frames, n_frames, d_dst, lay.bytes))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t per_slice = e->max_subbatch > 0 ? (size_t)e->max_subbatch : (size_t)n_frames;
    YuvSlice sl;
    HIP_TRY(hipEventRecord(e->yuv_ev[0], e->stream));
    for (size_t first = 0; first < (size_t)n_frames; first += per_slice) {
        const size_t n = std::min(per_slice, (size_t)n_frames - first);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = enqueue(e, frames, lay, first, n, d_dst, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
    }
    HIP_TRY(hipEventRecord(e->yuv_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->yuv_ev[0], e->yuv_ev[1]));
    e->yuv_ms = ms;
    return VJ_OK;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_yuv_to_bgr(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, uint8_t* d_dst, uint64_t dst_bytes, vj_image* out) {
    if (!e || !p || n_frames < 0 || (n_frames > 0 && (!frames || !out || !d_dst))) {
        set_error("vj_yuv_to_bgr: null argument");
        return VJ_ERR_ARG;
    }
    YuvLayout lay;
    int rc = yuv_decode_layout(frames, n_frames, p, &lay);
    if (rc) return rc;
    if (n_frames == 0) return VJ_OK;
    if ((rc = run_yuv(e, "vj_yuv_to_bgr", frames, n_frames, lay, d_dst, dst_bytes, yuv_decode_check_overlap, enqueue_decode_slice))) return rc;
    for (int i = 0; i < n_frames; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        out[i] = vj_image{d_dst + t.off, (int32_t)t.w, (int32_t)t.h, (int32_t)t.pitch, 1, (int32_t)t.ch};
    }
    return VJ_OK;
}

int vj_bgr_to_yuv(vj_env* e, const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, uint8_t* d_dst, uint64_t dst_bytes,
                  vj_yuv_image* out) {
    if (!e || !p || n_frames < 0 || (n_frames > 0 && (!frames || !out || !d_dst))) {
        set_error("vj_bgr_to_yuv: null argument");
        return VJ_ERR_ARG;
    }
    YuvLayout lay;
    int rc = yuv_encode_layout(frames, n_frames, p, layout, &lay);
    if (rc) return rc;
    if (n_frames == 0) return VJ_OK;
    if ((rc = run_yuv(e, "vj_bgr_to_yuv", frames, n_frames, lay, d_dst, dst_bytes, yuv_encode_check_overlap, enqueue_encode_slice))) return rc;
    const uint32_t L = lay.layout;
    for (int i = 0; i < n_frames; ++i) {
        const YuvSlot& t = lay.slots[(size_t)i];
        uint8_t* base = d_dst + t.off;
        out[i] = vj_yuv_image{base, base + yuv_plane_off(L, t.w, t.h, 1u), L == YUV_I420 ? base + yuv_plane_off(L, t.w, t.h, 2u) : nullptr,
                              (int32_t)t.w, (int32_t)t.h, (int32_t)t.pitch, (int32_t)yuv_plane_pitch(L, t.w, 1u), (int32_t)L, 1};
    }
    return VJ_OK;
}

int vj_yuv_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->yuv_ms;
    return VJ_OK;
}

}  // extern "C"
