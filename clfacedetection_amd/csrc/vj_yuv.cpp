// vj_yuv_to_bgr / vj_bgr_to_yuv: a decoder's 4:2:0 frames to BGR / BGRA in a device buffer of the caller's, and
// back.  The planner (vj_yuv_host.cpp) checks the call and lays the outputs out; here a slice of the call — all of it unless
// "max_subbatch" is set — is one copy (its frame records and its host frames, every plane gathered at a 4-byte pitch in the lane's
// page-locked staging buffer) and one launch per layout (decode) or channel count (encode) the slice holds.  The block lives in
// d_yuv: [records | staged planes].  The call's skeleton is the shared one (vj_slice.hpp, §4.24).
#include "vj_slice.hpp"
#include "vj_yuv_host.hpp"

namespace vj {

namespace {

int enqueue_decode_slice(vj_env* e, const vj_yuv_image* frames, const YuvLayout& lay, size_t first, size_t n, uint8_t* d_dst, YuvSlice* sl) {
    int rc;
    if ((rc = yuv_decode_plan_slice(frames, lay, first, n, sl))) return rc;
    StageBlock head;
    head.section(n * sizeof(YuvFrameDev));
    StageBlock b = head;
    bool has[3] = {false, false, false};
    for (size_t i = 0; i < n; ++i) {
        const vj_yuv_image& f = frames[first + i];
        has[f.layout] = true;
        if (f.on_device) continue;
        b.rows((size_t)f.width, (size_t)f.height);
        b.rows(yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width), (f.layout == VJ_YUV_I420 ? 2u : 1u) * ((size_t)f.height / 2u));
    }
    if ((rc = stage_reserve(&e->lane0, b.bytes))) return rc;
    if ((rc = e->d_yuv.ensure(b.bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_yuv.p;
    b = head;
    for (size_t i = 0; i < n; ++i) {
        const vj_yuv_image& f = frames[first + i];
        if (f.on_device) continue;
        YuvFrameDev& d = sl->recs[i];
        const size_t crow = yuv_chroma_row_bytes((uint32_t)f.layout, (uint32_t)f.width), crows = (size_t)f.height / 2u;
        d.y = dev + stage_rows(hs, &b, f.y, (size_t)f.y_stride, (size_t)f.height, (size_t)f.width);
        d.y_stride = (uint32_t)align4((size_t)f.width);
        d.c0 = dev + stage_rows(hs, &b, f.c0, (size_t)f.c_stride, crows, crow);
        d.c_stride = (uint32_t)align4(crow);
        if (f.layout == VJ_YUV_I420) d.c1 = dev + stage_rows(hs, &b, f.c1, (size_t)f.c_stride, crows, crow);
    }
    memcpy(hs, sl->recs.data(), n * sizeof(YuvFrameDev));
    HIP_TRY(hipMemcpyAsync(e->d_yuv.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
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
    StageBlock head;
    head.section(n * sizeof(YuvFrameDev));
    StageBlock b = head;
    bool has[5] = {false, false, false, false, false};
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        has[f.channels] = true;
        if (!f.on_device) b.rows((size_t)f.width * (size_t)f.channels, (size_t)f.height);
    }
    if ((rc = stage_reserve(&e->lane0, b.bytes))) return rc;
    if ((rc = e->d_yuv.ensure(b.bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_yuv.p;
    b = head;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)f.channels;
        sl->recs[i].y = dev + stage_rows(hs, &b, f.data, (size_t)f.stride, (size_t)f.height, row_bytes);
        sl->recs[i].y_stride = (uint32_t)align4(row_bytes);
    }
    memcpy(hs, sl->recs.data(), n * sizeof(YuvFrameDev));
    HIP_TRY(hipMemcpyAsync(e->d_yuv.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
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
    int rc;
    if ((rc = check_dst(who, frames, n_frames, d_dst, dst_bytes, lay.bytes, true, overlap))) return rc;
    YuvSlice sl;
    return run_slices(e, e->call_ev, &e->yuv_ms, (size_t)n_frames, slices_of(e, (size_t)n_frames),
                      [&](size_t first, size_t end) { return enqueue(e, frames, lay, first, end - first, d_dst, &sl); });
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
