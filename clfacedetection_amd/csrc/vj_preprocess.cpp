// vj_preprocess: gray, resized, equalized frames written into a device buffer of the caller's.  The planner
// (vj_prep_host.cpp) checks the call and lays the images out; here a slice of the call — all of it unless "max_subbatch" is set —
// is one copy (its frame records, the records equalize_lut reads, its taps and its host frames, gathered at a 4-byte pitch in the
// lane's page-locked staging buffer as vj_detect_mixed stages its atlas sources), one memset of the histograms, and the launches.
#include "vj_env_internal.hpp"
#include "vj_prep_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

int enqueue_prep_slice(vj_env* e, const vj_image* frames, const PrepLayout& lay, size_t first, size_t n, uint8_t* d_dst, PrepSlice* sl) {
    int rc;
    if ((rc = prep_plan_slice(frames, lay, first, n, sl))) return rc;
    const size_t rec_bytes = align16(n * sizeof(PrepFrameDev)), eq_bytes = align16(n * sizeof(AtlasFrameDev));
    const size_t tap_bytes = align16(sl->taps.size() * sizeof(PyrTap));
    size_t bytes = rec_bytes + eq_bytes + tap_bytes;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (!f.on_device) bytes += (((size_t)f.width * (size_t)image_channels(f) + 3u) & ~(size_t)3) * (size_t)f.height;
    }
    Lane* L = &e->lane0;
    if (L->h_stage_bytes < bytes) {
        if (L->h_stage) (void)hipHostFree(L->h_stage);
        L->h_stage = nullptr;
        L->h_stage_bytes = 0;
        HIP_TRY(hipHostMalloc(&L->h_stage, bytes, hipHostMallocDefault));
        L->h_stage_bytes = bytes;
    }
    if ((rc = e->d_prep.ensure(bytes))) return rc;
    uint8_t* hs = (uint8_t*)L->h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_prep.p;
    size_t at = rec_bytes + eq_bytes + tap_bytes;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f), pitch = (row_bytes + 3u) & ~(size_t)3;
        for (int y = 0; y < f.height; ++y) memcpy(hs + at + (size_t)y * pitch, f.data + (size_t)y * (size_t)f.stride, row_bytes);
        sl->recs[i].src = dev + at;
        sl->recs[i].stride = (uint32_t)pitch;
        at += pitch * (size_t)f.height;
    }
    memcpy(hs, sl->recs.data(), n * sizeof(PrepFrameDev));
    memcpy(hs + rec_bytes, sl->eq.data(), n * sizeof(AtlasFrameDev));
    if (!sl->taps.empty()) memcpy(hs + rec_bytes + eq_bytes, sl->taps.data(), sl->taps.size() * sizeof(PyrTap));
    HIP_TRY(hipMemcpyAsync(e->d_prep.p, hs, bytes, hipMemcpyHostToDevice, e->stream));
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const PrepFrameDev*)dev;
    a.n_frames = (uint32_t)n;
    a.n_units = sl->n_units;
    a.taps = (const PyrTap*)(dev + rec_bytes + eq_bytes);
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    int hrc;
    if (!lay.equalize) {
        hrc = launch_prep_resize(a, false, e->stream);
    } else {
        if ((rc = L->d_eq_hist.ensure(n * 256u * sizeof(uint32_t)))) return rc;
        if ((rc = L->d_eq_lut.ensure(n * 256u))) return rc;
        HIP_TRY(hipMemsetAsync(L->d_eq_hist.p, 0, n * 256u * sizeof(uint32_t), e->stream));
        a.hist = (uint32_t*)L->d_eq_hist.p;
        a.lut = (const uint8_t*)L->d_eq_lut.p;
#ifdef PREP_UNFUSED_HIST
        hrc = launch_prep_resize(a, false, e->stream);
        if (!hrc) hrc = launch_prep_hist(a, e->stream);
#else
        hrc = launch_prep_resize(a, true, e->stream);
#endif
        EqualizeArgs q;
        memset(&q, 0, sizeof(q));
        q.frames = (const AtlasFrameDev*)(dev + rec_bytes);
        q.n_frames = (uint32_t)n;
        q.hist = (uint32_t*)L->d_eq_hist.p;
        q.lut = (uint8_t*)L->d_eq_lut.p;
        if (!hrc) hrc = launch_equalize_lut(q, e->stream);
        if (!hrc) hrc = launch_prep_apply(a, e->stream);
    }
    if (hrc) {
        set_error("preprocess launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_preprocess(vj_env* e, const vj_image* frames, int n_frames, const vj_prep* p, uint8_t* d_dst, uint64_t dst_bytes, vj_image* out) {
    if (!e || !p || n_frames < 0 || (n_frames > 0 && (!frames || !out || !d_dst))) {
        set_error("vj_preprocess: null argument");
        return VJ_ERR_ARG;
    }
    PrepLayout lay;
    int rc = prep_layout(frames, n_frames, p, &lay);
    if (rc) return rc;
    if (n_frames == 0) return VJ_OK;
    if (dst_bytes < lay.bytes) {
        set_error("vj_preprocess: dst_bytes %llu is below the %llu bytes the layout needs", (unsigned long long)dst_bytes, (unsigned long long)lay.bytes);
        return VJ_ERR_ARG;
    }
    if (((uintptr_t)d_dst & 3u) != 0u) {
        set_error("vj_preprocess: d_dst must be a multiple of 4");
        return VJ_ERR_ARG;
    }
    if ((rc = prep_check_overlap(frames, n_frames, d_dst, lay.bytes))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t per_slice = e->max_subbatch > 0 ? (size_t)e->max_subbatch : (size_t)n_frames;
    PrepSlice sl;
    HIP_TRY(hipEventRecord(e->prep_ev[0], e->stream));
    for (size_t first = 0; first < (size_t)n_frames; first += per_slice) {
        const size_t n = std::min(per_slice, (size_t)n_frames - first);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = enqueue_prep_slice(e, frames, lay, first, n, d_dst, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
    }
    HIP_TRY(hipEventRecord(e->prep_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->prep_ev[0], e->prep_ev[1]));
    e->prep_ms = ms;
    for (int i = 0; i < n_frames; ++i) {
        const PrepSlot& t = lay.slots[(size_t)i];
        out[i] = vj_image{d_dst + t.off, (int32_t)t.dw, (int32_t)t.dh, (int32_t)t.pitch, 1, 1};
    }
    return VJ_OK;
}

int vj_preprocess_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->prep_ms;
    return VJ_OK;
}

}  // extern "C"
