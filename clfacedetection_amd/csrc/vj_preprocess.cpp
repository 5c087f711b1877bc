// vj_preprocess: gray, resized, equalized frames written into a device buffer of the caller's.  The planner
// (vj_prep_host.cpp) checks the call and lays the images out; here a slice of the call — all of it unless "max_subbatch" is set —
// is one copy (its frame records, the records equalize_lut reads, its taps and its host frames, gathered at a 4-byte pitch in the
// lane's page-locked staging buffer), one memset of the histograms, and the launches.  The call's skeleton is the shared one
// (vj_slice.hpp, §4.24).
#include "vj_slice.hpp"
#include "vj_prep_host.hpp"

namespace vj {

namespace {

int enqueue_prep_slice(vj_env* e, const vj_image* frames, const PrepLayout& lay, size_t first, size_t n, uint8_t* d_dst, PrepSlice* sl) {
    int rc;
    if ((rc = prep_plan_slice(frames, lay, first, n, sl))) return rc;
    StageBlock head;
    head.section(n * sizeof(PrepFrameDev));
    const size_t eq_at = head.section(n * sizeof(AtlasFrameDev)), tap_at = head.section(sl->taps.size() * sizeof(PyrTap));
    StageBlock b = head;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (!f.on_device) b.rows((size_t)f.width * (size_t)image_channels(f), (size_t)f.height);
    }
    Lane* L = &e->lane0;
    if ((rc = stage_reserve(L, b.bytes))) return rc;
    if ((rc = e->d_prep.ensure(b.bytes))) return rc;
    uint8_t* hs = (uint8_t*)L->h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_prep.p;
    b = head;
    for (size_t i = 0; i < n; ++i) {
        const vj_image& f = frames[first + i];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f);
        sl->recs[i].src = dev + stage_rows(hs, &b, f.data, (size_t)f.stride, (size_t)f.height, row_bytes);
        sl->recs[i].stride = (uint32_t)align4(row_bytes);
    }
    memcpy(hs, sl->recs.data(), n * sizeof(PrepFrameDev));
    memcpy(hs + eq_at, sl->eq.data(), n * sizeof(AtlasFrameDev));
    if (!sl->taps.empty()) memcpy(hs + tap_at, sl->taps.data(), sl->taps.size() * sizeof(PyrTap));
    HIP_TRY(hipMemcpyAsync(e->d_prep.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
    PrepArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const PrepFrameDev*)dev;
    a.n_frames = (uint32_t)n;
    a.n_units = sl->n_units;
    a.taps = (const PyrTap*)(dev + tap_at);
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
        q.frames = (const AtlasFrameDev*)(dev + eq_at);
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
    if ((rc = check_dst("vj_preprocess", frames, n_frames, d_dst, dst_bytes, lay.bytes, true, prep_check_overlap))) return rc;
    PrepSlice sl;
    rc = run_slices(e, e->call_ev, &e->prep_ms, (size_t)n_frames, slices_of(e, (size_t)n_frames),
                    [&](size_t first, size_t end) { return enqueue_prep_slice(e, frames, lay, first, end - first, d_dst, &sl); });
    if (rc) return rc;
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
