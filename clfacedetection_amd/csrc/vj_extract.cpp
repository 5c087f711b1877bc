// vj_extract: regions of the call's frames, resized to one size, written into a device buffer of the caller's.
// The planner (vj_extract_host.cpp) checks the call and maps the regions; here a slice of the call — all of it unless "max_subbatch"
// is set: then runs of regions that name at most that many distinct frames — is one copy (its region records, its taps and the host
// frames it names, gathered at a 4-byte pitch in the lane's page-locked staging buffer) and one launch.  Device-resident frames are
// read where they lie.  The call's skeleton is the shared one (vj_slice.hpp, §4.24).
#include "vj_slice.hpp"
#include "vj_extract_host.hpp"
#include "vj_prep_host.hpp"

namespace vj {

int enqueue_extract_slice(vj_env* e, const vj_image* frames, const vj_roi* regions, const ExtractLayout& lay, size_t first, size_t n,
                          uint8_t* d_dst, ExtractSlice* sl) {
    int rc;
    if ((rc = extract_plan_slice(frames, regions, lay, first, n, sl))) return rc;
    StageBlock head;
    head.section(n * sizeof(ExtractRegionDev));
    const size_t tap_at = head.section(sl->taps.size() * sizeof(PyrTap));
    StageBlock b = head;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (!f.on_device) b.rows((size_t)f.width * (size_t)image_channels(f), (size_t)f.height);
    }
    if ((rc = stage_reserve(&e->lane0, b.bytes))) return rc;
    if ((rc = e->d_extract.ensure(b.bytes))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_extract.p;
    b = head;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f);
        const size_t at = stage_rows(hs, &b, f.data, (size_t)f.stride, (size_t)f.height, row_bytes);
        for (size_t i = 0; i < n; ++i)
            if (regions[first + i].frame == fi) {
                sl->recs[i].src = dev + at;
                sl->recs[i].stride = (uint32_t)align4(row_bytes);
            }
    }
    memcpy(hs, sl->recs.data(), n * sizeof(ExtractRegionDev));
    if (!sl->taps.empty()) memcpy(hs + tap_at, sl->taps.data(), sl->taps.size() * sizeof(PyrTap));
    HIP_TRY(hipMemcpyAsync(e->d_extract.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
    ExtractArgs a;
    memset(&a, 0, sizeof(a));
    a.regions = (const ExtractRegionDev*)dev;
    a.n_regions = (uint32_t)n;
    a.n_units = sl->n_units;
    a.taps = (const PyrTap*)(dev + tap_at);
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    a.out_w = lay.out_w;
    a.out_h = lay.out_h;
    a.C = lay.C;
    a.gray = lay.gray ? 1u : 0u;
    a.planar = lay.planar ? 1u : 0u;
    a.rows = lay.rows;
    a.row_bytes = lay.row_bytes;
    const int hrc = launch_extract(a, e->stream);
    if (hrc) {
        set_error("extract launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

int vj_extract(vj_env* e, const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
               uint8_t* d_dst, uint64_t dst_bytes) {
    if (!e || !p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && (!regions || !d_dst))) {
        set_error("vj_extract: null argument");
        return VJ_ERR_ARG;
    }
    ExtractLayout lay;
    int rc = extract_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    if (n_regions == 0) return VJ_OK;
    if ((rc = check_dst("vj_extract", frames, n_frames, d_dst, dst_bytes, lay.bytes, false, prep_check_overlap))) return rc;
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    ExtractSlice sl;
    return run_slices(
        e, e->call_ev, &e->extract_ms, (size_t)n_regions, [&](size_t first) { return extract_slice_end(regions, (size_t)n_regions, first, max_frames); },
        [&](size_t first, size_t end) { return enqueue_extract_slice(e, frames, regions, lay, first, end - first, d_dst, &sl); });
}

int vj_extract_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->extract_ms;
    return VJ_OK;
}

}  // extern "C"
