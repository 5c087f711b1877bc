// vj_extract: regions of the call's frames, resized to one size, written into a device buffer of the caller's.
// The planner (vj_extract_host.cpp) checks the call and maps the regions; here a slice of the call — all of it unless "max_subbatch"
// is set: then runs of regions that name at most that many distinct frames — is one copy (its region records, its taps and the host
// frames it names, gathered at a 4-byte pitch in the lane's page-locked staging buffer as vj_preprocess stages them) and one launch.
// Device-resident frames are read where they lie.
#include "vj_env_internal.hpp"
#include "vj_extract_host.hpp"
#include "vj_prep_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

}  // namespace

int enqueue_extract_slice(vj_env* e, const vj_image* frames, const vj_roi* regions, const ExtractLayout& lay, size_t first, size_t n,
                          uint8_t* d_dst, ExtractSlice* sl) {
    int rc;
    if ((rc = extract_plan_slice(frames, regions, lay, first, n, sl))) return rc;
    const size_t rec_bytes = align16(n * sizeof(ExtractRegionDev)), tap_bytes = align16(sl->taps.size() * sizeof(PyrTap));
    size_t bytes = rec_bytes + tap_bytes;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
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
    if ((rc = e->d_extract.ensure(bytes))) return rc;
    uint8_t* hs = (uint8_t*)L->h_stage;
    const uint8_t* dev = (const uint8_t*)e->d_extract.p;
    size_t at = rec_bytes + tap_bytes;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f), pitch = (row_bytes + 3u) & ~(size_t)3;
        for (int y = 0; y < f.height; ++y) memcpy(hs + at + (size_t)y * pitch, f.data + (size_t)y * (size_t)f.stride, row_bytes);
        for (size_t i = 0; i < n; ++i)
            if (regions[first + i].frame == fi) {
                sl->recs[i].src = dev + at;
                sl->recs[i].stride = (uint32_t)pitch;
            }
        at += pitch * (size_t)f.height;
    }
    memcpy(hs, sl->recs.data(), n * sizeof(ExtractRegionDev));
    if (!sl->taps.empty()) memcpy(hs + rec_bytes, sl->taps.data(), sl->taps.size() * sizeof(PyrTap));
    HIP_TRY(hipMemcpyAsync(e->d_extract.p, hs, bytes, hipMemcpyHostToDevice, e->stream));
    ExtractArgs a;
    memset(&a, 0, sizeof(a));
    a.regions = (const ExtractRegionDev*)dev;
    a.n_regions = (uint32_t)n;
    a.n_units = sl->n_units;
    a.taps = (const PyrTap*)(dev + rec_bytes);
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
    if (dst_bytes < lay.bytes) {
        set_error("vj_extract: dst_bytes %llu is below the %llu bytes the layout needs", (unsigned long long)dst_bytes, (unsigned long long)lay.bytes);
        return VJ_ERR_ARG;
    }
    if ((rc = prep_check_overlap(frames, n_frames, d_dst, lay.bytes))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    ExtractSlice sl;
    HIP_TRY(hipEventRecord(e->extract_ev[0], e->stream));
    for (size_t first = 0; first < (size_t)n_regions;) {
        const size_t end = extract_slice_end(regions, (size_t)n_regions, first, max_frames);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = enqueue_extract_slice(e, frames, regions, lay, first, end - first, d_dst, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
        first = end;
    }
    HIP_TRY(hipEventRecord(e->extract_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->extract_ev[0], e->extract_ev[1]));
    e->extract_ms = ms;
    return VJ_OK;
}

int vj_extract_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->extract_ms;
    return VJ_OK;
}

}  // extern "C"
