// vj_extract_affine: affine-warped regions of the call's frames, all of one size, written into a device buffer of
// the caller's.  The planner (vj_affine_host.cpp) checks the call; here a slice of the call — all of it unless "max_subbatch" is set:
// then runs of affines that name at most that many distinct frames — is one copy (its region records and the host frames it names,
// gathered at a 4-byte pitch in the lane's page-locked staging buffer as vj_extract stages them) and one launch.  Device-resident
// frames are read where they lie.  The device block is vj_extract's (d_extract: it grows and is reused; a call has finished with it
// when it returns).
#include "vj_env_internal.hpp"
#include "vj_affine_host.hpp"
#include "vj_prep_host.hpp"

namespace vj {

namespace {

inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15; }

int enqueue_affine_slice(vj_env* e, const vj_image* frames, const vj_affine* affines, const AffineLayout& lay, size_t first, size_t n,
                         uint8_t* d_dst, AffineSlice* sl) {
    int rc;
    if ((rc = affine_plan_slice(frames, affines, lay, first, n, sl))) return rc;
    const size_t rec_bytes = align16(n * sizeof(AffineRegionDev));
    size_t bytes = rec_bytes;
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
    size_t at = rec_bytes;
    for (int fi : sl->frames) {
        const vj_image& f = frames[fi];
        if (f.on_device) continue;
        const size_t row_bytes = (size_t)f.width * (size_t)image_channels(f), pitch = (row_bytes + 3u) & ~(size_t)3;
        for (int y = 0; y < f.height; ++y) memcpy(hs + at + (size_t)y * pitch, f.data + (size_t)y * (size_t)f.stride, row_bytes);
        for (size_t i = 0; i < n; ++i)
            if (affines[first + i].frame == fi) {
                sl->recs[i].src = dev + at;
                sl->recs[i].stride = (uint32_t)pitch;
            }
        at += pitch * (size_t)f.height;
    }
    memcpy(hs, sl->recs.data(), n * sizeof(AffineRegionDev));
    HIP_TRY(hipMemcpyAsync(e->d_extract.p, hs, bytes, hipMemcpyHostToDevice, e->stream));
    AffineArgs a;
    memset(&a, 0, sizeof(a));
    a.regions = (const AffineRegionDev*)dev;
    a.n_regions = (uint32_t)n;
    a.n_units = sl->n_units;
    a.dst = d_dst;
    a.dst_bytes = lay.bytes;
    a.out_w = lay.out_w;
    a.out_h = lay.out_h;
    a.C = lay.C;
    a.gray = lay.gray ? 1u : 0u;
    a.planar = lay.planar ? 1u : 0u;
    a.rows = lay.rows;
    a.row_bytes = lay.row_bytes;
    const int hrc = launch_affine(a, e->stream);
    if (hrc) {
        set_error("affine launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_extract_affine(vj_env* e, const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                      uint8_t* d_dst, uint64_t dst_bytes) {
    if (!e || !p || n_frames < 0 || n < 0 || (n_frames > 0 && !frames) || (n > 0 && (!affines || !d_dst))) {
        set_error("vj_extract_affine: null argument");
        return VJ_ERR_ARG;
    }
    AffineLayout lay;
    int rc = affine_layout(frames, n_frames, affines, n, p, &lay);
    if (rc) return rc;
    if (n == 0) return VJ_OK;
    if (dst_bytes < lay.bytes) {
        set_error("vj_extract_affine: dst_bytes %llu is below the %llu bytes the layout needs", (unsigned long long)dst_bytes, (unsigned long long)lay.bytes);
        return VJ_ERR_ARG;
    }
    if ((rc = prep_check_overlap(frames, n_frames, d_dst, lay.bytes))) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    AffineSlice sl;
    HIP_TRY(hipEventRecord(e->affine_ev[0], e->stream));
    for (size_t first = 0; first < (size_t)n;) {
        const size_t end = affine_slice_end(affines, (size_t)n, first, max_frames);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = enqueue_affine_slice(e, frames, affines, lay, first, end - first, d_dst, &sl))) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
        first = end;
    }
    HIP_TRY(hipEventRecord(e->affine_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->affine_ev[0], e->affine_ev[1]));
    e->affine_ms = ms;
    return VJ_OK;
}

int vj_extract_affine_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->affine_ms;
    return VJ_OK;
}

}  // extern "C"
