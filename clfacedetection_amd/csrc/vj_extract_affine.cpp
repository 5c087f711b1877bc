// vj_extract_affine: affine-warped regions of the call's frames, all of one size, written into a device buffer of
// the caller's.  The planner (vj_affine_host.cpp) checks the call; here a slice of the call — all of it unless "max_subbatch" is set:
// then runs of affines that name at most that many distinct frames — is one copy (its region records and the host frames it names,
// gathered at a 4-byte pitch in the lane's page-locked staging buffer) and one launch.  Device-resident frames are read where they
// lie.  The device block is vj_extract's (d_extract: it grows and is reused; a call has finished with it when it returns), the
// call's skeleton the shared one (vj_slice.hpp, §4.24).
#include "vj_slice.hpp"
#include "vj_affine_host.hpp"
#include "vj_prep_host.hpp"

namespace vj {

namespace {

int enqueue_affine_slice(vj_env* e, const vj_image* frames, const vj_affine* affines, const AffineLayout& lay, size_t first, size_t n,
                         uint8_t* d_dst, AffineSlice* sl) {
    int rc;
    if ((rc = affine_plan_slice(frames, affines, lay, first, n, sl))) return rc;
    StageBlock head;
    head.section(n * sizeof(AffineRegionDev));
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
            if (affines[first + i].frame == fi) {
                sl->recs[i].src = dev + at;
                sl->recs[i].stride = (uint32_t)align4(row_bytes);
            }
    }
    memcpy(hs, sl->recs.data(), n * sizeof(AffineRegionDev));
    HIP_TRY(hipMemcpyAsync(e->d_extract.p, hs, b.bytes, hipMemcpyHostToDevice, e->stream));
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
    if ((rc = check_dst("vj_extract_affine", frames, n_frames, d_dst, dst_bytes, lay.bytes, false, prep_check_overlap))) return rc;
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    AffineSlice sl;
    return run_slices(
        e, e->call_ev, &e->affine_ms, (size_t)n, [&](size_t first) { return affine_slice_end(affines, (size_t)n, first, max_frames); },
        [&](size_t first, size_t end) { return enqueue_affine_slice(e, frames, affines, lay, first, end - first, d_dst, &sl); });
}

int vj_extract_affine_timing(const vj_env* e, float* ms) {
    if (!e || !ms) return VJ_ERR_ARG;
    *ms = e->affine_ms;
    return VJ_OK;
}

}  // extern "C"
