// vj_track: block matching of the boxes of one frame in another.  The planner (vj_track_host.cpp) checks the call
// and lays it out as two vj_extract calls; here a slice of the call — all rows unless "max_subbatch" is set: then runs of rows that
// name at most that many distinct frames — is vj_extract's slice routine twice (the templates, then the search patches, into the
// environment's scratch d_track: [templates | search patches | match records]) and the match launch; one copy brings the records
// of all rows back, and the host adds the boxes.  The two extractions share vj_extract's staging buffer and device block, so the
// second waits for the first.
#include "vj_env_internal.hpp"
#include "vj_track_host.hpp"

#include <vector>

using namespace vj;

extern "C" {

int vj_track(vj_env* e, const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows, const vj_track_params* p,
             vj_track_result* out) {
    if (!e || !p || n_frames < 0 || n_rows < 0 || (n_frames > 0 && !frames) || (n_rows > 0 && (!rows || !out))) {
        set_error("vj_track: null argument");
        return VJ_ERR_ARG;
    }
    TrackLayout lay;
    int rc = track_layout(frames, n_frames, rows, n_rows, p, &lay);
    if (rc) return rc;
    if (n_rows == 0) return VJ_OK;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n = (size_t)n_rows;
    const uint64_t total = lay.scratch_bytes + (uint64_t)n * sizeof(TrackMatchDev);
    if ((rc = e->d_track.ensure((size_t)total))) {
        if (rc == VJ_ERR_NOMEM) set_error("vj_track: no device memory for the %llu bytes of its patches and results", (unsigned long long)total);
        return rc;
    }
    uint8_t* dev = (uint8_t*)e->d_track.p;
    TrackArgs a;
    memset(&a, 0, sizeof(a));
    a.tmpl = dev + lay.tmpl_off;
    a.search = dev + lay.search_off;
    a.out = (TrackMatchDev*)(dev + lay.scratch_bytes);   // (scratch_bytes is a multiple of 16)
    a.search_pitch = lay.search.region_pitch;
    a.t = lay.t;
    a.r = lay.r;
    const size_t max_frames = e->max_subbatch > 0 ? (size_t)e->max_subbatch : 0;
    ExtractSlice sl;
    float match_ms = 0;
    bool pending = false;   // a match launch between track_ev[2] and [3] whose time has not been read
    auto fail = [&](int code) {
        (void)hipStreamSynchronize(e->stream);
        return code;
    };
    HIP_TRY(hipEventRecord(e->track_ev[0], e->stream));
    for (size_t first = 0; first < n;) {
        const size_t end = track_slice_end(rows, n, first, max_frames);
        if (first != 0) {
            // (a later slice reuses the staging buffer, the device block and the two match events)
            HIP_TRY(hipStreamSynchronize(e->stream));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e->track_ev[2], e->track_ev[3]));
            match_ms += ms;
            pending = false;
        }
        if ((rc = enqueue_extract_slice(e, frames, lay.tmpl_regions.data(), lay.tmpl, first, end - first, dev + lay.tmpl_off, &sl))) return fail(rc);
        HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = enqueue_extract_slice(e, frames, lay.search_regions.data(), lay.search, first, end - first, dev + lay.search_off, &sl))) return fail(rc);
        a.first = (uint32_t)first;
        a.n = (uint32_t)(end - first);
        HIP_TRY(hipEventRecord(e->track_ev[2], e->stream));
        const int hrc = launch_track(a, e->stream);
        if (hrc) {
            set_error("track launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return fail(VJ_ERR_HIP);
        }
        HIP_TRY(hipEventRecord(e->track_ev[3], e->stream));
        pending = true;
        first = end;
    }
    std::vector<TrackMatchDev> got(n);
    HIP_TRY(hipMemcpyAsync(got.data(), a.out, n * sizeof(TrackMatchDev), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipEventRecord(e->track_ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    float ms = 0;
    if (pending) {
        HIP_TRY(hipEventElapsedTime(&ms, e->track_ev[2], e->track_ev[3]));
        match_ms += ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, e->track_ev[0], e->track_ev[1]));
    e->track_ms = ms;
    e->track_match_ms = match_ms;
    for (size_t k = 0; k < n; ++k) track_result(lay, k, got[k], out + k);
    return VJ_OK;
}

int vj_track_timing(const vj_env* e, float* ms, float* match_ms) {
    if (!e || !ms || !match_ms) return VJ_ERR_ARG;
    *ms = e->track_ms;
    *match_ms = e->track_match_ms;
    return VJ_OK;
}

}  // extern "C"
