// The HIP half of the frame-processing calls (vj_stage_host.hpp is the byte-moving half): the page-locked staging
// buffer, the checks on a caller's destination, the slices of a call between its two events, and the slice of the calls that paint
// in place.  vj_preprocess, vj_extract, vj_extract_affine, vj_paint, vj_paint_yuv, vj_yuv_to_bgr and vj_bgr_to_yuv run through it.
#pragma once
#include "vj_env_internal.hpp"
#include "vj_stage_host.hpp"

namespace vj {

// lane->h_stage holds at least `bytes` (it grows and is reused; what it held is gone when it grows)
int stage_reserve(Lane* lane, size_t bytes);   // vj_env.cpp

// The destination of a call: dst_bytes holds the layout's `need`, d_dst is a multiple of 4 where the kernels store dwords, and
// overlap(frames, n_frames, d_dst, need) — the planner's check — finds no source frame inside it.
template <typename Frame, typename Overlap>
int check_dst(const char* who, const Frame* frames, int n_frames, const uint8_t* d_dst, uint64_t dst_bytes, uint64_t need, bool dwords, Overlap overlap) {
    if (dst_bytes < need) {
        set_error("%s: dst_bytes %llu is below the %llu bytes the layout needs", who, (unsigned long long)dst_bytes, (unsigned long long)need);
        return VJ_ERR_ARG;
    }
    if (dwords && ((uintptr_t)d_dst & 3u) != 0u) {
        set_error("%s: d_dst must be a multiple of 4", who);
        return VJ_ERR_ARG;
    }
    return overlap(frames, n_frames, d_dst, need);
}

// A call of `total` items in slices: end_of(first) says where the slice that begins at `first` ends, run(first, end) enqueues it.
// The events ev[0], ev[1] lie around all of it and *ms is their time; the call has finished when this returns, also with an error.
template <typename End, typename Run>
int run_slices(vj_env* e, hipEvent_t* ev, float* ms, size_t total, End end_of, Run run) {
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventRecord(ev[0], e->stream));
    for (size_t first = 0; first < total;) {
        const size_t end = end_of(first);
        // (a later slice reuses the staging buffer and the device block: the one before it has finished by then)
        if (first != 0) HIP_TRY(hipStreamSynchronize(e->stream));
        const int rc = run(first, end);
        if (rc) {
            (void)hipStreamSynchronize(e->stream);
            return rc;
        }
        first = end;
    }
    HIP_TRY(hipEventRecord(ev[1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipEventElapsedTime(ms, ev[0], ev[1]));
    return VJ_OK;
}
// ... an end_of for slices of "max_subbatch" items, or all of them in one
inline auto slices_of(const vj_env* e, size_t total) {
    const size_t per = e->max_subbatch > 0 ? (size_t)e->max_subbatch : total;
    return [=](size_t first) { return first + std::min(per, total - first); };
}

// A slice of a call that paints in place: one copy of [records | overlap lists | the rows `spans` touch of the host planes `planes` |
// scratch] into d_extract, launch(block, overlap lists, scratch) — the launches of both phases —, and for host planes one copy back,
// of which only every span is written to the caller's memory.  place(record, address, pitch, first row) tells a record of a staged
// plane where its rows lie; device-resident planes are painted where they lie.
template <typename Rec, typename Place, typename Launch>
int run_paint_slice(vj_env* e, std::vector<Rec>& recs, const std::vector<uint32_t>& overlaps, uint64_t scratch_bytes, std::vector<TouchedRows> planes,
                    std::vector<RowSpan> spans, Place place, Launch launch) {
    const size_t n = recs.size();
    if (n == 0) return VJ_OK;
    StageBlock b;
    b.section(n * sizeof(Rec));
    const size_t ovl_at = b.section(overlaps.size() * sizeof(uint32_t)), rows_at = b.bytes;
    touch_rows(&planes, &spans, &b);
    const size_t up_bytes = b.bytes;
    int rc;
    if ((rc = stage_reserve(&e->lane0, up_bytes))) return rc;
    if ((rc = e->d_extract.ensure((size_t)((uint64_t)up_bytes + scratch_bytes)))) return rc;
    uint8_t* hs = (uint8_t*)e->lane0.h_stage;
    uint8_t* dev = (uint8_t*)e->d_extract.p;
    gather_touched(hs, planes);
    for (size_t i = 0; i < n; ++i)
        if (spans[i].piece >= 0) {
            const TouchedRows& s = planes[(size_t)spans[i].piece];
            place(recs[i], dev + s.at, (uint32_t)s.pitch, s.y0);
        }
    memcpy(hs, recs.data(), n * sizeof(Rec));
    if (!overlaps.empty()) memcpy(hs + ovl_at, overlaps.data(), overlaps.size() * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(dev, hs, up_bytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = launch(dev, (const uint32_t*)(dev + ovl_at), dev + up_bytes))) return rc;
    if (up_bytes != rows_at) {
        HIP_TRY(hipMemcpyAsync(hs + rows_at, dev + rows_at, up_bytes - rows_at, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        scatter_touched(hs, planes, spans);
    }
    return VJ_OK;
}

}  // namespace vj
