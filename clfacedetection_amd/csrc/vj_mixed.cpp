// vj_detect_mixed, vj_detect_opencv_mixed, vj_pack_frames: batches of frames of differing sizes.  The planner
// (vj_atlas_host.cpp) says which groups of equal frames take a batched call of their own and lays the others out in atlases; here
// an atlas is packed on the device by one launch (vj_atlas.hip) and handed, as ONE device-resident gray frame with one region per
// frame, to the region entry point of the profile — vj_detect_opencv_rois / vj_detect_rois, whose contract ("what the batched call
// returns for the region as a sub-image") is this call's definition.  Both profiles run through one driver.
#include "vj_slice.hpp"
#include "vj_atlas_host.hpp"

#include <functional>

namespace vj {

namespace {

// Packs the atlas `pl` of `frames` into e->d_atlas: one copy brings the frame records and the atlas's host frames (gathered at a
// 4-byte pitch in the lane's page-locked staging buffer, as stage_frames gathers small frames), device-resident frames are read
// where they lie; one launch.  Events e->atlas_ev[0], [1] lie around the launch.  Nothing is waited for.
// equalize (VJ_FLAG_EQUALIZE_HIST): the frames' histograms and look-up tables first, from the same records, and the
// pack applies each frame's table before its store — no second gray copy; the events lie around all of it.
int enqueue_atlas_pack(vj_env* e, const vj_image* frames, const AtlasPlan& pl, bool clear, bool equalize = false) {
    int rc;
    const size_t n = pl.slots.size();
    const size_t atlas_bytes = (size_t)pl.pitch * (size_t)pl.h;
    if ((rc = e->d_atlas.ensure(atlas_bytes))) return rc;
    if (clear) HIP_TRY(hipMemsetAsync(e->d_atlas.p, 0, atlas_bytes, e->stream));
    StageBlock head;
    head.section(n * sizeof(AtlasFrameDev));
    StageBlock b = head;
    for (const AtlasSlot& s : pl.slots) {
        const vj_image& f = frames[s.frame];
        if (!f.on_device) b.rows((size_t)s.w * (size_t)image_channels(f), (size_t)s.h);
    }
    Lane* L = &e->lane0;
    if ((rc = stage_reserve(L, b.bytes))) return rc;
    if ((rc = e->d_atlas_src.ensure(b.bytes))) return rc;
    AtlasFrameDev* recs = (AtlasFrameDev*)L->h_stage;
    b = head;
    uint32_t hist_units = 0;
    for (size_t i = 0; i < n; ++i) {
        const AtlasSlot& s = pl.slots[i];
        const vj_image& f = frames[s.frame];
        const uint32_t ch = (uint32_t)image_channels(f);
        // (the planner's invariants, checked again where the kernel's stores depend on them)
        if ((s.ox & 3u) != 0u || (uint64_t)s.ox + ((s.w + 3u) & ~3u) > pl.w || (uint64_t)s.oy + s.h > pl.h || (pl.pitch & 3u) != 0u || pl.pitch < pl.w) {
            set_error("internal error: frame %d's slot leaves its atlas", s.frame);
            return VJ_ERR_HIP;
        }
        AtlasFrameDev& d = recs[i];
        d = AtlasFrameDev{f.data, (uint32_t)f.stride, ch, s.w, s.h, s.ox, s.oy, s.unit_first, equalize ? hist_units : 0u};
        hist_units += eq_hist_units(s.h);   // (an atlas is lower than 65535 rows)
        if (!f.on_device) {
            const size_t row_bytes = (size_t)s.w * ch;
            d.src = (const uint8_t*)e->d_atlas_src.p + stage_rows((uint8_t*)L->h_stage, &b, f.data, (size_t)f.stride, (size_t)s.h, row_bytes);
            d.stride = (uint32_t)align4(row_bytes);
        }
    }
    HIP_TRY(hipMemcpyAsync(e->d_atlas_src.p, L->h_stage, b.bytes, hipMemcpyHostToDevice, e->stream));
    AtlasPackArgs a{(const AtlasFrameDev*)e->d_atlas_src.p, (uint32_t)n, pl.n_units, (uint8_t*)e->d_atlas.p, pl.pitch, pl.w, pl.h, nullptr};
    HIP_TRY(hipEventRecord(e->atlas_ev[0], e->stream));
    if (equalize && (rc = enqueue_equalize_tables(e, L, e->d_atlas_src.p, (uint32_t)n, hist_units, &a.lut))) return rc;
    const int hrc = launch_atlas_pack(a, e->stream);
    if (hrc) {
        set_error("atlas pack launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    HIP_TRY(hipEventRecord(e->atlas_ev[1], e->stream));
    return VJ_OK;
}

struct MixedRun {
    // the profile's batched call on frames of one size
    std::function<int(const vj_image*, int, vj_result*)> batch;
    // ... and its region call on ONE device-resident gray frame; *windows: the grid positions of that pass
    std::function<int(const vj_image*, const vj_roi*, int, vj_result*, uint64_t*)> rois;
};

int detect_mixed(vj_env* e, const vj_image* frames, int n_frames, const vj_mixed_opts* opts, bool all_own, bool equalize, const MixedRun& run,
                 vj_result* out) {
    e->mixed_info = vj_mixed_info{};
    vj_mixed_info& info = e->mixed_info;
    std::vector<AtlasSize> sizes;
    int rc = atlas_check_frames(frames, n_frames, &sizes);
    if (rc) return rc;
    info.frames = (uint64_t)n_frames;
    if (n_frames == 0) return VJ_OK;
    const uint64_t atlas_px = opts && opts->atlas_px ? opts->atlas_px : ATLAS_DEFAULT_PX;
    const uint64_t own_call_px = opts && opts->own_call_px ? opts->own_call_px : ATLAS_DEFAULT_OWN_CALL_PX;
    AtlasRoute route = atlas_route(sizes, own_call_px, all_own);
    for (const std::vector<int>& g : route.own) info.frames_own_calls += g.size();
    std::vector<vj_rect> all;
    std::vector<int> big;
    // ---- the atlases: pack, then every frame as a region of the one device-resident frame
    if (!route.packed.empty()) HIP_TRY(hipSetDevice(e->device));
    AtlasPlan pl;
    std::vector<vj_roi> rois;
    std::vector<int> idx;
    for (size_t pos = 0; pos < route.packed.size(); pos += pl.n_frames) {
        if ((rc = atlas_plan(sizes, route.packed, pos, atlas_px, e->max_subbatch, &pl))) return rc;
        if (pl.oversized) {
            big.push_back(route.packed[pos]);
            continue;
        }
        if ((rc = enqueue_atlas_pack(e, frames, pl, false, equalize))) return rc;
        rois.clear();
        idx.clear();
        for (const AtlasSlot& s : pl.slots) {
            rois.push_back(vj_roi{0, (int32_t)s.ox, (int32_t)s.oy, (int32_t)s.w, (int32_t)s.h});
            idx.push_back(s.frame);
        }
        const vj_image atlas{(const uint8_t*)e->d_atlas.p, (int32_t)pl.w, (int32_t)pl.h, (int32_t)pl.pitch, 1, 1};
        vj_result part;
        memset(&part, 0, sizeof(part));
        uint64_t windows = 0;
        rc = run.rois(&atlas, rois.data(), (int)rois.size(), &part, &windows);
        if (!rc) rc = cv_roi_take_part(part, idx, &all, out);
        vj_result_free(&part);
        if (rc) return rc;
        HIP_TRY(hipEventSynchronize(e->atlas_ev[1]));   // (the region call has waited for the stream already)
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e->atlas_ev[0], e->atlas_ev[1]));
        info.pack_ms += ms;
        out->timing.integral_ms += ms;   // (image preparation, like the pyramid launch)
        out->timing.total_ms += ms;
        info.atlases += 1;
        info.frames_atlas += pl.n_frames;
        info.windows += windows;
        if ((uint64_t)pl.w * pl.h > (uint64_t)info.atlas_w * info.atlas_h) {
            info.atlas_w = pl.w;
            info.atlas_h = pl.h;
        }
    }
    // ---- batched calls on the original frames: the groups the rule sent there, and the frames too large for an empty atlas
    info.frames_oversized = big.size();
    std::vector<std::vector<int>> own = std::move(route.own);
    for (std::vector<int>& g : atlas_size_groups(sizes, big)) own.push_back(std::move(g));
    std::vector<vj_image> views;
    for (const std::vector<int>& g : own) {
        views.clear();
        for (int i : g) views.push_back(frames[i]);
        vj_result part;
        memset(&part, 0, sizeof(part));
        rc = run.batch(views.data(), (int)views.size(), &part);
        if (!rc) rc = cv_roi_take_part(part, g, &all, out);
        vj_result_free(&part);
        if (rc) return rc;
        info.own_calls += 1;
    }
    // (every part is in its final order and a frame's rectangles all come from one part: only the frames are put in order)
    return cv_roi_emit_parts(all, out);
}

}  // namespace

}  // namespace vj

using namespace vj;

extern "C" {

int vj_detect_opencv_mixed(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_cv_params* p,
                           const vj_mixed_opts* opts, vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (!(p->scale_factor > 1.0)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    // Flags whose result needs the image alone (the edge map of a crop is not the crop of the edge map; the find-biggest search keeps
    // its state per image), and bits vj_detect_opencv does not know: every group on its original frames.  What the atlas route
    // passes on is the flag word as the region call's fast routes know it: rough search means nothing without find-biggest, canny
    // pruning nothing under scale-image, the chain's bit nothing here.  VJ_FLAG_EQUALIZE_HIST: an atlas is packed through its frames'
    // look-up tables and the region call runs without the bit; a batched call of its own takes it as it is.
    const uint32_t known = VJ_FLAG_COUNTERS | VJ_FLAG_CV_CANNY_PRUNING | VJ_FLAG_CV_SCALE_IMAGE | VJ_FLAG_CV_FIND_BIGGEST | VJ_FLAG_CV_ROUGH_SEARCH |
                           VJ_FLAG_CV_CHAIN_DEVICE | VJ_FLAG_EQUALIZE_HIST;
    const bool all_own = (p->flags & VJ_FLAG_CV_FIND_BIGGEST) != 0u || (p->flags & ~known) != 0u ||
                         ((p->flags & VJ_FLAG_CV_CANNY_PRUNING) != 0u && (p->flags & VJ_FLAG_CV_SCALE_IMAGE) == 0u);
    vj_cv_params pr = *p;
    pr.flags &= VJ_FLAG_COUNTERS | VJ_FLAG_CV_SCALE_IMAGE;
    MixedRun run;
    run.batch = [&](const vj_image* f, int n, vj_result* part) { return vj_detect_opencv(e, c, f, n, p, part); };
    run.rois = [&](const vj_image* atlas, const vj_roi* rois, int n, vj_result* part, uint64_t* windows) {
        const int rc = vj_detect_opencv_rois(e, c, atlas, 1, rois, n, &pr, part);
        *windows = e->cv_rois_info.windows;
        return rc;
    };
    return detect_mixed(e, frames, n_frames, opts, all_own, (p->flags & VJ_FLAG_EQUALIZE_HIST) != 0u, run, out);
}

int vj_detect_mixed(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_params* p, const vj_mixed_opts* opts,
                    vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (!(p->scale_factor > 1.0f)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    // the skip modes walk the image's own window list: every group on its original frames (so does a call with the region pass
    // configured off, "rois_on_device" 0: vj_detect_rois would run one call per size on views of the atlas)
    const bool all_own = (p->flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW)) != 0u || !e->rois_on_device;
    // VJ_FLAG_EQUALIZE_HIST: an atlas is packed through its frames' look-up tables and the region call runs without the bit
    vj_params pr = *p;
    pr.flags &= ~(uint32_t)VJ_FLAG_EQUALIZE_HIST;
    MixedRun run;
    run.batch = [&](const vj_image* f, int n, vj_result* part) { return vj_detect(e, c, f, n, p, part); };
    run.rois = [&](const vj_image* atlas, const vj_roi* rois, int n, vj_result* part, uint64_t* windows) {
        *windows = 0;
        for (int i = 0; i < n; ++i) {
            uint64_t w = 0;
            if (vj_count_windows(c, rois[i].w, rois[i].h, &pr, &w) == VJ_OK) *windows += w;
        }
        return vj_detect_rois(e, c, atlas, 1, rois, n, &pr, part);
    };
    return detect_mixed(e, frames, n_frames, opts, all_own, (p->flags & VJ_FLAG_EQUALIZE_HIST) != 0u, run, out);
}

int vj_pack_frames(vj_env* e, const vj_image* frames, int n_frames, uint64_t atlas_px, uint8_t* atlas, int atlas_stride, int* atlas_w,
                   int* atlas_h, int32_t* origins_xy) {
    if (!e || !atlas_w || !atlas_h || n_frames < 0 || (n_frames > 0 && (!frames || !origins_xy))) return VJ_ERR_ARG;
    *atlas_w = *atlas_h = 0;
    std::vector<AtlasSize> sizes;
    int rc = atlas_check_frames(frames, n_frames, &sizes);
    if (rc) return rc;
    for (int i = 0; i < 2 * n_frames; ++i) origins_xy[i] = -1;
    std::vector<int> order((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i) order[(size_t)i] = i;
    AtlasPlan pl;
    size_t pos = 0;
    for (; pos < order.size(); pos += pl.n_frames) {   // (frames too large for an empty atlas are passed over)
        if ((rc = atlas_plan(sizes, order, pos, atlas_px ? atlas_px : ATLAS_DEFAULT_PX, e->max_subbatch, &pl))) return rc;
        if (!pl.oversized) break;
    }
    if (pos >= order.size()) return VJ_OK;
    *atlas_w = (int)pl.w;
    *atlas_h = (int)pl.h;
    for (const AtlasSlot& s : pl.slots) {
        origins_xy[2 * s.frame] = (int32_t)s.ox;
        origins_xy[2 * s.frame + 1] = (int32_t)s.oy;
    }
    if (!atlas) return VJ_OK;
    if (atlas_stride < (int)pl.w) {
        set_error("atlas_stride %d is below the atlas width %u", atlas_stride, pl.w);
        return VJ_ERR_ARG;
    }
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = enqueue_atlas_pack(e, frames, pl, true))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy2D(atlas, (size_t)atlas_stride, e->d_atlas.p, (size_t)pl.pitch, (size_t)pl.w, (size_t)pl.h, hipMemcpyDeviceToHost));
    return VJ_OK;
}

int vj_mixed_info_get(const vj_env* e, vj_mixed_info* out) {
    if (!e || !out) return VJ_ERR_ARG;
    *out = e->mixed_info;
    return VJ_OK;
}

}  // extern "C"
