// Host planner of vj_track that needs no device: see vj_track_host.hpp.
#include "vj_track_host.hpp"
#include "vj_cv_roi_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vj {

namespace {
inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15; }
}  // namespace

int track_layout(const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows, const vj_track_params* p, TrackLayout* out) {
    *out = TrackLayout{};
    if (!p || n_frames < 0 || n_rows < 0 || (n_frames > 0 && !frames) || (n_rows > 0 && !rows)) {
        set_error("vj_track: null argument");
        return VJ_ERR_ARG;
    }
    if (p->tmpl < (int32_t)TRACK_TMPL_MIN || p->tmpl > (int32_t)TRACK_TMPL_MAX || (p->tmpl & 3) != 0) {
        set_error("vj_track_params: tmpl %d must be a multiple of 4 in %u .. %u", p->tmpl, TRACK_TMPL_MIN, TRACK_TMPL_MAX);
        return VJ_ERR_ARG;
    }
    if (p->radius < (int32_t)TRACK_RADIUS_MIN || p->radius > (int32_t)TRACK_RADIUS_MAX) {
        set_error("vj_track_params: radius %d must lie in %u .. %u", p->radius, TRACK_RADIUS_MIN, TRACK_RADIUS_MAX);
        return VJ_ERR_ARG;
    }
    if (p->flags != 0u || p->reserved != 0u) {
        set_error("vj_track_params: %s must be 0", p->flags != 0u ? "flags" : "reserved");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(p->sx) || !std::isfinite(p->sy) || p->sx < 0 || p->sy < 0) {
        set_error("vj_track_params: %s must be finite and not negative", !std::isfinite(p->sx) || p->sx < 0 ? "sx" : "sy");
        return VJ_ERR_ARG;
    }
    out->t = (uint32_t)p->tmpl;
    out->r = (uint32_t)p->radius;
    out->tmpl_regions.reserve((size_t)n_rows);
    out->search_regions.reserve((size_t)n_rows);
    for (int k = 0; k < n_rows; ++k) {
        const vj_track_row& w = rows[k];
        if (w.src_frame < 0 || w.src_frame >= n_frames || w.dst_frame < 0 || w.dst_frame >= n_frames) {
            const bool src = w.src_frame < 0 || w.src_frame >= n_frames;
            set_error("row %d: %s %d is not one of the call's %d frames", k, src ? "src_frame" : "dst_frame", src ? w.src_frame : w.dst_frame, n_frames);
            return VJ_ERR_ARG;
        }
        out->tmpl_regions.push_back(vj_roi{w.src_frame, w.x, w.y, w.w, w.h});
        out->search_regions.push_back(vj_roi{w.dst_frame, w.x, w.y, w.w, w.h});
    }
    vj_extract_params ep;
    memset(&ep, 0, sizeof(ep));
    ep.out_w = ep.out_h = p->tmpl;
    ep.sx = p->sx;
    ep.sy = p->sy;
    ep.margin = 0.0;
    ep.flags = VJ_EXTRACT_GRAY;
    int rc;
    if ((rc = extract_layout(frames, n_frames, out->tmpl_regions.data(), n_rows, &ep, &out->tmpl))) return rc;
    ep.out_w = ep.out_h = p->tmpl + 2 * p->radius;
    ep.margin = (double)p->radius / (double)p->tmpl;
    if ((rc = extract_layout(frames, n_frames, out->search_regions.data(), n_rows, &ep, &out->search))) return rc;
    // every search patch at a multiple of 16 bytes (t * t is one already)
    out->search.region_pitch = align16(out->search.region_bytes);
    out->search.bytes = out->search.region_pitch * (uint64_t)n_rows;
    out->tmpl_off = 0;
    out->search_off = out->tmpl.bytes;
    out->scratch_bytes = out->tmpl.bytes + out->search.bytes;
    return VJ_OK;
}

size_t track_slice_end(const vj_track_row* rows, size_t n_rows, size_t first, size_t max_frames) {
    if (max_frames == 0) return n_rows;
    std::vector<int> seen;
    size_t k = first;
    for (; k < n_rows; ++k) {
        const int f[2] = {rows[k].src_frame, rows[k].dst_frame};
        size_t fresh = 0;
        for (int q = 0; q < 2; ++q)
            if (std::find(seen.begin(), seen.end(), f[q]) == seen.end() && (q == 0 || f[1] != f[0])) ++fresh;
        if (seen.size() + fresh > max_frames) break;
        for (int q = 0; q < 2; ++q)
            if (std::find(seen.begin(), seen.end(), f[q]) == seen.end()) seen.push_back(f[q]);
    }
    return std::max(k, std::min(first + 1, n_rows));
}

void track_result(const TrackLayout& lay, size_t k, const TrackMatchDev& m, vj_track_result* out) {
    const vj_roi& b = lay.tmpl.src[k];      // (x0, y0, w0, h0): the mapping does not look at the frame
    const vj_roi& s = lay.search.src[k];    // (X, Y, Wm, Hm)
    const double side = (double)(lay.t + 2u * lay.r);
    out->dx = m.dx;
    out->dy = m.dy;
    out->sad = m.sad;
    out->sad0 = m.sad0;
    out->x = b.x + cv_round((double)m.dx * (double)s.w / side);
    out->y = b.y + cv_round((double)m.dy * (double)s.h / side);
    out->w = b.w;
    out->h = b.h;
}

}  // namespace vj

using namespace vj;

extern "C" {

void vj_track_default(vj_track_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->tmpl = 32;
    p->radius = 8;
}

int vj_track_layout(const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows, const vj_track_params* p,
                    vj_roi* tmpl_regions, vj_roi* search_regions, uint64_t* scratch_bytes) {
    if (scratch_bytes) *scratch_bytes = 0;
    if (!p || !scratch_bytes || n_frames < 0 || n_rows < 0 || (n_frames > 0 && !frames) || (n_rows > 0 && (!rows || !tmpl_regions || !search_regions))) {
        set_error("vj_track_layout: null argument");
        return VJ_ERR_ARG;
    }
    *scratch_bytes = 0;
    TrackLayout lay;
    const int rc = track_layout(frames, n_frames, rows, n_rows, p, &lay);
    if (rc) return rc;
    for (int k = 0; k < n_rows; ++k) {
        tmpl_regions[k] = lay.tmpl.src[(size_t)k];
        search_regions[k] = lay.search.src[(size_t)k];
    }
    *scratch_bytes = lay.scratch_bytes;
    return VJ_OK;
}

}  // extern "C"
