// Host planner of vj_paint that needs no device: see vj_paint_host.hpp.
#include "vj_paint_host.hpp"
#include "vj_atlas_host.hpp"
#include "vj_cv_roi_host.hpp"   // cv_round
#include "vj_extract_host.hpp"  // extract_map_axis

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vj {

namespace {
inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15; }

// two frames of one kind (host, device) whose byte extents [data, last row's end) meet
int check_frames_disjoint(const vj_image* frames, int n_frames) {
    struct Ext { uintptr_t b, e; int i; };
    for (int dev = 0; dev < 2; ++dev) {
        std::vector<Ext> ext;
        for (int i = 0; i < n_frames; ++i) {
            const vj_image& f = frames[i];
            if ((f.on_device != 0) != (dev != 0)) continue;
            const int ch = f.channels <= 1 ? 1 : f.channels;
            const uintptr_t b = (uintptr_t)f.data;
            ext.push_back(Ext{b, b + (uint64_t)(f.height - 1) * (uint64_t)f.stride + (uint64_t)f.width * (uint64_t)ch, i});
        }
        std::sort(ext.begin(), ext.end(), [](const Ext& a, const Ext& b) { return a.b != b.b ? a.b < b.b : a.i < b.i; });
        // (sorted by start: if any earlier extent reaches past this start, the one with the greatest end does)
        for (size_t k = 1, far = 0; k < ext.size(); ++k) {
            if (ext[far].e > ext[k].b) {
                set_error("frame %d: its memory overlaps frame %d's (vj_paint writes the frames: each must own its bytes)",
                          std::max(ext[far].i, ext[k].i), std::min(ext[far].i, ext[k].i));
                return VJ_ERR_ARG;
            }
            if (ext[k].e > ext[far].e) far = k;
        }
    }
    return VJ_OK;
}
}  // namespace

int paint_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p, PaintLayout* out) {
    *out = PaintLayout{};
    if (!p || n_regions < 0 || (n_regions > 0 && !regions)) {
        set_error("vj_paint: null argument");
        return VJ_ERR_ARG;
    }
    std::vector<AtlasSize> fs;
    const int rc = atlas_check_frames(frames, n_frames, &fs);
    if (rc) {
        if (n_frames < 0 || (n_frames > 0 && !frames)) set_error("vj_paint: null argument");
        return rc;
    }
    if (p->mode < 0 || p->mode > (int32_t)PAINT_BLUR) {
        set_error("vj_paint_params: unknown mode %d", p->mode);
        return VJ_ERR_ARG;
    }
    if ((p->flags & ~(uint32_t)VJ_PAINT_ELLIPSE) != 0u || p->reserved != 0u) {
        set_error("vj_paint_params: %s", p->reserved != 0u ? "reserved must be 0" : "unknown bits in flags");
        return VJ_ERR_ARG;
    }
    if (p->size < 0) {
        set_error("vj_paint_params: size must not be negative");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(p->sx) || !std::isfinite(p->sy) || !std::isfinite(p->margin) || p->sx < 0 || p->sy < 0 || p->margin < 0) {
        set_error("vj_paint_params: %s must be finite and not negative", !std::isfinite(p->sx) || p->sx < 0 ? "sx" : !std::isfinite(p->sy) || p->sy < 0 ? "sy" : "margin");
        return VJ_ERR_ARG;
    }
    if (p->size == 0 && !(std::isfinite(p->rel) && p->rel > 0)) {
        set_error("vj_paint_params: with size 0, rel must be finite and positive");
        return VJ_ERR_ARG;
    }
    int lrc;
    if ((lrc = check_frames_disjoint(frames, n_frames))) return lrc;
    const double sx = p->sx == 0 ? 1.0 : p->sx, sy = p->sy == 0 ? 1.0 : p->sy;
    out->mode = (uint32_t)p->mode;
    out->ellipse = (p->flags & VJ_PAINT_ELLIPSE) != 0u;
    out->color = (uint32_t)p->color[0] | (uint32_t)p->color[1] << 8 | (uint32_t)p->color[2] << 16 | (uint32_t)p->color[3] << 24;
    out->mapped.reserve((size_t)n_regions);
    out->clipped.reserve((size_t)n_regions);
    out->sizes.reserve((size_t)n_regions);
    std::vector<char> touched((size_t)n_frames, 0);
    uint64_t units = 0, pre_units = 0;
    for (int r = 0; r < n_regions; ++r) {
        const vj_roi& g = regions[r];
        if (g.frame < 0 || g.frame >= n_frames) {
            set_error("region %d: frame %d is not one of the call's %d frames", r, g.frame, n_frames);
            return VJ_ERR_ARG;
        }
        if (g.w <= 0 || g.h <= 0) {
            set_error("region %d: w and h must be positive", r);
            return VJ_ERR_ARG;
        }
        vj_roi m;
        m.frame = g.frame;
        if ((lrc = extract_map_axis(r, "x", g.x, g.w, sx, p->margin, &m.x, &m.w))) return lrc;
        if ((lrc = extract_map_axis(r, "y", g.y, g.h, sy, p->margin, &m.y, &m.h))) return lrc;
        if (m.w > PAINT_MAX_SIDE || m.h > PAINT_MAX_SIDE) {
            set_error("region %d: its mapped %s side is above 32767 (the ellipse test's 64-bit products)", r, m.w > PAINT_MAX_SIDE ? "x" : "y");
            return VJ_ERR_LIMIT;
        }
        int32_t s = 0;
        if (out->mode != PAINT_FILL) {
            if (p->size > 0) {
                s = p->size;
            } else {
                const double v = (double)std::min(m.w, m.h) * p->rel;
                s = v <= 65536.0 ? std::max(cv_round(v), 1) : 65536;   // (beyond every limit below; an outline that thick is the whole shape)
            }
            if (out->mode == PAINT_BLUR) {
                s = std::max(s | 1, 3);
                if (s > PAINT_MAX_KK) {
                    set_error("region %d: BLUR's kernel side %d is above 255 (a column sum must fit 16 bits)", r, s);
                    return VJ_ERR_LIMIT;
                }
            } else if (out->mode == PAINT_PIXELATE && s > PAINT_MAX_CELL) {
                set_error("region %d: PIXELATE's cell side %d is above 4096 (a cell sum must fit 32 bits)", r, s);
                return VJ_ERR_LIMIT;
            }
        }
        const AtlasSize& f = fs[(size_t)g.frame];
        const int32_t cx0 = std::max(m.x, 0), cy0 = std::max(m.y, 0);
        const int32_t cx1 = (int32_t)std::min<int64_t>((int64_t)m.x + m.w, f.w), cy1 = (int32_t)std::min<int64_t>((int64_t)m.y + m.h, f.h);
        vj_roi k;
        k.frame = g.frame;
        k.x = k.y = k.w = k.h = 0;
        if (cx1 > cx0 && cy1 > cy0) {
            k.x = cx0, k.y = cy0, k.w = cx1 - cx0, k.h = cy1 - cy0;
            touched[(size_t)g.frame] = 1;
            const uint32_t B = (uint32_t)k.w * (uint32_t)f.ch;
            units += paint_apply_units(B, (uint32_t)k.h);
            if (out->mode == PAINT_BLUR) pre_units += paint_colsum_units(B, (uint32_t)k.h);
            if (out->mode == PAINT_PIXELATE) pre_units += paint_cell_units((uint32_t)k.w, (uint32_t)k.h, (uint32_t)s, paint_cell_lanes((uint32_t)s, (uint32_t)f.ch));
            out->scratch_bytes += align16(paint_scratch_bytes(out->mode, (uint32_t)k.w, (uint32_t)k.h, (uint32_t)f.ch, (uint32_t)s));
            if (units > 0x7fffffffull || pre_units > 0x7fffffffull) {
                set_error("vj_paint: the regions hold more work units than a 32-bit index holds");
                return VJ_ERR_LIMIT;
            }
        }
        out->mapped.push_back(m);
        out->clipped.push_back(k);
        out->sizes.push_back(s);
    }
    for (int i = 0; i < n_frames; ++i)
        if (touched[(size_t)i]) out->touched.push_back(i);
    return VJ_OK;
}

size_t paint_slice_end(const PaintLayout& lay, size_t first, size_t max_frames) {
    const size_t n = lay.touched.size();
    if (max_frames == 0) return n;
    return std::min(n, first + max_frames);
}

int paint_plan_slice(const vj_image* frames, const PaintLayout& lay, size_t first, size_t end, PaintSlice* out) {
    *out = PaintSlice{};
    if (first > end || end > lay.touched.size()) {
        set_error("internal error: a slice beyond the call's frames");
        return VJ_ERR_ARG;
    }
    out->frames.assign(lay.touched.begin() + (ptrdiff_t)first, lay.touched.begin() + (ptrdiff_t)end);
    // the regions bucketed by frame, stable: (frame, region index) ascending
    std::vector<int> order;
    for (size_t r = 0; r < lay.clipped.size(); ++r) {
        const vj_roi& k = lay.clipped[r];
        if (k.w > 0 && k.h > 0 && std::binary_search(out->frames.begin(), out->frames.end(), k.frame)) order.push_back((int)r);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lay.clipped[(size_t)a].frame < lay.clipped[(size_t)b].frame; });
    uint64_t unit = 0, pre = 0, scratch = 0;
    out->recs.reserve(order.size());
    for (int r : order) {
        const vj_roi &k = lay.clipped[(size_t)r], &m = lay.mapped[(size_t)r];
        const vj_image& f = frames[k.frame];
        PaintRegionDev d;
        memset(&d, 0, sizeof(d));
        d.frame = const_cast<uint8_t*>(f.data);
        d.stride = (uint32_t)f.stride;
        d.channels = (uint32_t)(f.channels <= 1 ? 1 : f.channels);
        d.fw = f.width, d.fh = f.height;
        d.X0 = m.x, d.Y0 = m.y, d.Wm = m.w, d.Hm = m.h;
        d.cx0 = k.x, d.cy0 = k.y, d.cx1 = k.x + k.w, d.cy1 = k.y + k.h;
        d.size = lay.sizes[(size_t)r];
        d.row0 = 0;
        d.unit_first = (uint32_t)unit;
        d.pre_first = (uint32_t)pre;
        d.scratch_off = scratch;
        const uint32_t B = (uint32_t)k.w * d.channels;
        unit += paint_apply_units(B, (uint32_t)k.h);
        if (lay.mode == PAINT_BLUR) pre += paint_colsum_units(B, (uint32_t)k.h);
        if (lay.mode == PAINT_PIXELATE) {
            d.lanes = paint_cell_lanes((uint32_t)d.size, d.channels);
            pre += paint_cell_units((uint32_t)k.w, (uint32_t)k.h, (uint32_t)d.size, d.lanes);
        }
        scratch += align16(paint_scratch_bytes(lay.mode, (uint32_t)k.w, (uint32_t)k.h, d.channels, (uint32_t)d.size));
        if (unit > 0x7fffffffull || pre > 0x7fffffffull) {
            set_error("vj_paint: the regions hold more work units than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
        out->recs.push_back(d);
        out->region.push_back(r);
    }
    // the overlap lists: for every record the later records of its frame whose K meets its own
    for (size_t i = 0; i < out->recs.size(); ++i) {
        PaintRegionDev& a = out->recs[i];
        a.ovl_first = (uint32_t)out->overlaps.size();
        for (size_t j = i + 1; j < out->recs.size() && lay.clipped[(size_t)out->region[j]].frame == lay.clipped[(size_t)out->region[i]].frame; ++j) {
            const PaintRegionDev& b = out->recs[j];
            if (a.cx0 < b.cx1 && b.cx0 < a.cx1 && a.cy0 < b.cy1 && b.cy0 < a.cy1) out->overlaps.push_back((uint32_t)j);
        }
        if ((out->overlaps.size() >> 32) != 0u) {
            set_error("vj_paint: the regions' overlap lists hold more entries than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
        a.ovl_count = (uint32_t)out->overlaps.size() - a.ovl_first;
    }
    out->n_units = (uint32_t)unit;
    out->n_pre_units = (uint32_t)pre;
    out->scratch_bytes = scratch;
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

void vj_paint_default(vj_paint_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->mode = VJ_PAINT_BLUR;
    p->sx = p->sy = 1.0;
    p->rel = 0.25;
}

int vj_paint_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                    vj_roi* clipped, int32_t* sizes, uint64_t* scratch_bytes) {
    if (!p || !scratch_bytes || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && (!regions || !clipped || !sizes))) {
        set_error("vj_paint_layout: null argument");
        return VJ_ERR_ARG;
    }
    *scratch_bytes = 0;
    PaintLayout lay;
    const int rc = paint_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    for (int r = 0; r < n_regions; ++r) {
        clipped[r] = lay.clipped[(size_t)r];
        sizes[r] = lay.sizes[(size_t)r];
    }
    *scratch_bytes = lay.scratch_bytes;
    return VJ_OK;
}

}  // extern "C"
