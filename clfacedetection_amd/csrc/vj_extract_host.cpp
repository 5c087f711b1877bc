// Host planner of vj_extract that needs no device: see vj_extract_host.hpp.
#include "vj_extract_host.hpp"
#include "vj_atlas_host.hpp"
#include "vj_cv_roi_levels_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>

namespace vj {

namespace {
constexpr double COORD_MAX = 16777216.0;   // 2^24

// one axis of a region: origin o and length len times factor f, then the margin -> the crop's origin and length
int map_axis(int r, const char* axis, int o, int len, double f, double margin, int32_t* c0, int32_t* clen) {
    const double vo = (double)o * f, vl = (double)len * f;
    if (!(std::fabs(vo) <= COORD_MAX)) {
        set_error("region %d: its mapped %s lies beyond +-2^24", r, axis);
        return VJ_ERR_LIMIT;
    }
    if (!(vl <= 65536.0)) {
        set_error("region %d: its mapped %s side is above 65535 (the taps' 16-bit indices)", r, axis);
        return VJ_ERR_LIMIT;
    }
    const int o0 = cv_round(vo), l0 = std::max(cv_round(vl), 1);
    const double vm = (double)l0 * margin;
    if (!(vm <= 65536.0) || (int64_t)l0 + 2 * (int64_t)cv_round(vm) > 65535) {
        set_error("region %d: its mapped %s side is above 65535 (the taps' 16-bit indices)", r, axis);
        return VJ_ERR_LIMIT;
    }
    const int m = cv_round(vm);
    *c0 = o0 - m;
    *clen = l0 + 2 * m;
    if (std::abs((int64_t)*c0) > (int64_t)COORD_MAX || std::abs((int64_t)*c0 + *clen) > (int64_t)COORD_MAX) {
        set_error("region %d: its mapped %s lies beyond +-2^24", r, axis);
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}
}  // namespace

int extract_map_axis(int r, const char* axis, int o, int len, double f, double margin, int32_t* c0, int32_t* clen) {
    return map_axis(r, axis, o, len, f, margin, c0, clen);
}

int extract_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p, ExtractLayout* out) {
    *out = ExtractLayout{};
    if (!p || n_regions < 0 || (n_regions > 0 && !regions)) {
        set_error("vj_extract: null argument");
        return VJ_ERR_ARG;
    }
    std::vector<AtlasSize> sizes;
    const int rc = atlas_check_frames(frames, n_frames, &sizes);
    if (rc) {
        if (n_frames < 0 || (n_frames > 0 && !frames)) set_error("vj_extract: null argument");
        return rc;
    }
    if ((p->flags & ~(uint32_t)(VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR)) != 0u || p->reserved != 0u) {
        set_error("vj_extract_params: %s", p->reserved != 0u ? "reserved must be 0" : "unknown bits in flags");
        return VJ_ERR_ARG;
    }
    if (p->out_w <= 0 || p->out_h <= 0) {
        set_error("vj_extract_params: out_w and out_h must be positive");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(p->sx) || !std::isfinite(p->sy) || !std::isfinite(p->margin) || p->sx < 0 || p->sy < 0 || p->margin < 0) {
        set_error("vj_extract_params: %s must be finite and not negative", !std::isfinite(p->sx) || p->sx < 0 ? "sx" : !std::isfinite(p->sy) || p->sy < 0 ? "sy" : "margin");
        return VJ_ERR_ARG;
    }
    if (p->out_w > 65535 || p->out_h > 65535) {
        set_error("vj_extract_params: out_w and out_h up to 65535 (the taps' 16-bit indices)");
        return VJ_ERR_LIMIT;
    }
    const double sx = p->sx == 0 ? 1.0 : p->sx, sy = p->sy == 0 ? 1.0 : p->sy;
    out->gray = (p->flags & VJ_EXTRACT_GRAY) != 0u;
    out->planar = (p->flags & VJ_EXTRACT_PLANAR) != 0u;
    out->out_w = (uint32_t)p->out_w;
    out->out_h = (uint32_t)p->out_h;
    out->src.reserve((size_t)n_regions);
    int ch = 0, ch_row = -1;
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
        vj_roi s;
        s.frame = g.frame;
        int lrc;
        if ((lrc = map_axis(r, "x", g.x, g.w, sx, p->margin, &s.x, &s.w))) return lrc;
        if ((lrc = map_axis(r, "y", g.y, g.h, sy, p->margin, &s.y, &s.h))) return lrc;
        const int fch = sizes[(size_t)g.frame].ch;
        if (ch_row < 0) {
            ch = fch;
            ch_row = r;
        } else if (!out->gray && fch != ch) {
            set_error("region %d: its frame has %d channels, region %d's has %d (VJ_EXTRACT_GRAY takes mixed frames)", r, fch, ch_row, ch);
            return VJ_ERR_ARG;
        }
        out->src.push_back(s);
    }
    if (ch_row < 0) ch = n_frames > 0 ? sizes[0].ch : 1;
    out->C = out->gray ? 1u : (uint32_t)ch;
    out->rows = out->planar ? out->C * out->out_h : out->out_h;
    out->row_bytes = out->planar ? out->out_w : out->out_w * out->C;
    out->region_bytes = (uint64_t)out->rows * out->row_bytes;
    out->region_pitch = out->region_bytes;
    out->bytes = out->region_pitch * (uint64_t)n_regions;
    if (extract_units(out->row_bytes, out->rows) * (uint64_t)n_regions > 0x7fffffffull) {
        set_error("vj_extract: the regions hold more work units than a 32-bit index holds");
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}

size_t extract_slice_end(const vj_roi* regions, size_t n_regions, size_t first, size_t max_frames) {
    if (max_frames == 0) return n_regions;
    std::vector<int> seen;
    size_t k = first;
    for (; k < n_regions; ++k) {
        if (std::find(seen.begin(), seen.end(), regions[k].frame) != seen.end()) continue;
        if (seen.size() == max_frames) break;
        seen.push_back(regions[k].frame);
    }
    return std::max(k, std::min(first + 1, n_regions));
}

int extract_plan_slice(const vj_image* frames, const vj_roi* regions, const ExtractLayout& lay, size_t first, size_t n, ExtractSlice* out) {
    out->recs.clear();
    out->taps.clear();
    out->frames.clear();
    out->n_units = 0;
    if (first + n > lay.src.size()) {
        set_error("internal error: a slice beyond the call's regions");
        return VJ_ERR_ARG;
    }
    std::map<std::tuple<uint32_t, uint32_t, bool, bool>, uint32_t> runs;
    auto run_of = [&](uint32_t src, uint32_t dst, bool rows, bool area) {
        const auto key = std::make_tuple(src, dst, rows, area);
        const auto it = runs.find(key);
        if (it != runs.end()) return it->second;
        const uint32_t at = (uint32_t)out->taps.size();
        out->taps.resize((size_t)at + dst);
        build_taps((int)src, (int)dst, rows, area, out->taps.data() + at);
        runs.emplace(key, at);
        return at;
    };
    const uint64_t per_region = extract_units(lay.row_bytes, lay.rows);
    uint64_t unit = 0;
    out->recs.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const vj_roi& s = lay.src[first + i];
        const vj_image& f = frames[regions[first + i].frame];
        if (std::find(out->frames.begin(), out->frames.end(), s.frame) == out->frames.end()) out->frames.push_back(s.frame);
        ExtractRegionDev d;
        memset(&d, 0, sizeof(d));
        d.src = f.data;
        d.dst_off = (uint64_t)(first + i) * lay.region_pitch;
        d.stride = (uint32_t)f.stride;
        d.channels = (uint32_t)(f.channels <= 1 ? 1 : f.channels);
        d.fw = f.width;
        d.fh = f.height;
        d.x0 = s.x;
        d.y0 = s.y;
        d.cw = (uint32_t)s.w;
        d.ch = (uint32_t)s.h;
        if (d.cw == lay.out_w && d.ch == lay.out_h) {   // vj_resize_linear to the crop's own size is the identity
            d.mode = EXTRACT_COPY;
        } else {
            const bool area = resize_is_area((int)d.cw, (int)d.ch, (int)lay.out_w, (int)lay.out_h) && d.cw == 2u * lay.out_w && d.ch == 2u * lay.out_h;
            d.mode = area ? EXTRACT_AREA : EXTRACT_BILINEAR;
            d.xtab = run_of(d.cw, lay.out_w, false, area);
            d.ytab = run_of(d.ch, lay.out_h, true, area);
        }
        d.unit_first = (uint32_t)unit;
        unit += per_region;
        if (unit > 0x7fffffffull || (out->taps.size() >> 32) != 0u) {
            set_error("vj_extract: the regions hold more work units than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
        out->recs.push_back(d);
    }
    out->n_units = (uint32_t)unit;
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

void vj_extract_default(vj_extract_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->sx = p->sy = 1.0;
}

int vj_extract_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                      vj_roi* src_regions, int* channels, uint64_t* bytes) {
    if (!p || !channels || !bytes || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && (!regions || !src_regions))) {
        set_error("vj_extract_layout: null argument");
        return VJ_ERR_ARG;
    }
    *channels = 0;
    *bytes = 0;
    ExtractLayout lay;
    const int rc = extract_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    for (int r = 0; r < n_regions; ++r) src_regions[r] = lay.src[(size_t)r];
    *channels = (int)lay.C;
    *bytes = lay.bytes;
    return VJ_OK;
}

}  // extern "C"
