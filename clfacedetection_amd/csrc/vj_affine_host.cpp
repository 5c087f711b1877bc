// Host planner of vj_extract_affine that needs no device: see vj_affine_host.hpp.
#include "vj_affine_host.hpp"
#include "vj_atlas_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vj {

int32_t affine_rne(double v) { return (int32_t)std::nearbyint(v); }   // (the default rounding mode: to nearest, ties to even)

int affine_layout(const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p, AffineLayout* out) {
    *out = AffineLayout{};
    if (!p || n < 0 || (n > 0 && !affines)) {
        set_error("vj_extract_affine: null argument");
        return VJ_ERR_ARG;
    }
    std::vector<AtlasSize> sizes;
    const int rc = atlas_check_frames(frames, n_frames, &sizes);
    if (rc) {
        if (n_frames < 0 || (n_frames > 0 && !frames)) set_error("vj_extract_affine: null argument");
        return rc;
    }
    if ((p->flags & ~(uint32_t)(VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR)) != 0u || p->reserved != 0u) {
        set_error("vj_affine_params: %s", p->reserved != 0u ? "reserved must be 0" : "unknown bits in flags");
        return VJ_ERR_ARG;
    }
    if (p->out_w <= 0 || p->out_h <= 0) {
        set_error("vj_affine_params: out_w and out_h must be positive");
        return VJ_ERR_ARG;
    }
    if (p->out_w > 65535 || p->out_h > 65535) {
        set_error("vj_affine_params: out_w and out_h up to 65535");
        return VJ_ERR_LIMIT;
    }
    out->gray = (p->flags & VJ_EXTRACT_GRAY) != 0u;
    out->planar = (p->flags & VJ_EXTRACT_PLANAR) != 0u;
    out->out_w = (uint32_t)p->out_w;
    out->out_h = (uint32_t)p->out_h;
    const double xl = (double)(p->out_w - 1), yl = (double)(p->out_h - 1);
    int ch = 0, ch_row = -1;
    for (int r = 0; r < n; ++r) {
        const vj_affine& g = affines[r];
        if (g.frame < 0 || g.frame >= n_frames) {
            set_error("affine %d: frame %d is not one of the call's %d frames", r, g.frame, n_frames);
            return VJ_ERR_ARG;
        }
        if (g.reserved != 0) {
            set_error("affine %d: reserved must be 0", r);
            return VJ_ERR_ARG;
        }
        for (int i = 0; i < 6; ++i)
            if (!std::isfinite(g.m[i])) {
                set_error("affine %d: m[%d] is not finite", r, i);
                return VJ_ERR_ARG;
            }
        // the same f64 expressions as the kernel's row terms; they are monotone in y, so the two ends bound every row
        const double lim[6] = {std::fabs(g.m[0]) * xl, std::fabs(g.m[3]) * xl, std::fabs(g.m[1] * 0.0 + g.m[2]), std::fabs(g.m[1] * yl + g.m[2]),
                               std::fabs(g.m[4] * 0.0 + g.m[5]), std::fabs(g.m[4] * yl + g.m[5])};
        static const char* const what[6] = {"|m[0]| (out_w - 1)", "|m[3]| (out_w - 1)", "|m[2]|", "|m[1] (out_h - 1) + m[2]|", "|m[5]|", "|m[4] (out_h - 1) + m[5]|"};
        for (int i = 0; i < 6; ++i)
            if (!(lim[i] <= AFFINE_COORD_MAX)) {
                set_error("affine %d: %s is above 2^19 (the fixed-point positions' 32 bits)", r, what[i]);
                return VJ_ERR_LIMIT;
            }
        const int fch = sizes[(size_t)g.frame].ch;
        if (ch_row < 0) {
            ch = fch;
            ch_row = r;
        } else if (!out->gray && fch != ch) {
            set_error("affine %d: its frame has %d channels, affine %d's has %d (VJ_EXTRACT_GRAY takes mixed frames)", r, fch, ch_row, ch);
            return VJ_ERR_ARG;
        }
    }
    if (ch_row < 0) ch = n_frames > 0 ? sizes[0].ch : 1;
    out->C = out->gray ? 1u : (uint32_t)ch;
    out->rows = out->planar ? out->C * out->out_h : out->out_h;
    out->row_bytes = out->planar ? out->out_w : out->out_w * out->C;
    out->region_bytes = (uint64_t)out->rows * out->row_bytes;
    out->bytes = out->region_bytes * (uint64_t)n;
    if (extract_units(out->row_bytes, out->rows) * (uint64_t)n > 0x7fffffffull) {
        set_error("vj_extract_affine: the regions hold more work units than a 32-bit index holds");
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}

size_t affine_slice_end(const vj_affine* affines, size_t n, size_t first, size_t max_frames) {
    if (max_frames == 0) return n;
    std::vector<int> seen;
    size_t k = first;
    for (; k < n; ++k) {
        if (std::find(seen.begin(), seen.end(), affines[k].frame) != seen.end()) continue;
        if (seen.size() == max_frames) break;
        seen.push_back(affines[k].frame);
    }
    return std::max(k, std::min(first + 1, n));
}

int affine_plan_slice(const vj_image* frames, const vj_affine* affines, const AffineLayout& lay, size_t first, size_t n, AffineSlice* out) {
    out->recs.clear();
    out->frames.clear();
    out->n_units = 0;
    const uint64_t per_region = extract_units(lay.row_bytes, lay.rows);
    if (lay.region_bytes == 0 || (first + n) * lay.region_bytes > lay.bytes) {
        set_error("internal error: a slice beyond the call's affines");
        return VJ_ERR_ARG;
    }
    uint64_t unit = 0;
    out->recs.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const vj_affine& g = affines[first + i];
        const vj_image& f = frames[g.frame];
        if (std::find(out->frames.begin(), out->frames.end(), g.frame) == out->frames.end()) out->frames.push_back(g.frame);
        AffineRegionDev d;
        memset(&d, 0, sizeof(d));
        d.src = f.data;
        d.dst_off = (uint64_t)(first + i) * lay.region_bytes;
        d.stride = (uint32_t)f.stride;
        d.channels = (uint32_t)(f.channels <= 1 ? 1 : f.channels);
        d.fw = f.width;
        d.fh = f.height;
        for (int k = 0; k < 6; ++k) d.m[k] = g.m[k];
        d.unit_first = (uint32_t)unit;
        unit += per_region;
        if (unit > 0x7fffffffull) {
            set_error("vj_extract_affine: the regions hold more work units than a 32-bit index holds");
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

void vj_affine_default(vj_affine_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
}

int vj_extract_affine_layout(const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                             int* channels, uint64_t* bytes) {
    if (!p || !channels || !bytes || n_frames < 0 || n < 0 || (n_frames > 0 && !frames) || (n > 0 && !affines)) {
        set_error("vj_extract_affine_layout: null argument");
        return VJ_ERR_ARG;
    }
    *channels = 0;
    *bytes = 0;
    AffineLayout lay;
    const int rc = affine_layout(frames, n_frames, affines, n, p, &lay);
    if (rc) return rc;
    *channels = (int)lay.C;
    *bytes = lay.bytes;
    return VJ_OK;
}

int vj_affine_from_rect(double x, double y, double w, double h, int out_w, int out_h, double m[6]) {
    if (!m) {
        set_error("vj_affine_from_rect: null argument");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(w) || !std::isfinite(h) || !(w > 0) || !(h > 0) || out_w <= 0 || out_h <= 0) {
        set_error("vj_affine_from_rect: x, y, w, h must be finite, w, h, out_w and out_h positive");
        return VJ_ERR_ARG;
    }
    m[0] = w / out_w;
    m[1] = 0.0;
    m[2] = x + 0.5 * w / out_w - 0.5;
    m[3] = 0.0;
    m[4] = h / out_h;
    m[5] = y + 0.5 * h / out_h - 0.5;
    return VJ_OK;
}

int vj_affine_from_eyes(double lx, double ly, double rx, double ry, int out_w, int out_h, double ex_l, double ex_r, double ey, double m[6]) {
    if (!m) {
        set_error("vj_affine_from_eyes: null argument");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(lx) || !std::isfinite(ly) || !std::isfinite(rx) || !std::isfinite(ry) || !std::isfinite(ex_l) || !std::isfinite(ex_r) ||
        !std::isfinite(ey) || out_w <= 0 || out_h <= 0) {
        set_error("vj_affine_from_eyes: the eyes and their places must be finite, out_w and out_h positive");
        return VJ_ERR_ARG;
    }
    if (!(ex_r > ex_l)) {
        set_error("vj_affine_from_eyes: ex_r must be above ex_l");
        return VJ_ERR_ARG;
    }
    if (lx == rx && ly == ry) {
        set_error("vj_affine_from_eyes: the eyes coincide");
        return VJ_ERR_ARG;
    }
    const double d = (ex_r - ex_l) * out_w;
    const double a = (rx - lx) / d, b = (ry - ly) / d;
    const double cxl = ex_l * out_w, cy = ey * out_h;
    m[0] = a;
    m[1] = -b;
    m[2] = lx - a * cxl + b * cy;
    m[3] = b;
    m[4] = a;
    m[5] = ly - b * cxl - a * cy;
    return VJ_OK;
}

}  // extern "C"
