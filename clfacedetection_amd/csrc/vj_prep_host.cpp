// Host planner of vj_preprocess that needs no device: see vj_prep_host.hpp.
#include "vj_prep_host.hpp"
#include "vj_atlas_host.hpp"
#include "vj_cv_roi_levels_host.hpp"

#include <cmath>
#include <cstring>

namespace vj {

namespace {
inline uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }

// cvRound(len * f), at least 1; above 65535 as 65536 (refused by the caller)
uint32_t scaled_len(int len, double f) {
    const double v = (double)len * f;
    if (!(v < 65536.0)) return 65536u;
    return (uint32_t)std::max(cv_round(v), 1);
}
}  // namespace

int prep_layout(const vj_image* frames, int n_frames, const vj_prep* p, PrepLayout* out) {
    *out = PrepLayout{};
    if (!p) {
        set_error("vj_preprocess: null parameters");
        return VJ_ERR_ARG;
    }
    std::vector<AtlasSize> sizes;
    const int rc = atlas_check_frames(frames, n_frames, &sizes);
    if (rc) return rc;
    if ((p->flags & ~(uint32_t)VJ_PREP_EQUALIZE) != 0u || p->reserved != 0u) {
        set_error("vj_prep: %s", p->reserved != 0u ? "reserved must be 0" : "unknown bits in flags");
        return VJ_ERR_ARG;
    }
    if (p->dst_w < 0 || p->dst_h < 0 || (p->dst_w > 0) != (p->dst_h > 0)) {
        set_error("vj_prep: dst_w and dst_h must both be positive, or both 0");
        return VJ_ERR_ARG;
    }
    if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || p->fx < 0 || p->fy < 0 || (p->fx > 0) != (p->fy > 0)) {
        set_error("vj_prep: fx and fy must both be positive and finite, or both 0");
        return VJ_ERR_ARG;
    }
    const bool fixed = p->dst_w > 0, scaled = !fixed && p->fx > 0;
    out->equalize = (p->flags & VJ_PREP_EQUALIZE) != 0u;
    out->slots.reserve((size_t)n_frames);
    uint64_t off = 0, units = 0;
    for (int i = 0; i < n_frames; ++i) {
        const AtlasSize& s = sizes[(size_t)i];
        PrepSlot t;
        t.sw = (uint32_t)s.w;
        t.sh = (uint32_t)s.h;
        t.ch = (uint32_t)s.ch;
        t.dw = fixed ? (uint32_t)p->dst_w : scaled ? scaled_len(s.w, p->fx) : t.sw;
        t.dh = fixed ? (uint32_t)p->dst_h : scaled ? scaled_len(s.h, p->fy) : t.sh;
        if (t.sw > 65535u || t.sh > 65535u || t.dw > 65535u || t.dh > 65535u) {
            set_error("frame %d: %u x %u -> %s%u x %u: sides up to 65535 (the taps' 16-bit indices)", i, t.sw, t.sh,
                      t.dw > 65535u || t.dh > 65535u ? "more than " : "", std::min(t.dw, 65535u), std::min(t.dh, 65535u));
            return VJ_ERR_LIMIT;
        }
        t.pitch = align4(t.dw);
        t.off = (off + 255u) & ~(uint64_t)255;
        off = t.off + (uint64_t)t.pitch * t.dh;
        units += prep_units(t.dw, t.dh);
        out->slots.push_back(t);
    }
    if (units > 0x7fffffffull) {
        set_error("vj_preprocess: the frames hold more work units than a 32-bit index holds");
        return VJ_ERR_LIMIT;
    }
    out->bytes = off;
    return VJ_OK;
}

int prep_check_overlap(const vj_image* frames, int n_frames, const uint8_t* dst, uint64_t bytes) {
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + bytes;
    for (int i = 0; i < n_frames; ++i) {
        const vj_image& f = frames[i];
        if (!f.on_device) continue;
        const int ch = f.channels <= 1 ? 1 : f.channels;
        const uintptr_t s0 = (uintptr_t)f.data, s1 = s0 + (uint64_t)(f.height - 1) * (uint64_t)f.stride + (uint64_t)f.width * (uint64_t)ch;
        if (s0 < d1 && d0 < s1) {
            set_error("frame %d: a device-resident source overlaps the destination buffer", i);
            return VJ_ERR_ARG;
        }
    }
    return VJ_OK;
}

int prep_plan_slice(const vj_image* frames, const PrepLayout& lay, size_t first, size_t n, PrepSlice* out) {
    out->recs.clear();
    out->eq.clear();
    out->taps.clear();
    out->n_units = 0;
    if (first + n > lay.slots.size()) {
        set_error("internal error: a slice beyond the call's frames");
        return VJ_ERR_ARG;
    }
    std::map<std::tuple<uint32_t, uint32_t, bool, bool>, uint32_t> runs;
    auto run_of = [&](uint32_t src, uint32_t dst, bool rows, bool area) {
        const auto key = std::make_tuple(src, dst, rows, area);
        const auto it = runs.find(key);
        if (it != runs.end()) return it->second;
        const uint32_t at = (uint32_t)out->taps.size();
        out->taps.resize((size_t)at + align4(dst));
        build_taps((int)src, (int)dst, rows, area, out->taps.data() + at);
        for (uint32_t k = dst; k < align4(dst); ++k) out->taps[(size_t)at + k] = out->taps[(size_t)at + dst - 1u];
        runs.emplace(key, at);
        return at;
    };
    uint64_t unit = 0;
    for (size_t i = 0; i < n; ++i) {
        const PrepSlot& t = lay.slots[first + i];
        const vj_image& f = frames[first + i];
        PrepFrameDev d;
        memset(&d, 0, sizeof(d));
        d.src = f.data;
        d.dst_off = t.off;
        d.stride = (uint32_t)f.stride;
        d.channels = t.ch;
        d.sw = t.sw;
        d.sh = t.sh;
        d.dw = t.dw;
        d.dh = t.dh;
        d.pitch = t.pitch;
        if (t.dw == t.sw && t.dh == t.sh) {   // vj_resize_linear to the source's own size is the identity
            d.mode = PREP_COPY;
        } else {
            const bool area = resize_is_area((int)t.sw, (int)t.sh, (int)t.dw, (int)t.dh) && t.sw == 2u * t.dw && t.sh == 2u * t.dh;
            d.mode = area ? PREP_AREA : PREP_BILINEAR;
            d.xtab = run_of(t.sw, t.dw, false, area);
            d.ytab = run_of(t.sh, t.dh, true, area);
        }
        d.unit_first = (uint32_t)unit;
        d.hist_slot = (uint32_t)i;
        unit += prep_units(t.dw, t.dh);
        if (unit > 0x7fffffffull || (out->taps.size() >> 32) != 0u) {
            set_error("vj_preprocess: the frames hold more work units than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
        out->recs.push_back(d);
        out->eq.push_back(AtlasFrameDev{nullptr, t.pitch, 1u, t.dw, t.dh, 0u, 0u, d.unit_first, 0u});
    }
    out->n_units = (uint32_t)unit;
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

void vj_prep_default(vj_prep* p) {
    if (p) memset(p, 0, sizeof(*p));
}

int vj_preprocess_layout(const vj_image* frames, int n_frames, const vj_prep* p, vj_image* out, uint64_t* bytes) {
    if (!p || !bytes || n_frames < 0 || (n_frames > 0 && (!frames || !out))) {
        set_error("vj_preprocess_layout: null argument");
        return VJ_ERR_ARG;
    }
    *bytes = 0;
    PrepLayout lay;
    const int rc = prep_layout(frames, n_frames, p, &lay);
    if (rc) return rc;
    for (int i = 0; i < n_frames; ++i) {
        const PrepSlot& t = lay.slots[(size_t)i];
        out[i] = vj_image{(const uint8_t*)(uintptr_t)t.off, (int32_t)t.dw, (int32_t)t.dh, (int32_t)t.pitch, 1, 1};
    }
    *bytes = lay.bytes;
    return VJ_OK;
}

}  // extern "C"
