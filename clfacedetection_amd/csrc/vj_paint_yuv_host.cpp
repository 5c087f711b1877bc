// Host planner of vj_paint_yuv that needs no device: see vj_paint_yuv_host.hpp.
#include "vj_paint_yuv_host.hpp"
#include "vj_yuv_host.hpp"

#include <algorithm>
#include <cstring>

namespace vj {

namespace {
inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15; }

const char* const PLANE_NAMES[3] = {"y", "c0", "c1"};

// two planes of one kind (host, device) whose byte extents [first byte, last row's end) meet, planes of one frame included
int check_planes_disjoint(const vj_yuv_image* frames, int n_frames) {
    struct Ext { uintptr_t b, e; int i; uint32_t id; };
    for (int dev = 0; dev < 2; ++dev) {
        std::vector<Ext> ext;
        for (int i = 0; i < n_frames; ++i) {
            if ((frames[i].on_device != 0) != (dev != 0)) continue;
            for (uint32_t id = 0; id < 3u; ++id) {
                const PaintYuvPlane q = paint_yuv_plane(frames[i], id);
                if (!q.p) continue;
                const uintptr_t b = (uintptr_t)q.p;
                ext.push_back(Ext{b, b + (uint64_t)(q.h - 1) * q.stride + (uint64_t)q.w * q.comps, i, id});
            }
        }
        std::sort(ext.begin(), ext.end(), [](const Ext& a, const Ext& b) { return a.b != b.b ? a.b < b.b : a.i != b.i ? a.i < b.i : a.id < b.id; });
        // (sorted by start: if any earlier extent reaches past this start, the one with the greatest end does)
        for (size_t k = 1, far = 0; k < ext.size(); ++k) {
            if (ext[far].e > ext[k].b) {
                const Ext &x = ext[far], &y = ext[k];
                const bool swap = x.i > y.i || (x.i == y.i && x.id > y.id);
                const Ext &lo = swap ? y : x, &hi = swap ? x : y;
                set_error("frame %d: its %s plane overlaps frame %d's %s plane (vj_paint_yuv writes the planes: each must own its bytes)",
                          hi.i, PLANE_NAMES[hi.id], lo.i, PLANE_NAMES[lo.id]);
                return VJ_ERR_ARG;
            }
            if (ext[k].e > ext[far].e) far = k;
        }
    }
    return VJ_OK;
}

// the work of one record: paint_apply's units of its rows, the phase-1 units and the scratch bytes of its mode
struct RecWork { uint64_t units, pre, scratch; uint32_t lanes; };
RecWork rec_work(uint32_t mode, uint32_t kw, uint32_t kh, uint32_t comps, uint32_t size) {
    RecWork w{paint_apply_units(kw * comps, kh), 0, 0, 0};
    if (mode == PAINT_BLUR) w.pre = paint_colsum_units(kw * comps, kh);
    if (mode == PAINT_PIXELATE) {
        w.lanes = paint_cell_lanes(size, comps);
        w.pre = paint_cell_units(kw, kh, size, w.lanes);
    }
    // per component, each rounded up to 16: the pair plane's record holds both components in one range
    w.scratch = comps * align16(paint_scratch_bytes(mode, kw, kh, 1u, size));
    return w;
}

int too_many_units() {
    set_error("vj_paint_yuv: the regions hold more work units than a 32-bit index holds");
    return VJ_ERR_LIMIT;
}
}  // namespace

PaintYuvPlane paint_yuv_plane(const vj_yuv_image& f, uint32_t id) {
    const bool planar = f.layout == VJ_YUV_I420;
    if (id == PAINT_YUV_PLANE_Y) return PaintYuvPlane{f.y, (uint32_t)f.y_stride, 1u, f.width, f.height};
    if (id == PAINT_YUV_PLANE_C0) return PaintYuvPlane{f.c0, (uint32_t)f.c_stride, planar ? 1u : 2u, f.width / 2, f.height / 2};
    return PaintYuvPlane{planar ? f.c1 : nullptr, (uint32_t)f.c_stride, 1u, f.width / 2, f.height / 2};
}

int paint_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                     PaintYuvLayout* out) {
    *out = PaintYuvLayout{};
    if (!p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && !regions)) {
        set_error("vj_paint_yuv: null argument");
        return VJ_ERR_ARG;
    }
    // the frames by vj_yuv_to_bgr's rules (its planner, with its default parameters: the BGR side is not looked at)
    vj_yuv_params yp;
    vj_yuv_default(&yp);
    YuvLayout yl;
    int rc = yuv_decode_layout(frames, n_frames, &yp, &yl);
    if (rc) return rc;
    if ((rc = check_planes_disjoint(frames, n_frames))) return rc;
    // the regions and the parameters by vj_paint's rules, on the Y planes as gray frames
    std::vector<vj_image> ys((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i) ys[(size_t)i] = vj_image{frames[i].y, frames[i].width, frames[i].height, frames[i].y_stride, frames[i].on_device, 1};
    if ((rc = paint_layout(ys.data(), n_frames, regions, n_regions, p, &out->luma))) return rc;
    const PaintLayout& L = out->luma;
    const int32_t B = p->color[0], G = p->color[1], R = p->color[2], H = 1 << 19;
    out->yc = (uint8_t)((269484 * R + 528482 * G + 102760 * B + H + (16 << 20)) >> 20);
    out->uc = (uint8_t)((-155188 * R - 305135 * G + 460324 * B + H + (128 << 20)) >> 20);
    out->vc = (uint8_t)((460324 * R - 385875 * G - 74448 * B + H + (128 << 20)) >> 20);
    uint64_t units = 0, pre = 0;
    for (int r = 0; r < n_regions; ++r) {
        const vj_roi& k = L.clipped[(size_t)r];
        vj_roi c;
        c.frame = k.frame;
        c.x = c.y = c.w = c.h = 0;
        const int32_t s = L.sizes[(size_t)r], cs = paint_yuv_chroma_size(L.mode, s);
        if (k.w > 0 && k.h > 0) {
            c.x = k.x >> 1, c.y = k.y >> 1;
            c.w = ((k.x + k.w + 1) >> 1) - c.x, c.h = ((k.y + k.h + 1) >> 1) - c.y;
            for (uint32_t id = 0; id < 3u; ++id) {   // the records paint_yuv_plan_slice will make of the region
                const PaintYuvPlane q = paint_yuv_plane(frames[k.frame], id);
                if (!q.p) continue;
                const vj_roi& pr = id == PAINT_YUV_PLANE_Y ? k : c;
                const RecWork w = rec_work(L.mode, (uint32_t)pr.w, (uint32_t)pr.h, q.comps, (uint32_t)(id == PAINT_YUV_PLANE_Y ? s : cs));
                units += w.units, pre += w.pre;
                out->scratch_bytes += w.scratch;
            }
            if (units > 0x7fffffffull || pre > 0x7fffffffull) return too_many_units();
        }
        out->chroma.push_back(c);
        out->csizes.push_back(cs);
    }
    return VJ_OK;
}

int paint_yuv_plan_slice(const vj_yuv_image* frames, const PaintYuvLayout& lay, size_t first, size_t end, PaintYuvSlice* out) {
    *out = PaintYuvSlice{};
    const PaintLayout& L = lay.luma;
    if (first > end || end > L.touched.size()) {
        set_error("internal error: a slice beyond the call's frames");
        return VJ_ERR_ARG;
    }
    out->frames.assign(L.touched.begin() + (ptrdiff_t)first, L.touched.begin() + (ptrdiff_t)end);
    // the regions bucketed by frame, stable: (frame, region index) ascending
    std::vector<int> order;
    for (size_t r = 0; r < L.clipped.size(); ++r) {
        const vj_roi& k = L.clipped[r];
        if (k.w > 0 && k.h > 0 && std::binary_search(out->frames.begin(), out->frames.end(), k.frame)) order.push_back((int)r);
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return L.clipped[(size_t)a].frame < L.clipped[(size_t)b].frame; });
    uint64_t unit = 0, pre = 0, scratch = 0;
    out->recs.reserve(order.size() * 3u);
    for (int r : order) {
        const vj_roi &k = L.clipped[(size_t)r], &m = L.mapped[(size_t)r], &c = lay.chroma[(size_t)r];
        const vj_yuv_image& f = frames[k.frame];
        for (uint32_t id = 0; id < 3u; ++id) {
            const PaintYuvPlane q = paint_yuv_plane(f, id);
            if (!q.p) continue;
            PaintYuvRec d;
            memset(&d, 0, sizeof(d));
            d.plane = const_cast<uint8_t*>(q.p);
            d.stride = q.stride;
            d.comps = q.comps;
            d.pw = q.w, d.ph = q.h;
            d.X0 = m.x, d.Y0 = m.y, d.Wm = m.w, d.Hm = m.h;
            d.cx0 = k.x, d.cy0 = k.y, d.cx1 = k.x + k.w, d.cy1 = k.y + k.h;
            d.size = L.sizes[(size_t)r];
            const vj_roi& pr = id == PAINT_YUV_PLANE_Y ? k : c;
            d.kx0 = pr.x, d.ky0 = pr.y, d.kx1 = pr.x + pr.w, d.ky1 = pr.y + pr.h;
            d.sub = id == PAINT_YUV_PLANE_Y ? 0u : 1u;
            d.psize = L.mode == PAINT_BLUR || L.mode == PAINT_PIXELATE ? (d.sub ? lay.csizes[(size_t)r] : d.size) : 0;
            d.plane_id = id;
            if (id == PAINT_YUV_PLANE_Y) d.color = lay.yc;
            else if (q.comps == 2u) d.color = f.layout == VJ_YUV_NV12 ? (uint32_t)lay.uc | (uint32_t)lay.vc << 8 : (uint32_t)lay.vc | (uint32_t)lay.uc << 8;
            else d.color = id == PAINT_YUV_PLANE_C0 ? lay.uc : lay.vc;
            const RecWork w = rec_work(L.mode, (uint32_t)pr.w, (uint32_t)pr.h, q.comps, (uint32_t)d.psize);
            d.lanes = w.lanes;
            d.unit_first = (uint32_t)unit;
            d.pre_first = (uint32_t)pre;
            d.scratch_off = scratch;
            unit += w.units, pre += w.pre, scratch += w.scratch;
            if (unit > 0x7fffffffull || pre > 0x7fffffffull) return too_many_units();
            out->recs.push_back(d);
            out->region.push_back(r);
        }
    }
    // the overlap lists: for every record the later records of the same plane whose rectangle (K, or Kc: two regions whose K are
    // disjoint can share a chroma sample) meets its own
    for (size_t i = 0; i < out->recs.size(); ++i) {
        PaintYuvRec& a = out->recs[i];
        a.ovl_first = (uint32_t)out->overlaps.size();
        const int fa = L.clipped[(size_t)out->region[i]].frame;
        for (size_t j = i + 1; j < out->recs.size() && L.clipped[(size_t)out->region[j]].frame == fa; ++j) {
            const PaintYuvRec& b = out->recs[j];
            if (b.plane_id == a.plane_id && a.kx0 < b.kx1 && b.kx0 < a.kx1 && a.ky0 < b.ky1 && b.ky0 < a.ky1) out->overlaps.push_back((uint32_t)j);
        }
        if ((out->overlaps.size() >> 32) != 0u) {
            set_error("vj_paint_yuv: the regions' overlap lists hold more entries than a 32-bit index holds");
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

int vj_paint_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                        vj_roi* clipped, vj_roi* chroma, int32_t* sizes, int32_t* chroma_sizes, uint64_t* scratch_bytes) {
    if (!p || !scratch_bytes || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) ||
        (n_regions > 0 && (!regions || !clipped || !chroma || !sizes || !chroma_sizes))) {
        set_error("vj_paint_yuv_layout: null argument");
        return VJ_ERR_ARG;
    }
    *scratch_bytes = 0;
    PaintYuvLayout lay;
    const int rc = paint_yuv_layout(frames, n_frames, regions, n_regions, p, &lay);
    if (rc) return rc;
    for (int r = 0; r < n_regions; ++r) {
        clipped[r] = lay.luma.clipped[(size_t)r];
        chroma[r] = lay.chroma[(size_t)r];
        sizes[r] = lay.luma.sizes[(size_t)r];
        chroma_sizes[r] = lay.csizes[(size_t)r];
    }
    *scratch_bytes = lay.scratch_bytes;
    return VJ_OK;
}

}  // extern "C"
