// Host planner of vj_extract_yuv / vj_extract_affine_yuv that needs no device: see vj_extract_yuv_host.hpp.
#include "vj_extract_yuv_host.hpp"

#include <cstring>

namespace vj {

namespace {

// the frames by vj_yuv_to_bgr's rules and `yp`; the Y planes as the gray frames vj_extract's and vj_extract_affine's planners check
int yuv_source(const char* who, const vj_yuv_image* frames, int n_frames, const vj_yuv_params* yp, YuvSource* out) {
    *out = YuvSource{};
    YuvLayout yl;
    const int rc = yuv_decode_layout(frames, n_frames, yp, &yl);
    if (rc) {
        if (n_frames < 0 || (n_frames > 0 && !frames)) set_error("%s: null argument", who);
        return rc;
    }
    out->channels = yl.channels;
    out->swap_rb = yl.swap_rb;
    out->luma.resize((size_t)n_frames);
    for (int i = 0; i < n_frames; ++i)
        out->luma[(size_t)i] = vj_image{frames[i].y, frames[i].width, frames[i].height, frames[i].y_stride, frames[i].on_device, 1};
    return VJ_OK;
}

// The planners laid the output out for one channel (the Y planes are gray): the counts of C channels, and the unit limit again
template <typename Layout>
int set_channels(const char* who, Layout* lay, uint32_t C, uint64_t n, uint64_t* pitch) {
    lay->C = lay->gray ? 1u : C;
    lay->rows = lay->planar ? lay->C * lay->out_h : lay->out_h;
    lay->row_bytes = lay->planar ? lay->out_w : lay->out_w * lay->C;
    lay->region_bytes = (uint64_t)lay->rows * lay->row_bytes;
    if (pitch) *pitch = lay->region_bytes;
    lay->bytes = lay->region_bytes * n;
    if (extract_units(lay->row_bytes, lay->rows) * n > 0x7fffffffull) {
        set_error("%s: the regions hold more work units than a 32-bit index holds", who);
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}

YuvPlanesDev planes_of(const vj_yuv_image& f, uint32_t unit_first) {
    YuvPlanesDev d;
    memset(&d, 0, sizeof(d));
    d.y = f.y;
    d.c0 = f.c0;
    d.c1 = f.layout == VJ_YUV_I420 ? f.c1 : nullptr;
    d.y_stride = (uint32_t)f.y_stride;
    d.c_stride = (uint32_t)f.c_stride;
    d.fw = f.width;
    d.fh = f.height;
    d.layout = (uint32_t)f.layout;
    d.unit_first = unit_first;
    return d;
}

}  // namespace

int extract_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                       const vj_yuv_params* yp, ExtractYuvLayout* out) {
    *out = ExtractYuvLayout{};
    if (!p || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && !regions)) {
        set_error("vj_extract_yuv: null argument");
        return VJ_ERR_ARG;
    }
    int rc;
    if ((rc = yuv_source("vj_extract_yuv", frames, n_frames, yp, &out->src))) return rc;
    if ((rc = extract_layout(out->src.luma.data(), n_frames, regions, n_regions, p, &out->lay))) return rc;
    return set_channels("vj_extract_yuv", &out->lay, out->src.channels, (uint64_t)n_regions, &out->lay.region_pitch);
}

int affine_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                      const vj_yuv_params* yp, AffineYuvLayout* out) {
    *out = AffineYuvLayout{};
    if (!p || n_frames < 0 || n < 0 || (n_frames > 0 && !frames) || (n > 0 && !affines)) {
        set_error("vj_extract_affine_yuv: null argument");
        return VJ_ERR_ARG;
    }
    int rc;
    if ((rc = yuv_source("vj_extract_affine_yuv", frames, n_frames, yp, &out->src))) return rc;
    if ((rc = affine_layout(out->src.luma.data(), n_frames, affines, n, p, &out->lay))) return rc;
    return set_channels("vj_extract_affine_yuv", &out->lay, out->src.channels, (uint64_t)n, nullptr);
}

int extract_yuv_plan_slice(const vj_yuv_image* frames, const vj_roi* regions, const ExtractYuvLayout& lay, size_t first, size_t n, ExtractYuvSlice* out) {
    out->recs.clear();
    const int rc = extract_plan_slice(lay.src.luma.data(), regions, lay.lay, first, n, &out->luma);
    if (rc) return rc;
    out->recs.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const ExtractRegionDev& g = out->luma.recs[i];
        ExtractYuvRegionDev d;
        memset(&d, 0, sizeof(d));
        d.f = planes_of(frames[regions[first + i].frame], g.unit_first);
        d.dst_off = g.dst_off;
        d.x0 = g.x0, d.y0 = g.y0, d.cw = g.cw, d.ch = g.ch;
        d.xtab = g.xtab, d.ytab = g.ytab;
        d.mode = g.mode;
        out->recs.push_back(d);
    }
    return VJ_OK;
}

int affine_yuv_plan_slice(const vj_yuv_image* frames, const vj_affine* affines, const AffineYuvLayout& lay, size_t first, size_t n, AffineYuvSlice* out) {
    out->recs.clear();
    const int rc = affine_plan_slice(lay.src.luma.data(), affines, lay.lay, first, n, &out->luma);
    if (rc) return rc;
    out->recs.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const AffineRegionDev& g = out->luma.recs[i];
        AffineYuvRegionDev d;
        memset(&d, 0, sizeof(d));
        d.f = planes_of(frames[affines[first + i].frame], g.unit_first);
        d.dst_off = g.dst_off;
        for (int k = 0; k < 6; ++k) d.m[k] = g.m[k];
        out->recs.push_back(d);
    }
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

extern "C" {

int vj_extract_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                          const vj_yuv_params* yp, vj_roi* src_regions, int* channels, uint64_t* bytes) {
    if (channels) *channels = 0;
    if (bytes) *bytes = 0;
    if (!p || !channels || !bytes || n_frames < 0 || n_regions < 0 || (n_frames > 0 && !frames) || (n_regions > 0 && (!regions || !src_regions))) {
        set_error("vj_extract_yuv_layout: null argument");
        return VJ_ERR_ARG;
    }
    ExtractYuvLayout lay;
    const int rc = extract_yuv_layout(frames, n_frames, regions, n_regions, p, yp, &lay);
    if (rc) return rc;
    for (int r = 0; r < n_regions; ++r) src_regions[r] = lay.lay.src[(size_t)r];
    *channels = (int)lay.lay.C;
    *bytes = lay.lay.bytes;
    return VJ_OK;
}

int vj_extract_affine_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                                 const vj_yuv_params* yp, int* channels, uint64_t* bytes) {
    if (channels) *channels = 0;
    if (bytes) *bytes = 0;
    if (!p || !channels || !bytes || n_frames < 0 || n < 0 || (n_frames > 0 && !frames) || (n > 0 && !affines)) {
        set_error("vj_extract_affine_yuv_layout: null argument");
        return VJ_ERR_ARG;
    }
    AffineYuvLayout lay;
    const int rc = affine_yuv_layout(frames, n_frames, affines, n, p, yp, &lay);
    if (rc) return rc;
    *channels = (int)lay.lay.C;
    *bytes = lay.lay.bytes;
    return VJ_OK;
}

}  // extern "C"
