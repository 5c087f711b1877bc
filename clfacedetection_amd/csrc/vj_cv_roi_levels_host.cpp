// Host planner of CV_HAAR_SCALE_IMAGE inside regions that needs no device: see vj_cv_roi_levels_host.hpp.
#include "vj_cv_roi_levels_host.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace vj {

int cv_scale_image_levels(int win_w, int win_h, int W, int H, double scale_factor, int min_w, int min_h, int max_w, int max_h,
                          std::vector<CvLevelHost>* out, int* n_empty) {
    out->clear();
    if (n_empty) *n_empty = 0;
    double factor = 1;
    for (int k = 0;; ++k, factor *= scale_factor) {
        if (k > 65536) {
            set_error("scale_factor %.17g gives more than 65536 pyramid levels", scale_factor);
            return VJ_ERR_LIMIT;
        }
        CvLevelHost s;
        s.factor = factor;
        s.idx = k;
        s.win_w = cv_round(win_w * factor);
        s.win_h = cv_round(win_h * factor);
        s.lw = cv_round(W / factor);
        s.lh = cv_round(H / factor);
        if (s.lw - win_w + 1 <= 0 || s.lh - win_h + 1 <= 0) break;
        if (s.win_w > max_w || s.win_h > max_h) break;
        if (s.win_w < min_w || s.win_h < min_h) continue;
        // x, y = 0, ystep, ... < size - window (:1015-1020, :1079-1080)
        s.step = factor > 2 ? 1 : 2;
        s.end_x = (s.lw - win_w + s.step - 1) / s.step;
        s.end_y = (s.lh - win_h + s.step - 1) / s.step;
        if (s.end_x <= 0 || s.end_y <= 0) {   // (a level exactly one window wide or high: no position)
            if (n_empty) ++*n_empty;
            continue;
        }
        out->push_back(s);
    }
    return VJ_OK;
}

void build_taps(int src, int dst, bool rows, bool area, PyrTap* out) {
    const double scale = 1. / ((double)dst / src);
    for (int d = 0; d < dst; ++d) {
        PyrTap& t = out[d];
        if (area) {
            t.i0 = (uint16_t)std::min(2 * d, src - 1);
            t.i1 = (uint16_t)std::min(2 * d + 1, src - 1);
            t.c0 = t.c1 = 0;
            continue;
        }
        float f = (float)((d + 0.5) * scale - 0.5);
        int i = (int)std::floor(f);
        f -= (float)i;
        if (!rows) {
            if (i < 0) { i = 0; f = 0.f; }
            if (i >= src - 1) { i = src - 1; f = 0.f; }
        }
        t.i0 = (uint16_t)std::min(std::max(i, 0), src - 1);
        t.i1 = (uint16_t)std::min(std::max(i + 1, 0), src - 1);
        auto coef = [](float v) { return (int16_t)std::min(32767, std::max(-32768, cv_round((double)(v * 2048.f)))); };
        t.c0 = coef(1.f - f);
        t.c1 = coef(f);
    }
}

bool resize_is_area(int sw, int sh, int dw, int dh) {
    const double sx = 1. / ((double)dw / sw), sy = 1. / ((double)dh / sh);
    return std::fabs(sx - 2.) < 2.220446049250313e-16 && std::fabs(sy - 2.) < 2.220446049250313e-16;
}

uint32_t CvTapCache::get(int src, int dst, bool rows, bool area) {
    const auto key = std::make_tuple(src, dst, rows, area);
    const auto it = first.find(key);
    if (it != first.end()) return it->second;
    const uint32_t at = (uint32_t)taps.size();
    taps.resize(taps.size() + (size_t)dst);
    build_taps(src, dst, rows, area, taps.data() + at);
    first.emplace(key, at);
    return at;
}

namespace {

inline uint32_t align4(uint32_t v) { return (v + 3u) & ~3u; }

// Shelves of the canvas's width, tallest level image first: one goes to the first shelf with room beside what it holds (every shelf
// is at least as high as anything that comes after it), else it opens a new shelf below.  false: the canvas exceeds the budget.
bool pack_shelves(const std::vector<CvRegionLevel>& lv, size_t n, uint64_t budget_px, std::vector<uint32_t>* ox, std::vector<uint32_t>* oy,
                  uint32_t* cw, uint32_t* ch) {
    uint64_t area = 0;
    uint32_t widest = 4;
    for (size_t i = 0; i < n; ++i) {
        area += (uint64_t)align4((uint32_t)lv[i].lv.lw) * (uint64_t)lv[i].lv.lh;
        widest = std::max(widest, align4((uint32_t)lv[i].lv.lw));
    }
    if (area > budget_px) return false;
    const uint32_t W = std::max(widest, align4((uint32_t)std::ceil(std::sqrt((double)area))));
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lv[x].lv.lh > lv[y].lv.lh; });
    struct Shelf { uint32_t y, used; };
    std::vector<Shelf> shelves;
    size_t open = 0;   // shelves before this one are full to within the narrowest level image seen: not searched again
    uint64_t H = 0;
    ox->assign(n, 0u);
    oy->assign(n, 0u);
    for (size_t i : order) {
        const uint32_t aw = align4((uint32_t)lv[i].lv.lw);
        Shelf* fit = nullptr;
        for (size_t s = open; s < shelves.size(); ++s)
            if (shelves[s].used + aw <= W) { fit = &shelves[s]; break; }
        if (!fit) {
            shelves.push_back(Shelf{(uint32_t)H, 0u});
            H += (uint64_t)lv[i].lv.lh;
            if ((uint64_t)W * H > budget_px) return false;
            fit = &shelves.back();
        }
        (*ox)[i] = fit->used;
        (*oy)[i] = fit->y;
        fit->used += aw;
        while (open < shelves.size() && shelves[open].used + 4u > W) ++open;
    }
    H = std::max<uint64_t>(H, 1);
    if (H >= 65535ull || (uint64_t)(W + 1u) * (H + 3ull) >= (1ull << 30) || (uint64_t)W * H > budget_px) return false;
    *cw = W;
    *ch = (uint32_t)H;
    return true;
}

}  // namespace

int cv_roi_plan_canvas(const std::vector<CvRoiHost>& regs, size_t first, int win_w, int win_h, double scale_factor, int min_w, int min_h,
                       uint64_t budget_px, CvTapCache* taps, CvRegionCanvas* out) {
    *out = CvRegionCanvas{};
    if (first >= regs.size()) return VJ_OK;
    // ---- the level images of the regions from `first` on, while their pixels stay within the budget (the first one in any case)
    std::vector<CvRegionLevel> lv;
    std::vector<size_t> region_end;   // levels of regions [first, first + k] end at region_end[k]
    std::vector<uint32_t> empty_end;  // ... and their levels without a grid position number empty_end[k]
    std::vector<CvLevelHost> one;
    uint64_t area = 0;
    for (size_t r = first; r < regs.size(); ++r) {
        const CvRoiHost& g = regs[r];
        if (g.frame < 0 || g.x < 0 || g.y < 0 || g.w <= 0 || g.h <= 0 || g.w > 65535 || g.h > 65535) {
            set_error("region %zu is not an image rectangle", r);
            return VJ_ERR_ARG;
        }
        // (maxSize is the image, tempcv.cpp:1230-1234: the region as a sub-image)
        int n_empty = 0;
        const int rc = cv_scale_image_levels(win_w, win_h, g.w, g.h, scale_factor, min_w, min_h, g.w, g.h, &one, &n_empty);
        if (rc) return rc;
        uint64_t a = 0;
        for (const CvLevelHost& s : one) a += (uint64_t)align4((uint32_t)s.lw) * (uint64_t)s.lh;
        if (r > first && area + a > budget_px) break;
        area += a;
        for (const CvLevelHost& s : one) lv.push_back(CvRegionLevel{(int)r, s, 0u});
        region_end.push_back(lv.size());
        empty_end.push_back((empty_end.empty() ? 0u : empty_end.back()) + (uint32_t)n_empty);
    }
    // ---- pack; a canvas the shelves make larger than the budget takes fewer regions
    std::vector<uint32_t> ox, oy;
    size_t take = region_end.size();
    uint32_t cw = 0, ch = 0;
    while (take > 0 && !pack_shelves(lv, region_end[take - 1], budget_px, &ox, &oy, &cw, &ch)) take = take == 1 ? 0 : std::max<size_t>(1, take * 3 / 4);
    if (take == 0) {
        out->oversized = true;
        out->n_regions = 1;
        return VJ_OK;
    }
    lv.resize(region_end[take - 1]);
    out->n_regions = take;
    out->n_empty_levels = empty_end[take - 1];
    out->w = cw;
    out->h = ch;
    out->pitch = align4(cw);
    out->dev.resize(lv.size());
    uint64_t unit = 0, row = 0;
    for (size_t i = 0; i < lv.size(); ++i) {
        const CvRoiHost& g = regs[(size_t)lv[i].region];
        const CvLevelHost& s = lv[i].lv;
        const bool is_area = resize_is_area(g.w, g.h, s.lw, s.lh);
        PyrRegionLevelDev& d = out->dev[i];
        d = PyrRegionLevelDev{(uint32_t)g.frame, (uint32_t)g.x, (uint32_t)g.y, (uint32_t)g.w, (uint32_t)g.h, ox[i], oy[i], (uint32_t)s.lw, (uint32_t)s.lh,
                              taps->get(g.w, s.lw, false, is_area), taps->get(g.h, s.lh, true, is_area), (uint32_t)unit, is_area ? 1u : 0u, {0u, 0u, 0u}};
        unit += (uint64_t)((s.lw + PYR_REGION_TW - 1) / PYR_REGION_TW) * (uint64_t)((s.lh + PYR_REGION_TH - 1) / PYR_REGION_TH);
        lv[i].row_first = (uint32_t)row;
        row += (uint64_t)s.end_y;
        out->windows += (uint64_t)s.end_x * (uint64_t)s.end_y;
        // (the unit indices and the detection counter are 32-bit; a canvas of budget_px pixels holds fewer positions than pixels)
        if (unit > 0x7fffffffull || row > 0x7fffffffull || out->windows > 0xffffffffull || taps->taps.size() > 0xffffffffull) {
            set_error("the level images of the regions hold more work units than a 32-bit index holds");
            return VJ_ERR_LIMIT;
        }
    }
    out->n_pyr_units = (uint32_t)unit;
    out->n_rows = (uint32_t)row;
    out->levels = std::move(lv);
    return VJ_OK;
}

bool cv_rois_levels_pay(const vj_roi* rois, int n_rois) {
    std::vector<std::pair<int, int>> sizes((size_t)std::max(n_rois, 0));
    for (size_t i = 0; i < sizes.size(); ++i) sizes[i] = std::make_pair(rois[i].w, rois[i].h);
    std::sort(sizes.begin(), sizes.end());
    const size_t n_sizes = (size_t)(std::unique(sizes.begin(), sizes.end()) - sizes.begin());
    return sizes.size() <= n_sizes * (size_t)CV_ROI_LEVELS_MAX_REGIONS_PER_SIZE;
}

}  // namespace vj
