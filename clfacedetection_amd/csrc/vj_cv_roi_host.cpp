// Host side of the OpenCV profile's region calls that needs no device: see vj_cv_roi_host.hpp.
#include "vj_cv_roi_host.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>

namespace vj {

namespace {
int channels_of(const vj_image& im) { return im.channels <= 1 ? 1 : im.channels; }
}  // namespace

CvRoiFactor cv_roi_factor(int win_w, int win_h, double factor) {
    return CvRoiFactor{std::max(2., factor), cv_round(win_w * factor), cv_round(win_h * factor), 0};
}

int cv_count_factors(int win_w, int win_h, int w, int h, double scale_factor, int cap) {
    int n = 0;
    // (w - 10 in double: the same comparison for every int, without the overflow near INT_MIN)
    for (double factor = 1; factor * win_w < (double)w - 10 && factor * win_h < (double)h - 10; factor *= scale_factor)
        if (++n > cap) break;
    return n;
}

bool cv_roi_inside(const vj_roi& r, const vj_image* frames, int n_frames) {
    return r.frame >= 0 && r.frame < n_frames && frames[r.frame].data && r.w > 0 && r.h > 0 && r.x >= 0 && r.y >= 0 &&
           r.x <= frames[r.frame].width - r.w && r.y <= frames[r.frame].height - r.h;
}

bool cv_frames_uniform(const vj_image* frames, int n_frames, int* W, int* H, int* CH) {
    if (n_frames <= 0) return false;
    *W = frames[0].width;
    *H = frames[0].height;
    *CH = channels_of(frames[0]);
    if (*W <= 0 || *H <= 0 || *W >= 65535 || *H >= 65535 || (uint64_t)(*W + 1) * (uint64_t)(*H + 3) >= (1ull << 30)) return false;
    if (*CH != 1 && *CH != 3 && *CH != 4) return false;
    for (int i = 0; i < n_frames; ++i)
        if (!frames[i].data || frames[i].width != *W || frames[i].height != *H || channels_of(frames[i]) != *CH || frames[i].stride < *W * *CH)
            return false;
    return true;
}

std::vector<int> cv_rois_by_frame(const vj_roi* rois, int n_rois) {
    std::vector<int> by_frame((size_t)std::max(n_rois, 0));
    for (size_t i = 0; i < by_frame.size(); ++i) by_frame[i] = (int)i;
    std::stable_sort(by_frame.begin(), by_frame.end(), [&](int x, int y) { return rois[x].frame < rois[y].frame; });
    return by_frame;
}

void cv_rois_of_subbatch(const vj_roi* rois, const std::vector<int>& by_frame, size_t* next, int f0, int nf, std::vector<CvRoiHost>* regs) {
    regs->clear();
    for (; *next < by_frame.size() && rois[by_frame[*next]].frame < f0 + nf; ++*next) {
        const vj_roi& r = rois[by_frame[*next]];
        regs->push_back(CvRoiHost{r.frame - f0, r.x, r.y, r.w, r.h, by_frame[*next]});
    }
}

int cv_roi_build_units(const std::vector<CvRoiHost>& regs, int win_w, int win_h, double scale_factor, const std::vector<CvRoiFactor>& factors,
                       uint32_t stride, uint32_t frame_elems, int min_w, int min_h, std::vector<CvRoiDev>* rois,
                       std::vector<CvRoiUnit>* units, uint64_t* windows) {
    rois->resize(regs.size());
    units->clear();
    *windows = 0;
    for (size_t i = 0; i < regs.size(); ++i) {
        const CvRoiHost& r = regs[i];
        if (r.frame < 0 || r.x < 0 || r.y < 0 || r.w <= 0 || r.h <= 0) {
            set_error("region %zu is not an image rectangle", i);
            return VJ_ERR_ARG;
        }
        (*rois)[i] = CvRoiDev{(uint32_t)r.frame, (uint32_t)r.x, (uint32_t)r.y, (uint32_t)r.w, (uint32_t)r.h, {0, 0, 0}};
        const int nk = cv_count_factors(win_w, win_h, r.w, r.h, scale_factor, (int)factors.size());
        if (nk > (int)factors.size()) {
            set_error("region %zu takes more factors than the tables hold", i);
            return VJ_ERR_LIMIT;
        }
        for (int k = 0; k < nk; ++k) {
            const CvRoiFactor& f = factors[(size_t)k];
            const int end_x = cv_round((r.w - f.win_w) / f.ystep), end_y = cv_round((r.h - f.win_h) / f.ystep);
            if (f.win_w < min_w || f.win_h < min_h) continue;
            if (end_x <= 0 || end_y <= 0) continue;
            // evaluated windows lie inside the region (border rule), the region inside the frame; a feature may overshoot its window
            // by one column / row (separate rounding): the frame allocation's zeroed slack rows, as for whole frames
            const uint64_t origin_max = (uint64_t)((int64_t)r.y + r.h - f.win_h) * stride + (uint64_t)((int64_t)r.x + r.w - f.win_w);
            if (origin_max + f.max_reach >= (uint64_t)frame_elems) {
                set_error("feature reach exceeds the frame allocation");
                return VJ_ERR_LIMIT;
            }
            *windows += (uint64_t)end_x * (uint64_t)end_y;
            // the detection counter and the unit index are 32-bit
            if (*windows > 0xffffffffull || units->size() + (uint64_t)end_y > 0x7fffffffull) {
                set_error("the regions hold more windows than a 32-bit detection count holds");
                return VJ_ERR_LIMIT;
            }
            for (uint32_t iy = 0; iy < (uint32_t)end_y; ++iy) units->push_back(CvRoiUnit{(uint32_t)i, (uint32_t)k, iy, (uint32_t)end_x});
        }
    }
    return VJ_OK;
}

int cv_roi_rects_of(const CvDet* raw, size_t n_raw, const std::vector<CvRoiFactor>& factors, const std::vector<CvRoiHost>& regs,
                    std::vector<vj_rect>* all) {
    for (size_t i = 0; i < n_raw; ++i) {
        const CvDet& d = raw[i];
        if (d.slot >= factors.size() || d.frame >= regs.size()) {
            set_error("the region pass returned a detection outside its regions");
            return VJ_ERR_HIP;
        }
        const CvRoiFactor& f = factors[d.slot];
        all->push_back(vj_rect{(int32_t)d.x, (int32_t)d.y, f.win_w, f.win_h, 0.0f, regs[d.frame].id, (int32_t)d.slot});
    }
    return VJ_OK;
}

int cv_result_epilogue(const std::vector<vj_rect>& all, const StageProgram* prog, vj_result* out) {
    out->count = (uint32_t)all.size();
    if (!all.empty()) {
        out->rects = (vj_rect*)malloc(all.size() * sizeof(vj_rect));
        if (!out->rects) return VJ_ERR_NOMEM;
        memcpy(out->rects, all.data(), all.size() * sizeof(vj_rect));
    }
    if (prog) {
        vj_counters& k = out->counters;
        uint64_t rect_evals = 0;
        for (size_t s = 0; s < prog->n_nodes.size() && s < (size_t)VJ_MAX_STAGES; ++s) {
            k.stump_evals += k.stage_entered[s] * prog->n_nodes[s];
            rect_evals += k.stage_entered[s] * prog->n_rects[s];
        }
        k.gather_bytes = 48ull * k.stage_entered[0] + 16ull * rect_evals;
    }
    return VJ_OK;
}

int finish_cv_roi_result(std::vector<vj_rect>& all, const StageProgram* prog, const vj_cv_params* p, vj_result* out) {
    std::sort(all.begin(), all.end(), cv_rect_before);
    const int rc = cv_result_epilogue(all, (p->flags & VJ_FLAG_COUNTERS) != 0 ? prog : nullptr, out);
    if (rc) return rc;
    // groupRectangles(rectList, max(minNeighbors, 1), GROUP_EPS), a region at a time
    if (p->min_neighbors != 0 && out->count) return vj_group_rectangles(out->rects, &out->count, (int)std::max<uint32_t>(p->min_neighbors, 1u), 0.2);
    return VJ_OK;
}

std::vector<CvRoiSizeGroup> cv_roi_size_groups(const vj_image* frames, const vj_roi* rois, int n_rois) {
    std::map<std::tuple<int, int, int>, size_t> slot;
    for (int i = 0; i < n_rois; ++i) slot.emplace(std::make_tuple(rois[i].w, rois[i].h, channels_of(frames[rois[i].frame])), 0);
    size_t n = 0;
    for (auto& kv : slot) kv.second = n++;   // groups in (w, h, channels) order
    std::vector<CvRoiSizeGroup> groups(n);
    for (int i = 0; i < n_rois; ++i) {
        const vj_roi& r = rois[i];
        const vj_image& f = frames[r.frame];
        CvRoiSizeGroup& g = groups[slot[std::make_tuple(r.w, r.h, channels_of(f))]];
        g.idx.push_back(i);
        g.views.push_back(vj_image{f.data + (size_t)r.y * (size_t)f.stride + (size_t)r.x * (size_t)channels_of(f), r.w, r.h, f.stride,
                                   f.on_device, f.channels});
    }
    return groups;
}

int cv_roi_take_part(const vj_result& part, const std::vector<int>& idx, std::vector<vj_rect>* all, vj_result* out) {
    for (uint32_t k = 0; k < part.count; ++k) {
        vj_rect rr = part.rects[k];
        if (rr.frame < 0 || (size_t)rr.frame >= idx.size()) {
            set_error("a sub-image result names frame %d of %zu", rr.frame, idx.size());
            return VJ_ERR_ARG;
        }
        rr.frame = idx[(size_t)rr.frame];   // index in the batch -> region index
        all->push_back(rr);
    }
    out->counters.windows += part.counters.windows;
    out->counters.stump_evals += part.counters.stump_evals;
    out->counters.gather_bytes += part.counters.gather_bytes;
    for (int s = 0; s < VJ_MAX_STAGES; ++s) out->counters.stage_entered[s] += part.counters.stage_entered[s];
    out->timing.integral_ms += part.timing.integral_ms;
    out->timing.cascade_ms += part.timing.cascade_ms;
    out->timing.total_ms += part.timing.total_ms;
    out->timing.n_cascade_launches += part.timing.n_cascade_launches;
    return VJ_OK;
}

int cv_roi_emit_parts(std::vector<vj_rect>& all, vj_result* out) {
    std::stable_sort(all.begin(), all.end(), [](const vj_rect& a, const vj_rect& b) { return a.frame < b.frame; });
    return cv_result_epilogue(all, nullptr, out);
}

int cv_chain_regions(const vj_rect* raw, size_t n_raw, uint32_t min_neighbors, int W, int H, int f0, int nf,
                     std::vector<CvRoiHost>* regs, std::vector<vj_rect>* regions) {
    std::vector<vj_rect> cand(raw, raw + n_raw);
    std::sort(cand.begin(), cand.end(), [](const vj_rect& a, const vj_rect& b) {
        return std::tie(a.frame, a.scale_idx, a.y, a.x) < std::tie(b.frame, b.scale_idx, b.y, b.x);
    });
    uint32_t n = (uint32_t)cand.size();
    if (min_neighbors != 0 && n != 0u) {
        const int rc = vj_group_rectangles(cand.data(), &n, (int)std::max<uint32_t>(min_neighbors, 1u), 0.2);
        if (rc) return rc;
    }
    regs->clear();
    for (uint32_t i = 0; i < n; ++i) {
        const vj_rect& r = cand[i];
        if (r.frame < f0 || r.frame >= f0 + nf || r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 || r.x > W - r.w || r.y > H - r.h) {
            set_error("region %zu lies outside its frame", regions->size());
            return VJ_ERR_ARG;
        }
        regs->push_back(CvRoiHost{r.frame - f0, r.x, r.y, r.w, r.h, (int)regions->size()});
        regions->push_back(r);
    }
    return VJ_OK;
}

bool cv_chain_regions_match(const std::vector<vj_rect>& regions, const vj_result& first) {
    if (regions.size() != first.count) return false;
    for (size_t i = 0; i < regions.size(); ++i) {
        const vj_rect& a = regions[i];
        const vj_rect& b = first.rects[i];
        if (a.x != b.x || a.y != b.y || a.w != b.w || a.h != b.h || a.frame != b.frame) return false;
    }
    return true;
}

CvChainRoute cv_chain_route(uint32_t flags_first, uint32_t flags_second) {
    const bool asked = (flags_first & VJ_FLAG_CV_CHAIN_DEVICE) != 0u;
    CvChainRoute r{flags_first & ~(uint32_t)VJ_FLAG_CV_CHAIN_DEVICE, flags_second & ~(uint32_t)VJ_FLAG_CV_CHAIN_DEVICE, 0};
    const bool fast = ((r.flags_first | r.flags_second) & ~(uint32_t)VJ_FLAG_COUNTERS) == 0u;
    r.handoff = !fast ? 3 : asked ? 1 : 2;
    return r;
}

std::vector<uint32_t> cv_chain_rank(const vj_rect* raw, size_t n) {
    std::vector<uint32_t> idx(n), rank(n);
    for (size_t i = 0; i < n; ++i) idx[i] = (uint32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t i, uint32_t j) {
        return std::tie(raw[i].frame, raw[i].scale_idx, raw[i].y, raw[i].x) < std::tie(raw[j].frame, raw[j].scale_idx, raw[j].y, raw[j].x);
    });
    for (size_t k = 0; k < n; ++k) rank[idx[k]] = (uint32_t)k;
    return rank;
}

int cv_chain_region_ids(const CvRoiDev* rois, size_t n_regions, const vj_rect* raw, size_t n_raw, int f0, size_t base, std::vector<int>* ids) {
    ids->clear();
    if (n_regions != n_raw) {
        set_error("the device made %zu regions of %zu candidates", n_regions, n_raw);
        return VJ_ERR_HIP;
    }
    const std::vector<uint32_t> rank = cv_chain_rank(raw, n_raw);
    std::vector<bool> seen(n_raw, false);
    ids->reserve(n_regions);
    for (size_t r = 0; r < n_regions; ++r) {
        const CvRoiDev& d = rois[r];
        const size_t src = d.pad[0];
        if (src >= n_raw || seen[src]) {
            set_error("region %zu names candidate %zu of %zu%s", r, src, n_raw, src < n_raw ? " a second time" : "");
            return VJ_ERR_HIP;
        }
        seen[src] = true;
        const vj_rect& q = raw[src];
        if ((int64_t)d.frame + f0 != q.frame || (int64_t)d.x != q.x || (int64_t)d.y != q.y || (int64_t)d.w != q.w || (int64_t)d.h != q.h) {
            set_error("region %zu is not candidate %zu's rectangle", r, src);
            return VJ_ERR_HIP;
        }
        ids->push_back((int)(base + rank[src]));
    }
    return VJ_OK;
}

int cv_chain_grouped_regions(const CvRoiDev* rois, size_t n_regions, int f0, int nf, std::vector<vj_rect>* regions, std::vector<int>* ids) {
    ids->clear();
    ids->reserve(n_regions);
    uint32_t last = 0;
    for (size_t r = 0; r < n_regions; ++r) {
        const CvRoiDev& d = rois[r];
        if (d.frame >= (uint32_t)std::max(nf, 0) || d.frame < last) {
            set_error("grouped region %zu names frame %u of %d out of order", r, d.frame, nf);
            return VJ_ERR_HIP;
        }
        last = d.frame;
        ids->push_back((int)regions->size());
        regions->push_back(vj_rect{(int32_t)d.x, (int32_t)d.y, (int32_t)d.w, (int32_t)d.h, (float)(int)d.pad[0], f0 + (int32_t)d.frame, -1});
    }
    return VJ_OK;
}

int cv_chain_rects_of(const CvDet* raw, size_t n_raw, const std::vector<CvRoiFactor>& factors, const std::vector<int>& ids, std::vector<vj_rect>* all) {
    for (size_t i = 0; i < n_raw; ++i) {
        const CvDet& d = raw[i];
        if (d.slot >= factors.size() || d.frame >= ids.size()) {
            set_error("the region pass returned a detection outside its regions");
            return VJ_ERR_HIP;
        }
        const CvRoiFactor& f = factors[d.slot];
        all->push_back(vj_rect{(int32_t)d.x, (int32_t)d.y, f.win_w, f.win_h, 0.0f, ids[d.frame], (int32_t)d.slot});
    }
    return VJ_OK;
}

void cv_chain_info_add(vj_cv_chain_info* info, bool on_device, uint64_t regions, uint64_t units, uint64_t windows) {
    info->sub_batches += 1;
    if (on_device) info->sub_batches_device += 1;
    info->regions += regions;
    info->units += units;
    info->windows += windows;
}

int cv_chain_state_error(const CvChainState& s) {
    if (s.err_outside != 0u) {
        set_error("%u regions lie outside their frames", s.err_outside);
        return VJ_ERR_ARG;
    }
    if (s.err_factors != 0u) {
        set_error("%u regions take more factors than the tables hold", s.err_factors);
        return VJ_ERR_LIMIT;
    }
    if (s.err_reach != 0u) {
        set_error("feature reach exceeds the frame allocation");
        return VJ_ERR_LIMIT;
    }
    if (s.windows > 0xffffffffull || s.n_units > 0x7fffffffull) {
        set_error("the regions hold more windows than a 32-bit detection count holds");
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}

}  // namespace vj
