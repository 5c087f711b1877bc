// Host side of vj_detect_opencv_rois / vj_detect_opencv_chain that needs no device: argument checks, the factors a
// region takes, the unit list of the region pass, the fallback's grouping by region size and its index remap, the chain's regions,
// and the shaping of a result.  Compiled without HIP too: tests/cv_roi_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_internal.hpp"
#include "vj_cv_roi_units.hpp"

#include <cmath>
#include <tuple>

namespace vj {

inline int cv_round(double v) { return (int)std::lrint(v); }   // cvRound: round half to even

// A region as the pass sees it: a rectangle of frame `frame` of the sub-batch on the device; `id`: what rect.frame reports.
struct CvRoiHost { int frame, x, y, w, h, id; };

// What a factor of the enumeration gives whatever the region (the doubles of the loop, factor *= scale_factor)
struct CvRoiFactor {
    double ystep;          // max(2, factor)
    int win_w, win_h;      // cvRound(orig * factor)
    uint64_t max_reach;    // furthest element a feature touches, from the window origin (set by the table builder)
};
CvRoiFactor cv_roi_factor(int win_w, int win_h, double factor);

// The factors cvHaarDetectObjects enumerates for a w x h image (tempcv.cpp:1344-1349); cap + 1 when there are more than `cap`.
int cv_count_factors(int win_w, int win_h, int w, int h, double scale_factor, int cap);

bool cv_roi_inside(const vj_roi& r, const vj_image* frames, int n_frames);
// Frames a batch of the profile accepts: one size and channel count, within the 32-bit offsets of a frame's sum image
bool cv_frames_uniform(const vj_image* frames, int n_frames, int* W, int* H, int* CH);

// Region indices ordered by frame (stable), and the regions of the next sub-batch [f0, f0 + nf) taken from that order
std::vector<int> cv_rois_by_frame(const vj_roi* rois, int n_rois);
void cv_rois_of_subbatch(const vj_roi* rois, const std::vector<int>& by_frame, size_t* next, int f0, int nf, std::vector<CvRoiHost>* regs);

// The scale loop of every region (tempcv.cpp:1344-1377 with the region's size): one unit per window row, ordered by (region, factor,
// row); `factors` holds at least the factors of the largest region.  *windows: the grid positions of all units.
int cv_roi_build_units(const std::vector<CvRoiHost>& regs, int win_w, int win_h, double scale_factor, const std::vector<CvRoiFactor>& factors,
                       uint32_t stride, uint32_t frame_elems, int min_w, int min_h, std::vector<CvRoiDev>* rois,
                       std::vector<CvRoiUnit>* units, uint64_t* windows);

// The pass's detections as rectangles: rect.frame = the region's id, x / y relative to the region
int cv_roi_rects_of(const CvDet* raw, size_t n_raw, const std::vector<CvRoiFactor>& factors, const std::vector<CvRoiHost>& regs,
                    std::vector<vj_rect>* all);

// The order of a result of the profile: (frame, scale_idx, y, x)
inline bool cv_rect_before(const vj_rect& a, const vj_rect& b) {
    return std::tie(a.frame, a.scale_idx, a.y, a.x) < std::tie(b.frame, b.scale_idx, b.y, b.x);
}

// The end of every call of the profile: `all` into out->rects / out->count, and the counters' derived fields (stump_evals,
// gather_bytes) from the per-stage counts already in out->counters (prog null: an uncounted call, or no pass ran).
int cv_result_epilogue(const std::vector<vj_rect>& all, const StageProgram* prog, vj_result* out);

// `all` into *out as vj_detect_opencv shapes a result: sorted by (region, scale_idx, y, x), grouped per region when min_neighbors != 0;
// the counters' derived fields from the stage program (null: no pass ran).
int finish_cv_roi_result(std::vector<vj_rect>& all, const StageProgram* prog, const vj_cv_params* p, vj_result* out);

// The fallback: regions by (w, h, channels), each group's sub-image views in region order
struct CvRoiSizeGroup {
    std::vector<int> idx;           // region indices
    std::vector<vj_image> views;    // {data + y * stride + x * channels, w, h, stride, on_device, channels}
};
std::vector<CvRoiSizeGroup> cv_roi_size_groups(const vj_image* frames, const vj_roi* rois, int n_rois);
// one group's result into the whole: rect.frame from index in the group to region index; counters and times add up
int cv_roi_take_part(const vj_result& part, const std::vector<int>& idx, std::vector<vj_rect>* all, vj_result* out);
// the parts are in their final order: only the regions are put in order
int cv_roi_emit_parts(std::vector<vj_rect>& all, vj_result* out);

// The chain: a sub-batch's raw candidates of the first cascade — sorted, grouped per frame when min_neighbors != 0 — as the regions
// of the second (appended to *regions; regs: the same, relative to the sub-batch, ids continuing)
int cv_chain_regions(const vj_rect* raw, size_t n_raw, uint32_t min_neighbors, int W, int H, int f0, int nf,
                     std::vector<CvRoiHost>* regs, std::vector<vj_rect>* regions);
bool cv_chain_regions_match(const std::vector<vj_rect>& regions, const vj_result& first);

// ---- the chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE; vj_cv_chain.hip): what the host does around it
// Which way a vj_detect_opencv_chain call goes (vj_cv_chain_info::handoff: 1 device, 2 host, 3 the two public calls), and the two
// flag words with VJ_FLAG_CV_CHAIN_DEVICE taken out: nothing keyed on flags ever sees the bit.  Only flags_first is read for it.
struct CvChainRoute { uint32_t flags_first, flags_second; int handoff; };
CvChainRoute cv_chain_route(uint32_t flags_first, uint32_t flags_second);

// rank[i]: the place of raw[i] among raw[0..n) in the order of the result, (frame, scale_idx, y, x); equal keys keep their order
std::vector<uint32_t> cv_chain_rank(const vj_rect* raw, size_t n);

// Raw candidates as regions: device region r comes from record rois[r].pad[0] of the sub-batch's `raw` (rect.frame counts from the
// call's first frame, the sub-batch's from f0) and is out_first's rectangle base + rank of that record.  Refused (VJ_ERR_HIP): a
// source index out of range or used twice, a count that is not the records', a region that is not its record's rectangle.
int cv_chain_region_ids(const CvRoiDev* rois, size_t n_regions, const vj_rect* raw, size_t n_raw, int f0, size_t base, std::vector<int>* ids);

// Grouped regions, as read back: appended to *regions as vj_group_rectangles writes them (weight = members, scale_idx -1, frames
// counted from the call's first), ids continuing.  Refused (VJ_ERR_HIP): frames out of [0, nf) or not in order.
int cv_chain_grouped_regions(const CvRoiDev* rois, size_t n_regions, int f0, int nf, std::vector<vj_rect>* regions, std::vector<int>* ids);

// The second cascade's detections as rectangles: rect.frame = ids[the device's region index]
int cv_chain_rects_of(const CvDet* raw, size_t n_raw, const std::vector<CvRoiFactor>& factors, const std::vector<int>& ids, std::vector<vj_rect>* all);

// One sub-batch into the call's record; what the device's state block makes the call return (VJ_OK: nothing refused)
void cv_chain_info_add(vj_cv_chain_info* info, bool on_device, uint64_t regions, uint64_t units, uint64_t windows);
int cv_chain_state_error(const CvChainState& s);

}  // namespace vj
