// Records the region pass of the OpenCV profile (vj_cv_roi.hip) shares with the host code that builds and reads
// them (vj_cv_roi_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs, nothing else.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VJ_HD __host__ __device__
#else
#define VJ_HD
#endif

namespace vj {

struct CvDet {
    uint32_t x, y, slot, frame;
};

// A region is the sub-image an OpenCV caller would hand over: factors, grid ends and the border rule come from its w x h.
struct CvRoiDev {
    uint32_t frame;          // in the sub-batch whose integral images are on the device
    uint32_t x, y, w, h;     // inside the frame
    uint32_t pad[3];         // the chain's device hand-off (vj_cv_chain.hip): pad[0] = index of the first cascade's record the region
                             // comes from (raw candidates) or the members of its class (grouped)
};
static_assert(sizeof(CvRoiDev) == 32, "CvRoiDev is 32 bytes");
// One unit of work: window row `iy` of (region, factor slot), end_x positions long.
struct CvRoiUnit { uint32_t roi, slot, iy, end_x; };

// ---- vj_detect_opencv_chain with VJ_FLAG_CV_CHAIN_DEVICE: the regions and units are built on the device (vj_cv_chain.hip)
// What a factor slot of the region plan gives the device's unit builder: the doubles of the host's enumeration (factor *= scale_factor)
struct CvChainFactor {
    double factor, ystep;    // ystep = max(2, factor)
    int32_t win_w, win_h;    // cvRound(orig * factor)
    uint64_t max_reach;      // as CvRoiFactor::max_reach
};
static_assert(sizeof(CvChainFactor) == 32, "CvChainFactor is 32 bytes");

// The leading factors a w x h region takes (cv_count_factors on the table: factor * orig < size - 10 in f64), at most n
VJ_HD inline uint32_t cv_chain_count_factors(const CvChainFactor* f, uint32_t n, int orig_w, int orig_h, int w, int h) {
    uint32_t k = 0;
    while (k < n && f[k].factor * orig_w < (double)w - 10 && f[k].factor * orig_h < (double)h - 10) ++k;
    return k;
}
// endX / endY of a factor's grid in a region `size` long (tempcv.cpp:1371-1372): cvRound((size - win) / ystep), an IEEE f64 divide
// and a round to nearest even
VJ_HD inline int cv_chain_grid_end(int size, int win, double ystep) { return (int)__builtin_rint((size - win) / ystep); }
// Why cv_roi_build_units skips a (region, factor) or refuses the call
enum { CV_CHAIN_SLOT_OK = 0, CV_CHAIN_SLOT_SKIP = 1, CV_CHAIN_SLOT_REACH = 2 };
// One (region, factor) of cv_roi_build_units: the grid ends, and whether the slot is skipped (below the minimum size, or an empty
// grid) or reaches beyond the frame allocation
VJ_HD inline int cv_chain_slot(const CvChainFactor& f, int rx, int ry, int rw, int rh, int min_w, int min_h, uint32_t stride, uint32_t frame_elems,
                               int* end_x, int* end_y) {
    *end_x = cv_chain_grid_end(rw, f.win_w, f.ystep);
    *end_y = cv_chain_grid_end(rh, f.win_h, f.ystep);
    if (f.win_w < min_w || f.win_h < min_h) return CV_CHAIN_SLOT_SKIP;
    if (*end_x <= 0 || *end_y <= 0) return CV_CHAIN_SLOT_SKIP;
    const uint64_t origin_max = (uint64_t)((int64_t)ry + rh - f.win_h) * stride + (uint64_t)((int64_t)rx + rw - f.win_w);
    return origin_max + f.max_reach >= (uint64_t)frame_elems ? CV_CHAIN_SLOT_REACH : CV_CHAIN_SLOT_OK;
}

// What the hand-off kernels leave for the host to read after the sub-batch's one synchronisation
struct CvChainState {
    uint32_t n_regions;      // regions handed to the second cascade
    uint32_t n_units_run;    // the units the region pass walks: n_units when everything fitted and nothing was refused, else 0
    uint64_t n_units;        // the count pass's total, exact also when the unit buffer is too short for it
    uint64_t windows;        // grid positions of all units
    uint32_t overflow;       // frames with more candidates than the device groups (group_max)
    uint32_t err_outside;    // regions not inside their frame
    uint32_t err_factors;    // regions that take more factors than the tables hold
    uint32_t err_reach;      // (region, factor) pairs whose features reach beyond the frame allocation
};
static_assert(sizeof(CvChainState) == 40, "CvChainState is 40 bytes");

// ---- CV_HAAR_SCALE_IMAGE inside regions (vj_detect_opencv_rois, route 2): the level images of a canvas (vj_cv_roi_levels_host.cpp
// plans them, pyramid_regions in vj_pyramid.hip writes them)
struct alignas(8) PyrTap {  // one destination column or row of a level
    uint16_t i0, i1;       // the two source columns / rows (clamped to the source)
    int16_t  c0, c1;       // their 11-bit weights (2048 = 1.0); area levels do not read them
};
// One level image: cvResize of the crop [cx, cx + cw) x [cy, cy + ch) of frame `frame` to w x h at (ox, oy) of the canvas.  The taps
// index the CROP.  ox is a multiple of 4 (the kernel stores four pixels as one dword).
struct PyrRegionLevelDev {
    uint32_t frame;        // in the sub-batch on the device
    uint32_t cx, cy, cw, ch;
    uint32_t ox, oy, w, h;
    uint32_t xtab, ytab;   // first PyrTap of its columns / rows
    uint32_t unit_first;   // first work unit (a PYR_REGION_TW x PYR_REGION_TH block of destination pixels) of this level image
    uint32_t area;         // != 0: the crop is exactly 2 w x 2 h: dst = (2 x 2 sum + 2) >> 2
    uint32_t pad[3];
};
static_assert(sizeof(PyrRegionLevelDev) == 64, "PyrRegionLevelDev is 64 bytes");
constexpr uint32_t PYR_REGION_TW = 64, PYR_REGION_TH = 16;   // destination pixels per workgroup: 16 x 16 threads of four pixels each

}  // namespace vj
