// Host planner of CV_HAAR_SCALE_IMAGE inside regions (vj_detect_opencv_rois, route 2) that needs no device: the level
// loop of the scale-image branch (shared with vj_detect_opencv's plan), the resize taps, and the canvases that hold the level images
// of a sub-batch's regions.  Compiled without HIP too: tests/cv_roi_levels_asan_driver.cpp runs it under ASan + UBSan.
#pragma once
#include "vj_cv_roi_host.hpp"

#include <map>
#include <tuple>

namespace vj {

// One evaluated level of HaarDetectObjects' CV_HAAR_SCALE_IMAGE loop (tempcv.cpp:1268-1288) on a W x H image
struct CvLevelHost {
    double factor;         // factor *= scale_factor, in double
    int idx;               // the factor's number, skipped factors included
    int win_w, win_h;      // winSize = cvRound(orig * factor)
    int lw, lh;            // the level image: cvRound(W / factor) x cvRound(H / factor)
    int step;              // factor > 2 ? 1 : 2
    int end_x, end_y;      // grid positions x, y = 0, step, ... < size - window
};
// The loop itself: breaks where the level is smaller than the window or winSize exceeds max_w x max_h, skips levels below min_w x min_h
// and levels without a grid position (a level exactly one window wide or high; *n_empty counts them: the reference resizes and
// integrates them all the same).  VJ_ERR_LIMIT beyond 65536 factors.
int cv_scale_image_levels(int win_w, int win_h, int W, int H, double scale_factor, int min_w, int min_h, int max_w, int max_h,
                          std::vector<CvLevelHost>* out, int* n_empty = nullptr);

// cvResize(CV_INTER_LINEAR), 8-bit: source indices and 11-bit weights of the `dst` columns (rows = false) or rows
// of a `src` -> `dst` resize; area: the 2 x 2 mean's taps.  resize_is_area: the source is exactly twice the destination on both axes.
void build_taps(int src, int dst, bool rows, bool area, PyrTap* out);
bool resize_is_area(int sw, int sh, int dw, int dh);

// The taps of a call: one run per distinct (source length, destination length, rows, area), shared by every level image that has it
struct CvTapCache {
    std::map<std::tuple<int, int, bool, bool>, uint32_t> first;
    std::vector<PyrTap> taps;
    uint32_t get(int src, int dst, bool rows, bool area);
};

// One level image of a canvas: the device record and what the host needs to turn a detection into a rectangle
struct CvRegionLevel {
    int region;            // index in the planner's region list
    CvLevelHost lv;
    uint32_t row_first;    // its first row unit: rows [row_first, row_first + lv.end_y)
};
// A canvas: the level images of regions [first, first + n_regions) of the list, shelf-packed (origins at multiples of 4 columns; what no
// level image covers is never cleared — it cancels in every four-corner difference).
struct CvRegionCanvas {
    size_t n_regions = 0;          // regions taken from the list (those without any level included)
    bool oversized = false;        // the first region's level images do not fit an EMPTY canvas: n_regions = 1, nothing planned —
                                   // the caller sends it through the per-size route
    uint32_t w = 0, h = 0, pitch = 0;
    std::vector<CvRegionLevel> levels;
    std::vector<PyrRegionLevelDev> dev;   // parallel to `levels`
    uint32_t n_empty_levels = 0;   // levels of these regions that have no grid position: no level image, nothing to run
    uint32_t n_pyr_units = 0;
    uint32_t n_rows = 0;           // row units: one per (level image, grid row)
    uint64_t windows = 0;          // grid positions of all level images
};
// Plans the next canvas from regs[first] on: as many regions as fit `budget_px` canvas pixels (width * height; the 32-bit offsets of
// a frame of that size bound it: (w + 1) * (h + 3) < 2^30, h < 65535).  Level images are sorted by height and put on shelves.
int cv_roi_plan_canvas(const std::vector<CvRoiHost>& regs, size_t first, int win_w, int win_h, double scale_factor, int min_w, int min_h,
                       uint64_t budget_px, CvTapCache* taps, CvRegionCanvas* out);

// Which calls the level canvases pay for.  Measured: the per-size route costs about one plan, upload and wait per
// distinct region size and little per region — its calls batch the regions of one size and run the large levels on LDS tiles —, the
// canvases cost per region and nothing per size.  Many regions of few sizes (a first cascade's raw candidates: 2000 regions of 24
// sizes) are faster on the per-size route, regions that nearly all differ in size (grouped faces: 76 of 54) 21 times faster on
// canvases; the break-even lies near 60 regions per size.  The canvases take a call of at most this many regions per distinct
// (w, h) on average.
constexpr int CV_ROI_LEVELS_MAX_REGIONS_PER_SIZE = 32;
bool cv_rois_levels_pay(const vj_roi* rois, int n_rois);

}  // namespace vj
