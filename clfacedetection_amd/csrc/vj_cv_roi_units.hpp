// Records the region pass of the OpenCV profile (vj_cv_roi.hip) shares with the host code that builds and reads
// them (vj_cv_roi_host.cpp, which is compiled without HIP for the sanitizer runs): plain PODs, nothing else.
#pragma once
#include <stdint.h>

namespace vj {

struct CvDet {
    uint32_t x, y, slot, frame;
};

// A region is the sub-image an OpenCV caller would hand over: factors, grid ends and the border rule come from its w x h.
struct CvRoiDev {
    uint32_t frame;          // in the sub-batch whose integral images are on the device
    uint32_t x, y, w, h;     // inside the frame
    uint32_t pad[3];
};
static_assert(sizeof(CvRoiDev) == 32, "CvRoiDev is 32 bytes");
// One unit of work: window row `iy` of (region, factor slot), end_x positions long.
struct CvRoiUnit { uint32_t roi, slot, iy, end_x; };

}  // namespace vj
