"""MI355X-native Viola–Jones detect path: a drop-in for the clif/clod detect path of
GabrieleCocco/CLFaceDetection behind the C ABI in include/vj.h (libvjhip.so).

Only what the hot path needs lives here: csrc/ (HIP kernels + C ABI + host planning),
api.py (ctypes mirror of the reference's clod*/clif* functions), data/ (stock cascades
in the compact .vjc form), synth.py (synthetic frames for tests and bench).
"""
from .api import (  # noqa: F401
    CLOD_BLOCK_IMPLEMENTATION, CLOD_PER_STAGE_ITERATIONS, CLOD_PRECOMPUTE_FEATURES,
    CV_HAAR_DO_CANNY_PRUNING, CV_HAAR_DO_ROUGH_SEARCH, CV_HAAR_FIND_BIGGEST_OBJECT, CV_HAAR_SCALE_IMAGE, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH, VJ_FLAG_CV_CHAIN_DEVICE, VJ_FLAG_EQUALIZE_HIST,
    VJ_FLAG_COUNTERS, VJ_FLAG_SIGNED_MEAN, VJ_FLAG_GRID_F64, VJ_FLAG_TILTED_AS_UPRIGHT, VJ_FLAG_SKIP_LIST, VJ_FLAG_SKIP_ROW, Cascade, DetectResult, DeviceFrames, Environment,
    ExtractParams, FrameStream, MixedInfo, MixedOpts, Params, Prep, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VJ_PREP_EQUALIZE, VjError, extract_layout, preprocess_layout,
    clifIntegral, clodDetectObjects, clodInitBuffers, clodInitEnvironment, clodReleaseBuffers,
    clodReleaseEnvironment, cvHaarDetectObjects, cvHaarDetectObjectsForROC, default_params, group_rectangles,
    cvRunHaarClassifierCascade, group_rectangles_levels, load_library, run_windows_opencv,
    CLOD_WINDOW_RESULT_DTYPE, VJ_WINDOW_OUTSIDE, runCascade, run_windows,
    AFFINE_DTYPE, AffineParams, affine_from_eyes, affine_from_rect, align_transforms, extract_affine_layout,
    PaintParams, VJ_PAINT_FILL, VJ_PAINT_OUTLINE, VJ_PAINT_PIXELATE, VJ_PAINT_BLUR, VJ_PAINT_ELLIPSE, paint_layout,
    YuvFrames, YuvParams, VJ_YUV_NV12, VJ_YUV_NV21, VJ_YUV_I420, VJ_YUV_RGB_ORDER, yuv_to_bgr_layout, bgr_to_yuv_layout,
    paint_yuv_layout, extract_yuv_layout, extract_affine_yuv_layout,
    TrackParams, TRACK_RESULT_DTYPE, track_layout, bridge_detections,
)
