"""ctypes binding of libvjhip.so — the host-side mirror of the reference's clif/clod
interface for the detect path.

The reference's public functions (clod.h:61-81, clif.h:42-73) take OpenCV/OpenCL
types; this module keeps their names, argument order and meaning on top of the C ABI
declared in include/vj.h, with numpy arrays standing in for IplImage / CvMat:

    clodInitEnvironment(device_index)            -> Environment
    clodInitBuffers(env, (width, height))
    clodDetectObjects(image, cascade, env, min_window_size, max_window_size,
                      min_neighbors, flags, use_opencl=True) -> DetectResult
    clifIntegral(image, env)                     -> (sum, square_sum)
    clodReleaseBuffers(env); clodReleaseEnvironment(env)

There is no CPU path here: `use_opencl=False` selects the WINDOW SET of the reference's
CPU variants (their skip after a stage-0 reject), still evaluated on the device, and a
missing/unbuildable libvjhip.so or a missing GPU raises VjError — nothing in this package
falls back to the oracle or to numpy.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from dataclasses import dataclass

import numpy as np

from .build import LIB_PATH, build_lib

VJ_MAX_STAGES = 64
VJ_FLAG_COUNTERS = 1 << 0
VJ_FLAG_SIGNED_MEAN = 1 << 1
VJ_FLAG_SKIP_LIST = 1 << 2     # the CLOD_PER_STAGE_ITERATIONS CPU variant's skip over the flattened window list (clod.cpp:729-732)
VJ_FLAG_SKIP_ROW = 1 << 3      # the plain CPU variant: round() positions, skip inside a row (clod.cpp:1409-1432)
VJ_FLAG_GRID_F64 = 1 << 4      # + one of the two above: the same loop of the block variant, whose step is a double (clod.cpp:862)
VJ_FLAG_TILTED_AS_UPRIGHT = 1 << 5   # clod profile: <tilted>1 rectangles count as upright ones, as in the reference (clod.cpp:448-492); else refused
VJ_FLAG_CV_CANNY_PRUNING = 1 << 6    # OpenCV profile: CV_HAAR_DO_CANNY_PRUNING (edge map per frame, a pruning test per visited window)
VJ_FLAG_CV_SCALE_IMAGE = 1 << 7      # OpenCV profile: CV_HAAR_SCALE_IMAGE (the image is scaled, the cascade runs at base size on every grid position)
VJ_FLAG_CV_FIND_BIGGEST = 1 << 8     # OpenCV profile: CV_HAAR_FIND_BIGGEST_OBJECT (largest window first, one grouped object per frame, then its surroundings only)
VJ_FLAG_CV_ROUGH_SEARCH = 1 << 9     # OpenCV profile: CV_HAAR_DO_ROUGH_SEARCH (with find-biggest: the search stops at 0.6 of the object's size, not 0.4)
VJ_FLAG_CV_CHAIN_DEVICE = 1 << 10    # detect_opencv_chain only (flags of the first cascade): regions and units are built on the device, one wait per sub-batch
VJ_PREP_EQUALIZE = 1 << 0            # vj_prep.flags: cv::equalizeHist of the resized image (Environment.preprocess(equalize=True))
VJ_EXTRACT_GRAY = 1 << 0             # vj_extract_params.flags: C = 1, colour sources through BGR2GRAY (Environment.extract(gray=True))
VJ_PAINT_FILL, VJ_PAINT_OUTLINE, VJ_PAINT_PIXELATE, VJ_PAINT_BLUR = 0, 1, 2, 3   # vj_paint_params.mode (Environment.paint(mode=...))
VJ_PAINT_ELLIPSE = 1 << 0            # vj_paint_params.flags: the ellipse inscribed in the mapped rectangle (Environment.paint(ellipse=True))
VJ_YUV_NV12, VJ_YUV_NV21, VJ_YUV_I420 = 0, 1, 2   # vj_yuv_image.layout (YuvFrames.layout, Environment.bgr_to_yuv(layout=...))
VJ_YUV_RGB_ORDER = 1 << 0            # vj_yuv_params.flags: the BGR side is RGB / RGBA (Environment.yuv_to_bgr(rgb=True))
YUV_LAYOUTS = {"nv12": VJ_YUV_NV12, "nv21": VJ_YUV_NV21, "i420": VJ_YUV_I420}
PAINT_MODES = {"fill": VJ_PAINT_FILL, "outline": VJ_PAINT_OUTLINE, "pixelate": VJ_PAINT_PIXELATE, "blur": VJ_PAINT_BLUR}
VJ_EXTRACT_PLANAR = 1 << 1           # vj_extract_params.flags: n x C x h x w instead of n x h x w x C (Environment.extract(planar=True))
VJ_FLAG_EQUALIZE_HIST = 1 << 11      # cv::equalizeHist on every frame, on the device, in front of detect / detect_opencv / detect_opencv_roc / the mixed calls; refused elsewhere

# cvHaarDetectObjects' flags (tempcv.hpp:127-130).  cvHaarDetectObjects below takes only CV_HAAR_DO_CANNY_PRUNING in its `flags`
# argument and refuses the other three values there; their paths are reached through `vj_flags` (VJ_FLAG_CV_SCALE_IMAGE,
# VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH) or Environment.detect_opencv(flags=...).
CV_HAAR_DO_CANNY_PRUNING = 1
CV_HAAR_SCALE_IMAGE = 2
CV_HAAR_FIND_BIGGEST_OBJECT = 4
CV_HAAR_DO_ROUGH_SEARCH = 8

# clod_flags of the reference (clod.h:17-19).  They select among the reference's CPU
# evaluators; the HIP path has one evaluator, so they are accepted and ignored.
CLOD_PRECOMPUTE_FEATURES = 2 << 0
CLOD_BLOCK_IMPLEMENTATION = 2 << 1
CLOD_PER_STAGE_ITERATIONS = 2 << 2

DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


class VjError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str):
        super().__init__(f"{what}: {detail}" if detail else what)
        self.code = code


class CascadeInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("win_w", "win_h", "n_stages", "n_trees", "n_nodes", "n_alpha",
                                          "max_trees_per_stage", "max_nodes_per_tree", "n_tilted", "n_three_rect",
                                          "is_stump_based", "is_stage_tree")]


class Params(C.Structure):
    _fields_ = [("min_w", C.c_int32), ("min_h", C.c_int32), ("max_w", C.c_int32), ("max_h", C.c_int32),
                ("scale_factor", C.c_float), ("min_neighbors", C.c_uint32), ("flags", C.c_uint32),
                ("scale_mask", C.c_uint64 * 2)]


class ScaleInfo(C.Structure):
    _fields_ = [("scale_idx", C.c_int32), ("scale", C.c_float), ("step", C.c_float),
                ("win_w", C.c_int32), ("win_h", C.c_int32),
                ("equ_x", C.c_int32), ("equ_y", C.c_int32), ("equ_w", C.c_int32), ("equ_h", C.c_int32),
                ("area", C.c_uint32), ("nx", C.c_int32), ("ny", C.c_int32), ("accepted", C.c_int32)]


class TileInfo(C.Structure):
    """vj_tile_info: one accepted scale of a plan and, where it runs on LDS tiles, its tile shape."""
    _fields_ = [("scale_idx", C.c_int32), ("scale", C.c_float), ("step", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32),
                ("lds_class", C.c_int32), ("tile_w", C.c_int32), ("tile_h", C.c_int32), ("pitch", C.c_int32), ("rows", C.c_int32),
                ("reach_x", C.c_int32), ("reach_y", C.c_int32), ("lead_scale_idx", C.c_int32), ("tile_row_end", C.c_int32)]


class TilePlanInfo(C.Structure):
    """vj_tile_plan_info: the LDS blocks of a plan's tile launches."""
    _fields_ = [("header_bytes", C.c_uint32), ("gather_reserve_bytes", C.c_uint32), ("max_tile_windows", C.c_uint32),
                ("n_classes", C.c_uint32), ("class_lds", C.c_uint32 * 4), ("class_per_cu", C.c_int32 * 4),
                ("class_tiles", C.c_uint32 * 4)]


class TileCutInfo(C.Structure):
    """vj_tile_cut_info: how a plan divides a frame's windows between the tile chain and the global-gather chain."""
    _fields_ = [("tile_split", C.c_float), ("gather_units", C.c_uint32), ("gather_windows", C.c_uint64),
                ("plan_windows", C.c_uint64)]


VJ_PLAN_TILES_FORMER_SHAPES = 1
VJ_PLAN_TILES_NO_GROUPS = 2


class _Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("stride", C.c_int32),
                ("on_device", C.c_int32), ("channels", C.c_int32)]


class CvParams(C.Structure):
    """vj_cv_params: cvHaarDetectObjects' arguments (OpenCV arithmetic profile)."""
    _fields_ = [("min_w", C.c_int32), ("min_h", C.c_int32), ("scale_factor", C.c_double), ("min_neighbors", C.c_uint32),
                ("flags", C.c_uint32)]


class CvPlanInfo(C.Structure):
    """vj_cv_plan_info: the LDS-tile scales and the stage-tree queue of an OpenCV-profile plan."""
    _fields_ = [("tile_windows", C.c_uint64), ("n_tile_scales", C.c_uint32), ("tree_prefix", C.c_uint32),
                ("tree_queue", C.c_int32), ("tq_shift", C.c_int32), ("tq_split_frames", C.c_int32), ("reserved", C.c_int32)]


class CvChainInfo(C.Structure):
    """vj_cv_chain_info: what the environment's last detect_opencv_chain call did.  handoff: 0 no call yet, 1 on the device, 2 through
    the host, 3 the two public calls."""
    _fields_ = [("handoff", C.c_int32), ("sub_batches", C.c_int32), ("sub_batches_device", C.c_int32), ("reruns", C.c_int32),
                ("regions", C.c_uint64), ("units", C.c_uint64), ("windows", C.c_uint64), ("handoff_ms", C.c_float),
                ("reserved", C.c_int32)]


class CvRoisInfo(C.Structure):
    """vj_cv_rois_info: what the environment's last detect_opencv_rois call did.  route: 0 no call yet, 1 one pass on the frames'
    integral images, 2 one pass on level canvases (VJ_FLAG_CV_SCALE_IMAGE), 3 one detect_opencv call per region size, 4 route 2 with
    some regions sent through route 3."""
    _fields_ = [("route", C.c_int32), ("canvases", C.c_int32), ("canvas_w", C.c_uint32), ("canvas_h", C.c_uint32),
                ("regions", C.c_uint64), ("level_images", C.c_uint64), ("windows", C.c_uint64), ("pyramid_ms", C.c_float),
                ("reserved", C.c_int32)]


class MixedOpts(C.Structure):
    """vj_mixed_opts: speed only.  atlas_px: pixel budget of one atlas (0: default); own_call_px: a group of equal frames with at
    least this many pixels in total gets a batched call of its own (0: default, 2**64 - 1: never)."""
    _fields_ = [("atlas_px", C.c_uint64), ("own_call_px", C.c_uint64)]


class Prep(C.Structure):
    """vj_prep"""
    _fields_ = [("dst_w", C.c_int32), ("dst_h", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ExtractParams(C.Structure):
    """vj_extract_params"""
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("sx", C.c_double), ("sy", C.c_double), ("margin", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class PaintParams(C.Structure):
    """vj_paint_params"""
    _fields_ = [("mode", C.c_int32), ("flags", C.c_uint32), ("sx", C.c_double), ("sy", C.c_double), ("margin", C.c_double),
                ("size", C.c_int32), ("rel", C.c_double), ("color", C.c_uint8 * 4), ("reserved", C.c_uint32)]


class _YuvImage(C.Structure):
    """vj_yuv_image"""
    _fields_ = [("y", C.c_void_p), ("c0", C.c_void_p), ("c1", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("y_stride", C.c_int32), ("c_stride", C.c_int32), ("layout", C.c_int32), ("on_device", C.c_int32)]


class YuvParams(C.Structure):
    """vj_yuv_params"""
    _fields_ = [("channels", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TrackParams(C.Structure):
    """vj_track_params"""
    _fields_ = [("tmpl", C.c_int32), ("radius", C.c_int32), ("sx", C.c_double), ("sy", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AffineParams(C.Structure):
    """vj_affine_params"""
    _fields_ = [("out_w", C.c_int32), ("out_h", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class MixedInfo(C.Structure):
    """vj_mixed_info: what the environment's last detect_mixed / detect_opencv_mixed call did."""
    _fields_ = [("atlases", C.c_int32), ("own_calls", C.c_int32), ("atlas_w", C.c_uint32), ("atlas_h", C.c_uint32),
                ("frames", C.c_uint64), ("frames_atlas", C.c_uint64), ("frames_own_calls", C.c_uint64),
                ("frames_oversized", C.c_uint64), ("windows", C.c_uint64), ("pack_ms", C.c_float), ("reserved", C.c_int32)]


class _Counters(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("stump_evals", C.c_uint64), ("gather_bytes", C.c_uint64),
                ("stage_entered", C.c_uint64 * VJ_MAX_STAGES)]


VJ_MAX_PASSES = 8
VJ_MAX_LAUNCHES = 16
LAUNCH_KINDS = {0: "grid", 1: "queue", 2: "tile", 3: "block"}


class _Launch(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lds_class", C.c_int32), ("stage_begin", C.c_int32), ("stage_end", C.c_int32),
                ("ms", C.c_float), ("lds_bytes", C.c_uint32), ("scale_mask", C.c_uint64 * 2),
                ("stage_entered", C.c_uint64 * VJ_MAX_STAGES)]


class _Timing(C.Structure):
    _fields_ = [("integral_ms", C.c_float), ("cascade_ms", C.c_float), ("total_ms", C.c_float),
                ("n_cascade_launches", C.c_int32), ("pass_ms", C.c_float * VJ_MAX_PASSES),
                ("pass_stage_begin", C.c_int32 * VJ_MAX_PASSES), ("pass_stage_end", C.c_int32 * VJ_MAX_PASSES),
                ("n_launches", C.c_int32), ("launch", _Launch * VJ_MAX_LAUNCHES), ("tile_split", C.c_float),
                ("balance_state", C.c_int32), ("balance_calls", C.c_int32)]


class _Result(C.Structure):
    _fields_ = [("rects", C.c_void_p), ("count", C.c_uint32), ("counters", _Counters), ("timing", _Timing)]


class CvRocParams(C.Structure):
    """vj_cv_roc_params: cvHaarDetectObjectsForROC's arguments (minSize, maxSize, scaleFactor, minNeighbors, flags)."""
    _fields_ = [("min_w", C.c_int32), ("min_h", C.c_int32), ("max_w", C.c_int32), ("max_h", C.c_int32),
                ("scale_factor", C.c_double), ("min_neighbors", C.c_uint32), ("flags", C.c_uint32)]


class _RocResult(C.Structure):
    _fields_ = [("r", _Result), ("reject_levels", C.c_void_p), ("level_weights", C.c_void_p)]


WINDOW_DTYPE = np.dtype([("frame", "<i4"), ("x", "<i4"), ("y", "<i4"), ("scale", "<i4")])                 # vj_window
WINDOW_RESULT_DTYPE = np.dtype([("result", "<i4"), ("reserved", "<i4"), ("stage_sum", "<f8")])           # vj_window_result
CLOD_WINDOW_RESULT_DTYPE = np.dtype([("result", "<i4"), ("variance", "<f4"), ("stage_sum", "<f4"), ("reserved", "<i4")])   # vj_clod_window_result
VJ_WINDOW_OUTSIDE = -2**31   # vj_clod_window_result.result of a window that does not lie inside its frame
RECT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("weight", "<f4"),
                       ("frame", "<i4"), ("scale_idx", "<i4")])
TRACK_RESULT_DTYPE = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("sad", "<u4"), ("sad0", "<u4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"),
                               ("h", "<i4")])                                                                 # vj_track_result
AFFINE_DTYPE = np.dtype([("frame", "<i4"), ("reserved", "<i4"), ("m", "<f8", (6,))])                      # vj_affine
STAGE_DTYPE = np.dtype([("first_tree", "<i4"), ("n_trees", "<i4"), ("threshold", "<f4"), ("parent", "<i4"),
                        ("next", "<i4"), ("child", "<i4")])
TREE_DTYPE = np.dtype([("first_node", "<i4"), ("n_nodes", "<i4"), ("first_alpha", "<i4")])
_RECT_DESC = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("weight", "<f4")])
NODE_DTYPE = np.dtype([("n_rects", "<i4"), ("tilted", "<i4"), ("threshold", "<f4"), ("left", "<i4"),
                       ("right", "<i4"), ("rect", _RECT_DESC, 3)])

# every function include/vj.h declares, with its signature; tests check the library
# exports exactly this set
_SIGNATURES = {
    "vj_strerror": (C.c_char_p, [C.c_int]),
    "vj_last_error": (C.c_char_p, []),
    "vj_cascade_load_xml": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "vj_cascade_load": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "vj_cascade_save": (C.c_int, [C.c_void_p, C.c_char_p]),
    "vj_cascade_from_arrays": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "vj_cascade_free": (None, [C.c_void_p]),
    "vj_cascade_get_info": (C.c_int, [C.c_void_p, C.POINTER(CascadeInfo)]),
    "vj_cascade_stages": (C.c_void_p, [C.c_void_p]),
    "vj_cascade_trees": (C.c_void_p, [C.c_void_p]),
    "vj_cascade_nodes": (C.c_void_p, [C.c_void_p]),
    "vj_cascade_alpha": (C.c_void_p, [C.c_void_p]),
    "vj_cascade_notice": (C.c_char_p, [C.c_void_p]),
    "vj_params_default": (None, [C.POINTER(Params)]),
    "vj_plan_scales": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(ScaleInfo), C.c_int,
                                 C.POINTER(C.c_int)]),
    "vj_plan_feature_table": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ScaleInfo), C.c_void_p, C.c_void_p]),
    "vj_plan_tiles": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_uint32, C.POINTER(TilePlanInfo),
                                C.POINTER(TileInfo), C.c_int, C.POINTER(C.c_int)]),
    "vj_plan_tiles_split": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_uint32, C.c_float,
                                      C.POINTER(TilePlanInfo), C.POINTER(TileCutInfo), C.POINTER(TileInfo), C.POINTER(C.c_uint64),
                                      C.c_int, C.POINTER(C.c_int)]),
    "vj_env_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "vj_env_destroy": (None, [C.c_void_p]),
    "vj_env_reserve": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "vj_env_device_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "vj_env_configure": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    "vj_env_query": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "vj_integral": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vj_integral_image": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vj_integral_batch_sq32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vj_integral_tilted": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vj_grayscale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "vj_canny": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "vj_equalize_hist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "vj_resize_linear": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]),
    "vj_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "vj_host_free": (None, [C.c_void_p, C.c_void_p]),
    "vj_detect_chain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(Params),
                                  C.POINTER(Params), C.POINTER(_Result), C.POINTER(_Result)]),
    "vj_stream_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(Params),
                                   C.POINTER(C.c_void_p)]),
    "vj_stream_submit": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int]),
    "vj_stream_collect": (C.c_int, [C.c_void_p, C.POINTER(_Result)]),
    "vj_stream_destroy": (None, [C.c_void_p]),
    "vj_detect_rois": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(Params),
                                 C.POINTER(_Result)]),
    "vj_detect_opencv": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(CvParams),
                                   C.POINTER(_Result)]),
    "vj_detect_opencv_rois": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(CvParams),
                                        C.POINTER(_Result)]),
    "vj_detect_opencv_chain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(CvParams),
                                         C.POINTER(CvParams), C.POINTER(_Result), C.POINTER(_Result)]),
    "vj_cv_params_default": (None, [C.POINTER(CvParams)]),
    "vj_cv_roc_params_default": (None, [C.POINTER(CvRocParams)]),
    "vj_detect_opencv_roc": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(CvRocParams),
                                       C.POINTER(_RocResult)]),
    "vj_roc_result_free": (None, [C.POINTER(_RocResult)]),
    "vj_run_windows_opencv": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32,
                                        C.c_int, C.c_void_p]),
    "vj_run_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32,
                                 C.c_int, C.c_uint32, C.c_void_p]),
    "vj_run_windows_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vj_cv_chain_info_get": (C.c_int, [C.c_void_p, C.POINTER(CvChainInfo)]),
    "vj_cv_rois_info_get": (C.c_int, [C.c_void_p, C.POINTER(CvRoisInfo)]),
    "vj_cv_plan_info_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(CvParams), C.POINTER(CvPlanInfo)]),
    "vj_detect": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(Params),
                            C.POINTER(_Result)]),
    "vj_detect_mixed": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(Params), C.POINTER(MixedOpts),
                                  C.POINTER(_Result)]),
    "vj_detect_opencv_mixed": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(CvParams), C.POINTER(MixedOpts),
                                         C.POINTER(_Result)]),
    "vj_pack_frames": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(C.c_int),
                                 C.POINTER(C.c_int), C.c_void_p]),
    "vj_mixed_info_get": (C.c_int, [C.c_void_p, C.POINTER(MixedInfo)]),
    "vj_prep_default": (None, [C.POINTER(Prep)]),
    "vj_preprocess_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.POINTER(Prep), C.POINTER(_Image), C.POINTER(C.c_uint64)]),
    "vj_preprocess": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(Prep), C.c_void_p, C.c_uint64, C.POINTER(_Image)]),
    "vj_preprocess_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_extract_default": (None, [C.POINTER(ExtractParams)]),
    "vj_extract_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(ExtractParams), C.c_void_p,
                                    C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vj_extract": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(ExtractParams), C.c_void_p, C.c_uint64]),
    "vj_extract_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_affine_default": (None, [C.POINTER(AffineParams)]),
    "vj_paint_default": (None, [C.POINTER(PaintParams)]),
    "vj_paint_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(PaintParams), C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_uint64)]),
    "vj_paint": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(PaintParams)]),
    "vj_paint_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_yuv_default": (None, [C.POINTER(YuvParams)]),
    "vj_yuv_to_bgr_layout": (C.c_int, [C.POINTER(_YuvImage), C.c_int, C.POINTER(YuvParams), C.POINTER(_Image), C.POINTER(C.c_uint64)]),
    "vj_yuv_to_bgr": (C.c_int, [C.c_void_p, C.POINTER(_YuvImage), C.c_int, C.POINTER(YuvParams), C.c_void_p, C.c_uint64, C.POINTER(_Image)]),
    "vj_bgr_to_yuv_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.POINTER(YuvParams), C.c_int, C.POINTER(_YuvImage), C.POINTER(C.c_uint64)]),
    "vj_bgr_to_yuv": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.POINTER(YuvParams), C.c_int, C.c_void_p, C.c_uint64,
                                C.POINTER(_YuvImage)]),
    "vj_yuv_luma": (C.c_int, [C.POINTER(_YuvImage), C.POINTER(_Image)]),
    "vj_yuv_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_paint_yuv_layout": (C.c_int, [C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(PaintParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "vj_paint_yuv": (C.c_int, [C.c_void_p, C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(PaintParams)]),
    "vj_paint_yuv_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_extract_yuv_layout": (C.c_int, [C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(ExtractParams), C.POINTER(YuvParams),
                                        C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vj_extract_yuv": (C.c_int, [C.c_void_p, C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(ExtractParams), C.POINTER(YuvParams),
                                 C.c_void_p, C.c_uint64]),
    "vj_extract_affine_yuv_layout": (C.c_int, [C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(AffineParams), C.POINTER(YuvParams),
                                               C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vj_extract_affine_yuv": (C.c_int, [C.c_void_p, C.POINTER(_YuvImage), C.c_int, C.c_void_p, C.c_int, C.POINTER(AffineParams), C.POINTER(YuvParams),
                                        C.c_void_p, C.c_uint64]),
    "vj_extract_yuv_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_track_default": (None, [C.POINTER(TrackParams)]),
    "vj_track_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(TrackParams), C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_uint64)]),
    "vj_track": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(TrackParams), C.c_void_p]),
    "vj_track_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vj_extract_affine_layout": (C.c_int, [C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(AffineParams), C.POINTER(C.c_int),
                                           C.POINTER(C.c_uint64)]),
    "vj_extract_affine": (C.c_int, [C.c_void_p, C.POINTER(_Image), C.c_int, C.c_void_p, C.c_int, C.POINTER(AffineParams), C.c_void_p, C.c_uint64]),
    "vj_extract_affine_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "vj_affine_from_rect": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "vj_affine_from_eyes": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                      C.POINTER(C.c_double)]),
    "vj_result_free": (None, [C.POINTER(_Result)]),
    "vj_group_rectangles": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.c_double]),
    "vj_group_rectangles_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "vj_count_windows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(C.c_uint64)]),
    "vj_shard_frames": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vj_shard_scales": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
}

_lib = None


def load_library(build: bool = True) -> C.CDLL:
    """dlopen libvjhip.so (building it first when stale).  Raises if that fails."""
    global _lib
    if _lib is not None:
        return _lib
    path = build_lib() if build else LIB_PATH
    if not os.path.exists(path):
        raise VjError(-1, "libvjhip.so is missing", f"expected at {path}; run clfacedetection_amd/build.py")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = the library does not export what vj.h declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        lib = load_library()
        raise VjError(rc, f"{what} failed ({lib.vj_strerror(rc).decode()})", lib.vj_last_error().decode())


def _order_after_torch(device: int):
    """The library's streams are non-blocking: they wait for no stream of torch's.  A call that hands the C ABI device memory which
    torch may still be writing (DeviceFrames) or using (an out= tensor, a block its allocator recycled) therefore first waits for
    torch's current stream on the environment's device.  Every such call returns only after its own work is complete, so the host
    waits for that stream either way.  Without torch in the process there is nothing to order, and it is not imported for this."""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        torch.cuda.current_stream(device).synchronize()


def default_params(**kw) -> Params:
    p = Params()
    load_library().vj_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "scales":          # iterable of scale indices -> scale_mask; an empty one = no scale (VJ_SCALE_MASK_NONE)
            for i in v:
                if not 0 <= i < 127:
                    raise ValueError("scale indices in a mask must be below 127")
                p.scale_mask[i >> 6] |= 1 << (i & 63)
            if (p.scale_mask[0] | p.scale_mask[1]) == 0:
                p.scale_mask[1] = 1 << 63
        else:
            setattr(p, k, v)
    return p


class Cascade:
    """CvHaarClassifierCascade stand-in (main.cpp:36 `cvLoad`)."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)
        info = CascadeInfo()
        _check(load_library().vj_cascade_get_info(self._h, C.byref(info)), "vj_cascade_get_info")
        self.info = info

    @classmethod
    def load_xml(cls, path: str) -> "Cascade":
        h = C.c_void_p()
        _check(load_library().vj_cascade_load_xml(os.fsencode(path), C.byref(h)), f"vj_cascade_load_xml({path})")
        return cls(h.value)

    @classmethod
    def load(cls, path_or_name: str) -> "Cascade":
        """Load a .vjc file, or a stock cascade by name (e.g. 'frontalface_alt')."""
        path = path_or_name
        if not os.path.exists(path):
            cand = os.path.join(DATA_DIR, f"haarcascade_{path_or_name}.vjc")
            if os.path.exists(cand):
                path = cand
        if path.endswith(".xml"):
            return cls.load_xml(path)
        h = C.c_void_p()
        _check(load_library().vj_cascade_load(os.fsencode(path), C.byref(h)), f"vj_cascade_load({path})")
        return cls(h.value)

    @classmethod
    def from_arrays(cls, win_w: int, win_h: int, stages: np.ndarray, trees: np.ndarray, nodes: np.ndarray,
                    alpha: np.ndarray) -> "Cascade":
        """vj_cascade_from_arrays: a cascade held in memory (STAGE_DTYPE / TREE_DTYPE / NODE_DTYPE arrays + f32 leaf values),
        e.g. converted from a CvHaarClassifierCascade."""
        st = np.ascontiguousarray(stages, STAGE_DTYPE)
        tr = np.ascontiguousarray(trees, TREE_DTYPE)
        nd = np.ascontiguousarray(nodes, NODE_DTYPE)
        al = np.ascontiguousarray(alpha, np.float32)
        h = C.c_void_p()
        _check(load_library().vj_cascade_from_arrays(int(win_w), int(win_h), st.ctypes.data, len(st), tr.ctypes.data, len(tr),
                                                     nd.ctypes.data, len(nd), al.ctypes.data, len(al), C.byref(h)),
               "vj_cascade_from_arrays")
        return cls(h.value)

    def save(self, path: str):
        _check(load_library().vj_cascade_save(self._h, os.fsencode(path)), f"vj_cascade_save({path})")

    def _view(self, fn, dtype, n):
        ptr = fn(self._h)
        buf = (C.c_char * (dtype.itemsize * n)).from_address(ptr)
        return np.frombuffer(buf, dtype, n).copy()

    @property
    def stages(self): return self._view(load_library().vj_cascade_stages, STAGE_DTYPE, self.info.n_stages)
    @property
    def trees(self): return self._view(load_library().vj_cascade_trees, TREE_DTYPE, self.info.n_trees)
    @property
    def nodes(self): return self._view(load_library().vj_cascade_nodes, NODE_DTYPE, self.info.n_nodes)
    @property
    def alpha(self): return self._view(load_library().vj_cascade_alpha, np.dtype("<f4"), self.info.n_alpha)
    @property
    def notice(self) -> str: return load_library().vj_cascade_notice(self._h).decode("latin-1")

    def plan_scales(self, width: int, height: int, params: Params | None = None) -> list[ScaleInfo]:
        p = params or default_params()
        n = C.c_int(0)
        lib = load_library()
        _check(lib.vj_plan_scales(self._h, width, height, C.byref(p), None, 0, C.byref(n)), "vj_plan_scales")
        arr = (ScaleInfo * max(n.value, 1))()
        _check(lib.vj_plan_scales(self._h, width, height, C.byref(p), arr, n.value, C.byref(n)), "vj_plan_scales")
        return list(arr)[:n.value]

    def feature_table(self, width: int, scale: ScaleInfo) -> tuple[np.ndarray, np.ndarray]:
        off = np.zeros((self.info.n_nodes, 3, 4), np.uint32)
        wts = np.zeros((self.info.n_nodes, 3), np.float32)
        _check(load_library().vj_plan_feature_table(self._h, width, C.byref(scale), off.ctypes.data,
                                                    wts.ctypes.data), "vj_plan_feature_table")
        return off, wts

    def plan_tiles(self, width: int, height: int, n_frames: int = 64, params: Params | None = None,
                   flags: int = 0, tile_split: float | None = None) -> tuple[TilePlanInfo, list[TileInfo]]:
        """vj_plan_tiles: the tile shapes of the plan a fresh environment builds for n_frames frames (host only).
        tile_split (vj_plan_tiles_split): the plan at that chain balance, negative = the shipped one; info.cut is then the
        vj_tile_cut_info and every entry carries gather_windows, its windows on the gather chain's first-pass units."""
        p = params or default_params()
        n = C.c_int(0)
        info = TilePlanInfo()
        lib = load_library()
        # (room for every enumerated scale: the plan holds the accepted ones; asking vj_plan_tiles for the count builds the plan twice)
        _check(lib.vj_plan_scales(self._h, width, height, C.byref(p), None, 0, C.byref(n)), "vj_plan_scales")
        arr = (TileInfo * max(n.value, 1))()
        if tile_split is None:
            _check(lib.vj_plan_tiles(self._h, width, height, C.byref(p), n_frames, flags, C.byref(info), arr, n.value, C.byref(n)),
                   "vj_plan_tiles")
            return info, list(arr)[:n.value]
        cut = TileCutInfo()
        gw = (C.c_uint64 * max(n.value, 1))()
        _check(lib.vj_plan_tiles_split(self._h, width, height, C.byref(p), n_frames, flags, float(tile_split), C.byref(info),
                                       C.byref(cut), arr, gw, n.value, C.byref(n)), "vj_plan_tiles_split")
        info.cut = cut
        tiles = list(arr)[:n.value]
        for t, w in zip(tiles, gw):
            t.gather_windows = int(w)
        return info, tiles

    def shard_scales(self, width: int, height: int, rank: int, world: int, params: Params | None = None) -> list[int]:
        """vj_shard_scales: the scale indices of `rank` when one frame is split over `world` ranks by scale."""
        p = params or default_params()
        m = (C.c_uint64 * 2)()
        _check(load_library().vj_shard_scales(self._h, width, height, C.byref(p), world, rank, m), "vj_shard_scales")
        return [k for k in range(127) if (m[k >> 6] >> (k & 63)) & 1]      # bit 127 = VJ_SCALE_MASK_NONE: an empty share

    def count_windows(self, width: int, height: int, params: Params | None = None) -> int:
        p = params or default_params()
        out = C.c_uint64(0)
        _check(load_library().vj_count_windows(self._h, width, height, C.byref(p), C.byref(out)), "vj_count_windows")
        return out.value

    def close(self):
        if self._h:
            load_library().vj_cascade_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class DetectResult:
    """CLODDetectObjectsResult (clod.h:44-47) + provenance, counters and device timing."""
    rects: np.ndarray            # RECT_DTYPE, sorted by (frame, scale_idx, y, x)
    windows: int
    stump_evals: int
    gather_bytes: int
    stage_entered: list
    integral_ms: float
    cascade_ms: float
    total_ms: float
    n_cascade_launches: int
    passes: list = None          # [(stage_begin, stage_end, ms)] per cascade pass
    launches: list = None        # per kernel launch: dict(kind, lds_class, stage_begin, stage_end, ms, lds_bytes, scales)
    tile_split: float = 0.0      # the chain balance the call's plan was built for
    balance_state: int = 0       # 0 static, 1 the workload's feedback search is running, 2 finished
    balance_calls: int = 0       # calls the search has measured so far
    reject_levels: np.ndarray = None   # detect_opencv_roc only: int32, parallel to rects — the stage each window reached
    level_weights: np.ndarray = None   # ... float64: the stage sum it reached it with

    @property
    def match_count(self) -> int:
        return len(self.rects)


class Environment:
    """CLODEnvironmentData stand-in: one HIP device, its stream and its buffers."""

    def __init__(self, device_index: int = 0):
        h = C.c_void_p()
        _check(load_library().vj_env_create(device_index, C.byref(h)), "vj_env_create")
        self._h = h
        self._device = int(device_index)

    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        _check(load_library().vj_env_device_name(self._h, buf, 256), "vj_env_device_name")
        return buf.value.decode()

    def configure(self, key: str, value) -> None:
        """Set a tunable: speed only, results never depend on them.  The keys, their values and defaults are listed in
        include/vj.h and DESIGN.md §7 (e.g. 'pass_split' "4,9,15", 'blocks_per_cu' 8); configure("defaults", "") puts
        every tunable back to what a fresh Environment has."""
        _check(load_library().vj_env_configure(self._h, key.encode(), str(value).encode()), f"vj_env_configure({key})")

    def query(self, key: str) -> str:
        """The current value of a tunable, in the syntax configure accepts."""
        buf = C.create_string_buffer(1024)
        _check(load_library().vj_env_query(self._h, key.encode(), buf, len(buf)), f"vj_env_query({key})")
        return buf.value.decode()

    def reserve(self, width: int, height: int, batch: int = 1):
        _check(load_library().vj_env_reserve(self._h, width, height, batch), "vj_env_reserve")

    def integral(self, gray: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """clifIntegral on a 2-D uint8 image; a 3-D (h, w, 3 | 4) BGR / BGRA image goes through
        clifGrayscaleIntegral's conversion first (vj_integral_image)."""
        if gray.dtype != np.uint8 or gray.ndim not in (2, 3):
            raise ValueError("integral expects a 2-D uint8 image or a (h, w, 3|4) uint8 BGR/BGRA image")
        s = np.empty((gray.shape[0] + 1, gray.shape[1] + 1), np.uint32)
        q = np.empty((gray.shape[0] + 1, gray.shape[1] + 1), np.uint64)
        if gray.ndim == 3:
            g = _pixel_contiguous(gray)
            im = _Image(g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], 0, g.shape[2])
            _check(load_library().vj_integral_image(self._h, C.byref(im), s.ctypes.data, q.ctypes.data), "vj_integral_image")
            return s, q
        g = gray if gray.strides[1] == 1 else np.ascontiguousarray(gray)
        h, w = g.shape
        _check(load_library().vj_integral(self._h, g.ctypes.data, w, h, g.strides[0], s.ctypes.data, q.ctypes.data),
               "vj_integral")
        return s, q

    def integral_sq32(self, frames, color: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """The integral images of a batch of equal-sized frames as detect() and FrameStream keep them on the device
        (vj_integral_batch_sq32): sum and the squared sum mod 2^32, both uint32 (n, h + 1, w + 1).  frames as detect()."""
        imgs, n, keep = self._images(frames, color, self._device)
        if n == 0:
            raise ValueError("integral_sq32 expects at least one frame")
        s = np.empty((n, imgs[0].height + 1, imgs[0].width + 1), np.uint32)
        q = np.empty_like(s)
        _check(load_library().vj_integral_batch_sq32(self._h, imgs, n, s.ctypes.data, q.ctypes.data), "vj_integral_batch_sq32")
        return s, q

    def _one_image(self, img: np.ndarray):
        if img.dtype != np.uint8 or img.ndim not in (2, 3):
            raise ValueError("expected a 2-D uint8 image or a (h, w, 3|4) uint8 BGR/BGRA image")
        g = _pixel_contiguous(img) if img.ndim == 3 else (img if img.strides[1] == 1 else np.ascontiguousarray(img))
        return _Image(g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], 0, g.shape[2] if g.ndim == 3 else 1), g

    def integral_tilted(self, img: np.ndarray) -> np.ndarray:
        """vj_integral_tilted: cvIntegral's tilted sum, (h+1, w+1) uint32."""
        im, keep = self._one_image(img)
        t = np.empty((img.shape[0] + 1, img.shape[1] + 1), np.uint32)
        _check(load_library().vj_integral_tilted(self._h, C.byref(im), t.ctypes.data), "vj_integral_tilted")
        return t

    def grayscale(self, img: np.ndarray) -> np.ndarray:
        """clifGrayscale: the 8-bit gray image the integral kernels see (BGR / BGRA -> gray on the device)."""
        im, keep = self._one_image(img)
        g = np.empty(img.shape[:2], np.uint8)
        _check(load_library().vj_grayscale(self._h, C.byref(im), g.ctypes.data, g.strides[0]), "vj_grayscale")
        return g

    def canny(self, img, color: bool = False) -> np.ndarray:
        """vj_canny: cvCanny(gray, edges, 0, 50, 3) on the device, the edge map CV_HAAR_DO_CANNY_PRUNING computes per frame
        (uint8, 255 on edges, 0 elsewhere).  img: a 2-D uint8 image, a (h, w, 3|4) BGR / BGRA image (color=True), or a
        one-frame DeviceFrames."""
        imgs, n, keep = self._images(img, color, self._device)
        if n != 1:
            raise ValueError("canny takes one image")
        e = np.empty((imgs[0].height, imgs[0].width), np.uint8)
        _check(load_library().vj_canny(self._h, C.byref(imgs[0]), e.ctypes.data, e.strides[0]), "vj_canny")
        return e

    def equalize_hist(self, img, color: bool = False) -> np.ndarray:
        """vj_equalize_hist: cv::equalizeHist of the 8-bit gray image on the device, the image VJ_FLAG_EQUALIZE_HIST puts in front
        of a detect call; returns a (h, w) uint8 array.  img as for canny."""
        imgs, n, keep = self._images(img, color, self._device)
        if n != 1:
            raise ValueError("equalize_hist takes one image")
        d = np.empty((imgs[0].height, imgs[0].width), np.uint8)
        _check(load_library().vj_equalize_hist(self._h, C.byref(imgs[0]), d.ctypes.data, d.strides[0]), "vj_equalize_hist")
        return d

    def resize_linear(self, img, dst_w: int, dst_h: int, color: bool = False) -> np.ndarray:
        """vj_resize_linear: cvResize(gray, dst, CV_INTER_LINEAR) of the 8-bit gray image on the device, one level of the
        pyramid VJ_FLAG_CV_SCALE_IMAGE builds; returns a (dst_h, dst_w) uint8 array.  img as for canny."""
        imgs, n, keep = self._images(img, color, self._device)
        if n != 1:
            raise ValueError("resize_linear takes one image")
        d = np.empty((int(dst_h), int(dst_w)), np.uint8)
        _check(load_library().vj_resize_linear(self._h, C.byref(imgs[0]), int(dst_w), int(dst_h), d.ctypes.data, d.strides[0]),
               "vj_resize_linear")
        return d

    def host_alloc(self, shape, dtype=np.uint8) -> np.ndarray:
        """vj_host_alloc: a page-locked numpy array (freed with host_free) for copy-free frame uploads."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = C.c_void_p()
        _check(load_library().vj_host_alloc(self._h, n, C.byref(ptr)), "vj_host_alloc")
        buf = (C.c_char * n).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype).reshape(shape)
        self.__dict__.setdefault("_pinned", {})[arr.ctypes.data] = ptr.value
        return arr

    def host_free(self, arr: np.ndarray):
        ptr = self.__dict__.get("_pinned", {}).pop(arr.ctypes.data, None)
        if ptr is not None:
            load_library().vj_host_free(self._h, C.c_void_p(ptr))

    def detect_chain(self, first: Cascade, second: Cascade, frames, params_first: Params | None = None,
                     params_second: Params | None = None, color: bool = False):
        """vj_detect_chain: `second` on every raw candidate of `first`, hand-off on the device.  Returns (result_first,
        result_second); result_second.rects['frame'] indexes result_first.rects, x / y are relative to that region."""
        p1 = params_first or default_params()
        p2 = params_second or default_params()
        imgs, n, keep = self._images(frames, color, self._device)
        r1, r2 = _Result(), _Result()
        lib = load_library()
        _check(lib.vj_detect_chain(self._h, first._h, second._h, imgs, n, C.byref(p1), C.byref(p2), C.byref(r1), C.byref(r2)),
               "vj_detect_chain")
        return self._result(lib, r1, first), self._result(lib, r2, second)

    def stream(self, cascade: Cascade, width: int, height: int, max_batch: int, params: Params | None = None,
               channels: int = 1) -> "FrameStream":
        return FrameStream(self, cascade, width, height, max_batch, params or default_params(), channels)

    @staticmethod
    def _images(frames, color: bool, device: int | None = None):
        """-> (ctypes array of vj_image, n, arrays to keep alive).  device: the environment's, for a call that will run on it — device
        frames are then ordered after torch's current stream there (_order_after_torch); None for the host-only layout calls."""
        keep = []
        if isinstance(frames, DeviceFrames):
            if device is not None:
                _order_after_torch(device)
            n = frames.n
            imgs = (_Image * max(n, 1))()
            for i in range(n):
                imgs[i] = _Image(frames.frame_ptr(i), frames.width, frames.height, frames.stride, 1, frames.channels)
            return imgs, n, keep
        if isinstance(frames, np.ndarray) and frames.ndim == (3 if color else 2):
            frames = [frames]
        frames = list(frames)
        n = len(frames)
        imgs = (_Image * max(n, 1))()
        for i, f in enumerate(frames):
            if color:
                if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] not in (3, 4):
                    raise ValueError("color frames must be (h, w, 3|4) uint8 (BGR / BGRA)")
                g = _pixel_contiguous(f)
                keep.append(g)
                imgs[i] = _Image(g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], 0, g.shape[2])
                continue
            if f.dtype != np.uint8 or f.ndim != 2:
                raise ValueError("frames must be 2-D uint8 (8-bit single channel)")
            g = f if f.strides[1] == 1 else np.ascontiguousarray(f)
            keep.append(g)
            imgs[i] = _Image(g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], 0, 1)
        return imgs, n, keep

    def detect_rois(self, cascade: Cascade, frames, rois, params: Params | None = None, color: bool = False) -> DetectResult:
        """vj_detect_rois: `rois` = rows of (frame, x, y, w, h), regions of any sizes (frames of one size and a linear
        cascade: one pass for all of them on the frames' integral images; else one batched pass per region size).  In the
        result rects['frame'] is the ROI's row and x / y are relative to the ROI's origin."""
        p = params or default_params()
        imgs, n, keep = self._images(frames, color, self._device)
        r = np.ascontiguousarray(np.asarray(rois, np.int32).reshape(-1, 5))
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect_rois(self._h, cascade._h, imgs, n, r.ctypes.data, len(r), C.byref(p), C.byref(res)),
               "vj_detect_rois")
        return self._result(lib, res, cascade)

    def detect_opencv(self, cascade: Cascade, frames, min_size=(0, 0), scale_factor: float = 1.1, min_neighbors: int = 0,
                      flags: int = 0, color: bool = False) -> DetectResult:
        """vj_detect_opencv: cvHaarDetectObjects' scale-cascade path (OpenCV arithmetic profile: f64 sums, threshold
        bias, ystep = max(2, factor), skip after a stage-0 reject, border rule).  result.windows = visited positions.
        flags: VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, or VJ_FLAG_CV_SCALE_IMAGE for the CV_HAAR_SCALE_IMAGE branch (an image
        pyramid, the cascade at base size on every grid position; result.windows = grid positions; the canny flag is ignored), or
        VJ_FLAG_CV_FIND_BIGGEST for CV_HAAR_FIND_BIGGEST_OBJECT (the scales from the largest window down, searched on the device; at
        most one rectangle per frame with weight = neighbors and scale_idx = -1; min_neighbors 0 counts as 1; the canny and
        scale-image flags are ignored), with VJ_FLAG_CV_ROUGH_SEARCH for CV_HAAR_DO_ROUGH_SEARCH next to it."""
        imgs, n, keep = self._images(frames, color, self._device)
        p = CvParams(int(min_size[0]), int(min_size[1]), float(scale_factor), int(min_neighbors), int(flags))
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect_opencv(self._h, cascade._h, imgs, n, C.byref(p), C.byref(res)), "vj_detect_opencv")
        return self._result(lib, res, cascade)

    def detect_opencv_rois(self, cascade: Cascade, frames, rois, min_size=(0, 0), scale_factor: float = 1.1, min_neighbors: int = 0,
                           flags: int = 0, color: bool = False) -> DetectResult:
        """vj_detect_opencv_rois: `cascade` in the OpenCV profile inside `rois` = rows of (frame, x, y, w, h); the result equals
        detect_opencv on every region as a sub-image (what cvSetImageROI gives an OpenCV caller): rects['frame'] is the region's
        row, x / y are relative to its origin, regions are grouped one by one.  flags 0 / VJ_FLAG_COUNTERS and frames of one size:
        the frames are integrated once and all regions run in one pass on those integral images; VJ_FLAG_CV_SCALE_IMAGE (with
        VJ_FLAG_COUNTERS, canny pruning or rough search at most) and frames of one size: every region's level images are resized
        into one canvas by one launch and walked by one pass per canvas (unless the call has more than 32 regions per distinct
        region size, which the next route runs faster); other flags or mixed frame sizes: one detect_opencv call per region size.  Same result either way; cv_rois_info() tells which way the last call went."""
        imgs, n, keep = self._images(frames, color, self._device)
        r = np.ascontiguousarray(np.asarray(rois, np.int32).reshape(-1, 5))
        p = CvParams(int(min_size[0]), int(min_size[1]), float(scale_factor), int(min_neighbors), int(flags))
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect_opencv_rois(self._h, cascade._h, imgs, n, r.ctypes.data, len(r), C.byref(p), C.byref(res)),
               "vj_detect_opencv_rois")
        return self._result(lib, res, cascade)

    def detect_opencv_chain(self, first: Cascade, second: Cascade, frames, min_size=(0, 0), scale_factor: float = 1.1,
                            min_neighbors: int = 0, flags: int = 0, min_size_second=(0, 0), scale_factor_second: float = 1.1,
                            min_neighbors_second: int = 0, flags_second: int = 0, color: bool = False):
        """vj_detect_opencv_chain: `first` as detect_opencv runs it, then `second` inside everything it finds (its raw candidates
        when min_neighbors == 0, else its grouped objects) as detect_opencv_rois would; with flags within VJ_FLAG_COUNTERS the
        frames are uploaded and integrated once for both.  Returns (result_first, result_second); result_second.rects['frame']
        indexes result_first.rects, x / y are relative to that region.  frames: numpy arrays or DeviceFrames.
        flags | VJ_FLAG_CV_CHAIN_DEVICE: the hand-off between the two happens on the device (same results; cv_chain_info() tells
        which way the last call went)."""
        imgs, n, keep = self._images(frames, color, self._device)
        p1 = CvParams(int(min_size[0]), int(min_size[1]), float(scale_factor), int(min_neighbors), int(flags))
        p2 = CvParams(int(min_size_second[0]), int(min_size_second[1]), float(scale_factor_second), int(min_neighbors_second),
                      int(flags_second))
        r1, r2 = _Result(), _Result()
        lib = load_library()
        _check(lib.vj_detect_opencv_chain(self._h, first._h, second._h, imgs, n, C.byref(p1), C.byref(p2), C.byref(r1), C.byref(r2)),
               "vj_detect_opencv_chain")
        return self._result(lib, r1, first), self._result(lib, r2, second)

    def detect_opencv_roc(self, cascade: Cascade, frames, min_size=(0, 0), max_size=(0, 0), scale_factor: float = 1.1,
                          min_neighbors: int = 0, flags: int = VJ_FLAG_CV_SCALE_IMAGE, color: bool = False) -> DetectResult:
        """vj_detect_opencv_roc: cvHaarDetectObjectsForROC with outputRejectLevels (the CV_HAAR_SCALE_IMAGE branch).  Every grid
        window that passes the cascade or fails one of its last three stages comes back with .reject_levels (the stage it reached;
        the stage count for a pass) and .level_weights (that stage's f64 sum); stage trees report accepted windows only.
        max_size: the level loop ends at the first window larger than it ((0, 0), or a zero member: the frame).  min_neighbors != 0
        groups with groupRectangles' level overload (group_rectangles_levels).  flags must hold VJ_FLAG_CV_SCALE_IMAGE;
        VJ_FLAG_CV_FIND_BIGGEST and cascades of fewer than 4 stages are refused (VJ_ERR_UNSUPPORTED)."""
        imgs, n, keep = self._images(frames, color, self._device)
        p = CvRocParams(int(min_size[0]), int(min_size[1]), int(max_size[0]), int(max_size[1]), float(scale_factor),
                        int(min_neighbors), int(flags))
        res = _RocResult()
        lib = load_library()
        _check(lib.vj_detect_opencv_roc(self._h, cascade._h, imgs, n, C.byref(p), C.byref(res)), "vj_detect_opencv_roc")
        try:
            m = int(res.r.count)
            levels = np.ctypeslib.as_array((C.c_int32 * m).from_address(res.reject_levels)).copy() if m else np.zeros(0, np.int32)
            weights = np.ctypeslib.as_array((C.c_double * m).from_address(res.level_weights)).copy() if m else np.zeros(0, np.float64)
            out = self._result(lib, res.r, cascade)   # (copies the rectangles and frees them: vj_result_free leaves rects null)
        finally:
            lib.vj_roc_result_free(C.byref(res))
        out.reject_levels, out.level_weights = levels, weights
        return out

    def run_windows_opencv(self, cascade: Cascade, frames, windows, scales, start_stage: int = 0, color: bool = False):
        """vj_run_windows_opencv: see the module-level run_windows_opencv."""
        return _run_windows(*_CV_WINDOWS, self, cascade, frames, windows, scales, start_stage, color)

    def run_windows(self, cascade: Cascade, frames, windows, scales, start_stage: int = 0, flags: int = 0, color: bool = False):
        """vj_run_windows: see the module-level run_windows."""
        return _run_windows(*_CLOD_WINDOWS, self, cascade, frames, windows, scales, start_stage, color, flags)

    def run_windows_timing(self) -> tuple[float, float]:
        """vj_run_windows_timing: (integral_ms, pass_ms) of the last run_windows_opencv or run_windows call, device times summed
        over its sub-batches."""
        i, p = C.c_float(0), C.c_float(0)
        _check(load_library().vj_run_windows_timing(self._h, C.byref(i), C.byref(p)), "vj_run_windows_timing")
        return float(i.value), float(p.value)

    def cv_chain_info(self) -> CvChainInfo:
        """vj_cv_chain_info_get: route, sub-batches, reruns, regions / units / windows and the hand-off kernels' device time of the
        last detect_opencv_chain call."""
        info = CvChainInfo()
        _check(load_library().vj_cv_chain_info_get(self._h, C.byref(info)), "vj_cv_chain_info_get")
        return info

    def cv_rois_info(self) -> CvRoisInfo:
        """vj_cv_rois_info_get: route, regions, level images, canvases (count and the largest one's size), windows and the pyramid
        launches' device time of the last detect_opencv_rois call."""
        info = CvRoisInfo()
        _check(load_library().vj_cv_rois_info_get(self._h, C.byref(info)), "vj_cv_rois_info_get")
        return info

    def cv_plan_info(self, cascade: Cascade, width: int, height: int, n_frames: int, min_size=(0, 0),
                     scale_factor: float = 1.1, min_neighbors: int = 0, flags: int = 0) -> CvPlanInfo:
        """vj_cv_plan_info_get: the plan detect_opencv uses for a batch of n_frames width x height frames."""
        p = CvParams(int(min_size[0]), int(min_size[1]), float(scale_factor), int(min_neighbors), int(flags))
        info = CvPlanInfo()
        _check(load_library().vj_cv_plan_info_get(self._h, cascade._h, width, height, n_frames, C.byref(p), C.byref(info)),
               "vj_cv_plan_info_get")
        return info

    @staticmethod
    def _mixed_images(frames, device: int | None = None):
        """Frames of any sizes -> (ctypes array of vj_image, n, arrays to keep alive).  Items: 2-D uint8 arrays (gray), (h, w, 3 | 4)
        uint8 arrays (BGR / BGRA; rows may be strided views) and DeviceFrames, each of which contributes its frames.  device: as for
        _images."""
        keep, imgs = [], []
        if isinstance(frames, (np.ndarray, DeviceFrames)):
            frames = [frames]
        frames = list(frames)
        if device is not None and any(isinstance(f, DeviceFrames) for f in frames):
            _order_after_torch(device)
        for f in frames:
            if isinstance(f, DeviceFrames):
                imgs += [_Image(f.frame_ptr(i), f.width, f.height, f.stride, 1, f.channels) for i in range(f.n)]
                continue
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8 or f.ndim not in (2, 3) or (f.ndim == 3 and f.shape[2] not in (3, 4)):
                raise ValueError("a frame must be a 2-D uint8 array, a (h, w, 3|4) uint8 array (BGR / BGRA) or DeviceFrames")
            g = _pixel_contiguous(f) if f.ndim == 3 else (f if f.strides[1] == 1 else np.ascontiguousarray(f))
            keep.append(g)
            imgs.append(_Image(g.ctypes.data, g.shape[1], g.shape[0], g.strides[0], 0, g.shape[2] if g.ndim == 3 else 1))
        arr = (_Image * max(len(imgs), 1))(*imgs)
        return arr, len(imgs), keep

    @staticmethod
    def _mixed_opts(atlas_px, own_call_px):
        return MixedOpts(int(atlas_px), min(int(own_call_px), 2**64 - 1))

    def detect_mixed(self, cascade: Cascade, frames, params: Params | None = None, atlas_px: int = 0, own_call_px: int = 0) -> DetectResult:
        """vj_detect_mixed: detect() on a list of frames of ANY sizes, strides and channel counts (see _mixed_images), host and
        device-resident ones mixed, in one call: the result is the concatenation over i of what detect() returns for frames[i]
        alone (rects['frame'] = i, every frame grouped on its own, counters summed).  Groups of equal frames with at least
        own_call_px pixels take a batched call of their own; the others are packed into atlases on the device, integrated once and
        run as regions.  atlas_px / own_call_px change speed only; mixed_info() tells what the last call did."""
        p = params or default_params()
        imgs, n, keep = self._mixed_images(frames, self._device)
        o = self._mixed_opts(atlas_px, own_call_px)
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect_mixed(self._h, cascade._h, imgs, n, C.byref(p), C.byref(o), C.byref(res)), "vj_detect_mixed")
        return self._result(lib, res, cascade)

    def detect_opencv_mixed(self, cascade: Cascade, frames, min_size=(0, 0), scale_factor: float = 1.1, min_neighbors: int = 0,
                            flags: int = 0, atlas_px: int = 0, own_call_px: int = 0) -> DetectResult:
        """vj_detect_opencv_mixed: the same for detect_opencv (every flag of it; those whose result needs the image alone — canny
        pruning without scale-image, find-biggest — run per group of equal frames, without an atlas)."""
        imgs, n, keep = self._mixed_images(frames, self._device)
        p = CvParams(int(min_size[0]), int(min_size[1]), float(scale_factor), int(min_neighbors), int(flags))
        o = self._mixed_opts(atlas_px, own_call_px)
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect_opencv_mixed(self._h, cascade._h, imgs, n, C.byref(p), C.byref(o), C.byref(res)), "vj_detect_opencv_mixed")
        return self._result(lib, res, cascade)

    def pack_frames(self, frames, atlas_px: int = 0):
        """vj_pack_frames: the first atlas a mixed call would make of `frames` -> (atlas as a (h, w) uint8 array, origins as an
        (n, 2) int32 array of (x, y), -1 -1 for a frame that is not in it).  A frame's gray image lies at its origin; what no frame
        covers is 0."""
        imgs, n, keep = self._mixed_images(frames, self._device)
        lib = load_library()
        w, h = C.c_int(0), C.c_int(0)
        origins = np.full((n, 2), -1, np.int32)
        _check(lib.vj_pack_frames(self._h, imgs, n, int(atlas_px), None, 0, C.byref(w), C.byref(h), origins.ctypes.data), "vj_pack_frames")
        atlas = np.zeros((h.value, w.value), np.uint8)
        if atlas.size:
            _check(lib.vj_pack_frames(self._h, imgs, n, int(atlas_px), atlas.ctypes.data, atlas.strides[0], C.byref(w), C.byref(h),
                                      origins.ctypes.data), "vj_pack_frames")
        return atlas, origins

    @staticmethod
    def _prep_args(frames, size, fx, fy, equalize, color):
        """-> (ctypes array of vj_image, n, arrays to keep alive, vj_prep).  frames: as detect() (one array, a batch, DeviceFrames; color=True
        for BGR / BGRA arrays) or, as a list without color=True, as detect_mixed(): gray and BGR / BGRA arrays and DeviceFrames of any sizes."""
        if (fx is None) != (fy is None):
            raise ValueError("fx and fy go together")
        if size is not None and fx is not None:
            raise ValueError("size or fx / fy, not both")
        if color or isinstance(frames, (np.ndarray, DeviceFrames)):
            imgs, n, keep = Environment._images(frames, color)
        else:
            imgs, n, keep = Environment._mixed_images(frames)
        p = Prep()
        load_library().vj_prep_default(C.byref(p))
        if size is not None:
            p.dst_w, p.dst_h = int(size[0]), int(size[1])
        if fx is not None:
            p.fx, p.fy = float(fx), float(fy)
        p.flags = VJ_PREP_EQUALIZE if equalize else 0
        return imgs, n, keep, p

    @staticmethod
    def preprocess_layout(frames, size=None, fx=None, fy=None, equalize: bool = False, color: bool = False):
        """vj_preprocess_layout (host only): where preprocess() puts every output image -> ([(offset, width, height, stride)], bytes)."""
        imgs, n, keep, p = Environment._prep_args(frames, size, fx, fy, equalize, color)
        out = (_Image * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(load_library().vj_preprocess_layout(imgs, n, C.byref(p), out, C.byref(nbytes)), "vj_preprocess_layout")
        return [(int(out[i].data or 0), out[i].width, out[i].height, out[i].stride) for i in range(n)], int(nbytes.value)

    def preprocess(self, frames, size=None, fx=None, fy=None, equalize: bool = False, color: bool = False, out=None) -> list:
        """vj_preprocess: the front end of an OpenCV caller's detect call on the device — BGR2GRAY, resize(INTER_LINEAR)
        to size = (w, h) or by the factors fx, fy (neither: no resize), then with equalize=True equalizeHist of the resized image — for
        all frames in one call, device in, device out.  frames: see _prep_args.  Returns a list of DeviceFrames (gray, in device
        memory): ONE entry of n frames when all outputs share a size — it goes straight into detect(), detect_opencv_chain() and the
        rest —, else one entry per frame, which detect_mixed() takes as they are.  out: a torch.uint8 tensor on this device of at
        least preprocess_layout()'s bytes; None: one is allocated.  The returned objects keep it alive."""
        import torch
        imgs, n, keep, p = self._prep_args(frames, size, fx, fy, equalize, color)
        lib = load_library()
        res = (_Image * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(lib.vj_preprocess_layout(imgs, n, C.byref(p), res, C.byref(nbytes)), "vj_preprocess_layout")
        if out is None:
            out = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=torch.device("cuda", self._device))
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous torch.uint8 tensor in device memory")
        _order_after_torch(self._device)       # after the allocation: device frames, a caller's `out`, and a block the allocator recycled
        _check(lib.vj_preprocess(self._h, imgs, n, C.byref(p), C.c_void_p(out.data_ptr()), out.numel(), res), "vj_preprocess")
        if n == 0:
            return []
        r = [DeviceFrames(int(res[i].data), 1, res[i].height, res[i].width, res[i].stride, 1, 0, out) for i in range(n)]
        if all((f.width, f.height) == (r[0].width, r[0].height) for f in r):
            return [DeviceFrames(r[0].ptr, n, r[0].height, r[0].width, r[0].stride, 1, (r[1].ptr - r[0].ptr) if n > 1 else 0, out)]
        return r

    def preprocess_timing(self) -> float:
        """vj_preprocess_timing: device time of the last preprocess() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_preprocess_timing(self._h, C.byref(ms)), "vj_preprocess_timing")
        return float(ms.value)

    @staticmethod
    def _extract_args(frames, rects, size, scale, margin, gray, planar, color):
        """-> (ctypes array of vj_image, n, arrays to keep alive, (n, 5) int32 regions, vj_extract_params).  frames: as preprocess().
        rects: a RECT_DTYPE array (its frame, x, y, w, h fields) or rows of (frame, x, y, w, h)."""
        if color or isinstance(frames, (np.ndarray, DeviceFrames)):
            imgs, n, keep = Environment._images(frames, color)
        else:
            imgs, n, keep = Environment._mixed_images(frames)
        if isinstance(rects, np.ndarray) and rects.dtype.names is not None:
            r = np.stack([np.asarray(rects[k], np.int32).reshape(-1) for k in ("frame", "x", "y", "w", "h")], axis=1)
        else:
            r = np.asarray(rects)
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError("rects must be a RECT_DTYPE array or integer rows of (frame, x, y, w, h)")
            r = r.astype(np.int32).reshape(-1, 5)
        r = np.ascontiguousarray(r, np.int32)
        p = ExtractParams()
        load_library().vj_extract_default(C.byref(p))
        p.out_w, p.out_h = int(size[0]), int(size[1])
        p.sx, p.sy = float(scale[0]), float(scale[1])
        p.margin = float(margin)
        p.flags = (VJ_EXTRACT_GRAY if gray else 0) | (VJ_EXTRACT_PLANAR if planar else 0)
        return imgs, n, keep, r, p

    @staticmethod
    def extract_layout(frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False,
                       color: bool = False):
        """vj_extract_layout (host only): what extract() will cut -> ((n, 5) int32 rows of the mapped source regions (frame, x, y, w, h),
        which may lie outside their frames; channels of the output; bytes of the output)."""
        imgs, n, keep, r, p = Environment._extract_args(frames, rects, size, scale, margin, gray, planar, color)
        src = np.zeros((len(r), 5), np.int32)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(load_library().vj_extract_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), src.ctypes.data, C.byref(ch), C.byref(nbytes)),
               "vj_extract_layout")
        return src, int(ch.value), int(nbytes.value)

    def extract(self, frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False,
                color: bool = False, out=None):
        """vj_extract: the pixels inside rectangles, at one fixed size, on the device.  Region (frame, x, y, w, h) is
        mapped to source pixels as OpenCV's facedetect sample maps its boxes (cvRound of the coordinates times scale = (sx, sy)), grown
        by cvRound(side * margin) on every side, cut out with the frame's border replicated (never clipped) and resized to
        size = (w, h) with vj_resize_linear's arithmetic per channel; gray=True: one channel through BGR2GRAY.  frames: as preprocess()
        — the full-resolution frames, e.g. the DeviceFrames preprocess() was given.  Returns a torch.uint8 device tensor of shape
        (n, h, w, C), or (n, C, h, w) with planar=True.  out: a contiguous torch.uint8 tensor on this device with that many elements;
        None: one is allocated."""
        import torch
        imgs, n, keep, r, p = self._extract_args(frames, rects, size, scale, margin, gray, planar, color)
        lib = load_library()
        src = np.zeros((len(r), 5), np.int32)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(lib.vj_extract_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), src.ctypes.data, C.byref(ch), C.byref(nbytes)), "vj_extract_layout")
        shape = (len(r), ch.value, p.out_h, p.out_w) if planar else (len(r), p.out_h, p.out_w, ch.value)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self._device))
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous torch.uint8 tensor in device memory")
        if out.numel() != int(nbytes.value):
            raise ValueError(f"out must hold {int(nbytes.value)} bytes, the shape {shape}; it holds {out.numel()}")
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_extract(self._h, imgs, n, r.ctypes.data, len(r), C.byref(p), C.c_void_p(out.data_ptr()), out.numel()), "vj_extract")
        return out.view(shape)

    def extract_timing(self) -> float:
        """vj_extract_timing: device time of the last extract() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_extract_timing(self._h, C.byref(ms)), "vj_extract_timing")
        return float(ms.value)

    @staticmethod
    def _paint_images(frames, color, write: bool = True):
        """-> (ctypes array of vj_image, n, objects to keep alive, True if a device frame is among them).  frames: a DeviceFrames, a
        uint8 CUDA tensor (DeviceFrames.from_torch), a writeable uint8 numpy array — one frame or a batch, as detect() reads its
        shape, color=True for BGR / BGRA — or a list of these, each array then one frame (2-D gray, 3-D BGR / BGRA).  The frames are
        painted IN PLACE: an array the call would have to copy (read-only, another dtype, pixels not contiguous) is a ValueError.
        write=False (track(), which only reads them): a read-only array is taken too."""
        def is_tensor(f):
            return not isinstance(f, (np.ndarray, DeviceFrames)) and hasattr(f, "data_ptr") and hasattr(f, "is_cuda")

        why = "paint() writes into its frames" if write else "track() reads its frames where they lie"

        def one(f, ndim):
            if not isinstance(f, np.ndarray) or f.dtype != np.uint8:
                raise ValueError(f"{why}: a host frame must be a uint8 numpy array (no copy is made)")
            if f.ndim != ndim or (ndim == 3 and f.shape[2] not in (3, 4)):
                raise ValueError("a host frame must be a 2-D uint8 array or a (h, w, 3|4) uint8 array (BGR / BGRA)")
            if write and not f.flags.writeable:
                raise ValueError("paint() writes into its frames: a read-only array cannot be painted (no copy is made)")
            if f.shape[0] == 0 or f.shape[1] == 0:
                raise ValueError("a frame must not be empty")
            if (ndim == 3 and (f.strides[2] != 1 or f.strides[1] != f.shape[2])) or (ndim == 2 and f.strides[1] != 1) or f.strides[0] <= 0:
                raise ValueError(f"{why}: the pixels of a row must be contiguous (no copy is made)")
            return _Image(f.ctypes.data, f.shape[1], f.shape[0], f.strides[0], 0, f.shape[2] if ndim == 3 else 1)

        items = frames if isinstance(frames, (list, tuple)) else [frames]
        batch_ok = not isinstance(frames, (list, tuple))
        imgs, keep, dev = [], [], False
        for f in items:
            if is_tensor(f):
                if not f.is_cuda or f.dtype.itemsize != 1:
                    raise ValueError("a tensor frame must be a uint8 CUDA tensor")
                keep.append(f)
                f = DeviceFrames.from_torch(f)
            if isinstance(f, DeviceFrames):
                dev = True
                keep.append(f)
                imgs += [_Image(f.frame_ptr(i), f.width, f.height, f.stride, 1, f.channels) for i in range(f.n)]
                continue
            if not isinstance(f, np.ndarray):
                raise ValueError("frames must be DeviceFrames, uint8 CUDA tensors, writeable uint8 numpy arrays or a list of these")
            keep.append(f)
            nd = 3 if (color or (not batch_ok and f.ndim == 3)) else 2
            if batch_ok and f.ndim == nd + 1:
                imgs += [one(f[i], nd) for i in range(f.shape[0])]
            else:
                imgs.append(one(f, nd))
        arr = (_Image * max(len(imgs), 1))(*imgs)
        return arr, len(imgs), keep, dev

    @staticmethod
    def _paint_args(frames, rects, mode, size, rel, scale, margin, ellipse, fill, color):
        imgs, n, keep, dev = Environment._paint_images(frames, color)
        if isinstance(rects, np.ndarray) and rects.dtype.names is not None:
            r = np.stack([np.asarray(rects[k], np.int32).reshape(-1) for k in ("frame", "x", "y", "w", "h")], axis=1)
        else:
            r = np.asarray(rects)
            if r.size and not np.issubdtype(r.dtype, np.integer):
                raise ValueError("rects must be a RECT_DTYPE array or integer rows of (frame, x, y, w, h)")
            r = r.astype(np.int32).reshape(-1, 5)
        r = np.ascontiguousarray(r, np.int32)
        p = PaintParams()
        load_library().vj_paint_default(C.byref(p))
        if isinstance(mode, str):
            if mode not in PAINT_MODES:
                raise ValueError(f"mode must be one of {sorted(PAINT_MODES)} or a VJ_PAINT_* value")
            mode = PAINT_MODES[mode]
        p.mode = int(mode)
        p.flags = VJ_PAINT_ELLIPSE if ellipse else 0
        p.sx, p.sy = float(scale[0]), float(scale[1])
        p.margin = float(margin)
        p.size = int(size)
        p.rel = float(rel)
        fill = tuple(int(v) for v in (fill if np.ndim(fill) else (fill,) * 4))
        if len(fill) > 4 or any(not 0 <= v <= 255 for v in fill):
            raise ValueError("fill: up to four values of 0 .. 255, one per channel")
        for c, v in enumerate(fill + (0,) * (4 - len(fill))):
            p.color[c] = v
        return imgs, n, keep, dev, r, p

    @staticmethod
    def paint_layout(frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
                     ellipse: bool = False, color: bool = False):
        """vj_paint_layout (host only): what paint() will touch -> ((n, 5) int32 rows of the clipped rectangles (frame, x, y, w, h),
        w = h = 0 where nothing is painted; (n,) int32 sizes — the thickness, the cell side or the blur's kernel side, 0 for "fill";
        the scratch bytes of the call run as one slice)."""
        imgs, n, keep, dev, r, p = Environment._paint_args(frames, rects, mode, size, rel, scale, margin, ellipse, 0, color)
        clipped = np.zeros((len(r), 5), np.int32)
        sizes = np.zeros(len(r), np.int32)
        nbytes = C.c_uint64(0)
        _check(load_library().vj_paint_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), clipped.ctypes.data, sizes.ctypes.data,
                                              C.byref(nbytes)), "vj_paint_layout")
        return clipped, sizes, int(nbytes.value)

    def paint(self, frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
              ellipse: bool = False, fill=(0, 0, 0, 0), color: bool = False):
        """vj_paint: the pixels inside, or around, rectangles changed IN PLACE, on the device.  mode: "blur" (a box
        blur of the region, its border replicated), "pixelate" (cells replaced by their mean), "fill" (the colour `fill`, one value
        per channel) or "outline" (a frame of that colour along the rectangle, cvRectangle's use).  size: the blur's kernel side, the
        cell side or the line's thickness in pixels; 0: rel times the mapped region's shorter side.  scale, margin, rects: as
        extract().  ellipse=True: the ellipse inscribed in the rectangle instead of the rectangle.  Where regions overlap the
        later one wins, every value computed from the frames as they were before the call.  frames: see _paint_images — device
        frames are painted where they lie, host arrays through a staged copy of the touched rows.  Returns `frames`."""
        imgs, n, keep, dev, r, p = self._paint_args(frames, rects, mode, size, rel, scale, margin, ellipse, fill, color)
        _order_after_torch(self._device)       # work queued on the frames (a decoder, a copy_) has written them before they are painted
        _check(load_library().vj_paint(self._h, imgs, n, r.ctypes.data, len(r), C.byref(p)), "vj_paint")
        return frames

    def paint_timing(self) -> float:
        """vj_paint_timing: device time of the last paint() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_paint_timing(self._h, C.byref(ms)), "vj_paint_timing")
        return float(ms.value)

    @staticmethod
    def _paint_yuv_args(frames, rects, mode, size, rel, scale, margin, ellipse, fill, layout):
        """-> (ctypes array of vj_yuv_image, n, objects to keep alive, (n, 5) int32 rows, vj_paint_params).  frames: a YuvFrames; a
        uint8 CUDA tensor of stacked (n, h * 3 // 2, w) frames (YuvFrames.from_torch with `layout`); a writeable uint8 numpy array of
        stacked frames, (n, h * 3 // 2, w) or one (h * 3 // 2, w); a tuple of a frame's planes; or a list of these.  The frames are
        painted IN PLACE: an array the call would have to copy (read-only, rows whose bytes are not contiguous, stacked i420 frames
        whose rows do not follow each other) is a ValueError."""
        def is_tensor(f):
            return not isinstance(f, (np.ndarray, YuvFrames, tuple)) and hasattr(f, "data_ptr") and hasattr(f, "is_cuda")

        lay = Environment._yuv_layout_id(layout)

        def host(a, stacked):
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8:
                raise ValueError("paint_yuv() writes into its frames: a host frame must be a uint8 numpy array (no copy is made)")
            if not a.flags.writeable:
                raise ValueError("paint_yuv() writes into its frames: a read-only array cannot be painted (no copy is made)")
            if a.ndim < 2 or a.strides[-1] != 1 or a.strides[-2] <= 0 or (stacked and lay == VJ_YUV_I420 and a.strides[-2] != a.shape[-1]):
                raise ValueError("paint_yuv() writes into its frames: the bytes of a row must be contiguous, and the rows of a stacked "
                                 "i420 frame must follow each other (no copy is made)")
            return a

        flat = []
        for f in (frames if isinstance(frames, list) else [frames]):
            if is_tensor(f):
                if not f.is_cuda or f.dtype.itemsize != 1:
                    raise ValueError("a tensor frame must be a uint8 CUDA tensor")
                f = YuvFrames.from_torch(f if f.dim() == 3 else f[None], lay)
            elif isinstance(f, tuple):
                f = tuple(host(a, False) for a in f)
            elif not isinstance(f, YuvFrames):
                f = host(f, True)
            flat.append(f)
        imgs, n, keep = Environment._yuv_images(flat, lay)
        _, _, _, _, r, p = Environment._paint_args(np.zeros((2, 2), np.uint8), rects, mode, size, rel, scale, margin, ellipse, 0, False)
        fill = tuple(int(v) for v in (fill if np.ndim(fill) else (fill,) * 3))
        if len(fill) > 3 or any(not 0 <= v <= 255 for v in fill):
            raise ValueError("fill: up to three values of 0 .. 255: B, G, R")
        for c, v in enumerate(fill + (0,) * (3 - len(fill))):
            p.color[c] = v
        return imgs, n, keep + flat, r, p

    @staticmethod
    def paint_yuv_layout(frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
                         ellipse: bool = False, layout="nv12"):
        """vj_paint_yuv_layout (host only): what paint_yuv() will touch -> ((n, 5) int32 rows of K (frame, x, y, w, h) in luma pixels;
        (n, 5) rows of Kc in chroma samples — w = h = 0 where nothing is painted; (n,) int32 luma sizes and (n,) chroma sizes — the
        thickness, the cell side or the blur's kernel side, 0 for "fill"; the scratch bytes of the call run as one slice)."""
        imgs, n, keep, r, p = Environment._paint_yuv_args(frames, rects, mode, size, rel, scale, margin, ellipse, 0, layout)
        clipped, chroma = np.zeros((len(r), 5), np.int32), np.zeros((len(r), 5), np.int32)
        sizes, csizes = np.zeros(len(r), np.int32), np.zeros(len(r), np.int32)
        nbytes = C.c_uint64(0)
        _check(load_library().vj_paint_yuv_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), clipped.ctypes.data, chroma.ctypes.data,
                                                  sizes.ctypes.data, csizes.ctypes.data, C.byref(nbytes)), "vj_paint_yuv_layout")
        return clipped, chroma, sizes, csizes, int(nbytes.value)

    def paint_yuv(self, frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
                  ellipse: bool = False, fill=(0, 0, 0), layout="nv12"):
        """vj_paint_yuv: rectangles painted into NV12 / NV21 / I420 frames IN PLACE, on the device, without the BGR copy (DESIGN.md
        §4.23).  rects are in luma pixels; mode, size, rel, scale, margin, ellipse: as paint().  fill: B, G, R, converted once to
        (Y, U, V).  The Y plane becomes what paint() makes of it as a gray frame; a chroma sample is painted when any of its four luma
        pixels is, with halved sizes.  layout: of tensors and host arrays (a YuvFrames carries its own).  frames: see
        _paint_yuv_args — device frames are painted where they lie, host arrays through a staged copy of the touched rows.
        Returns `frames`."""
        imgs, n, keep, r, p = self._paint_yuv_args(frames, rects, mode, size, rel, scale, margin, ellipse, fill, layout)
        _order_after_torch(self._device)       # work queued on the frames (a decoder, a copy_) has written them before they are painted
        _check(load_library().vj_paint_yuv(self._h, imgs, n, r.ctypes.data, len(r), C.byref(p)), "vj_paint_yuv")
        return frames

    def paint_yuv_timing(self) -> float:
        """vj_paint_yuv_timing: device time of the last paint_yuv() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_paint_yuv_timing(self._h, C.byref(ms)), "vj_paint_yuv_timing")
        return float(ms.value)

    @staticmethod
    def _track_args(frames, rows, tmpl, radius, scale, color):
        """-> (ctypes array of vj_image, n, objects to keep alive, (n, 6) int32 rows, vj_track_params).  frames: as paint() takes them
        (_paint_images), read-only arrays included; rows: integer rows of (src_frame, dst_frame, x, y, w, h)."""
        imgs, n, keep, dev = Environment._paint_images(frames, color, write=False)
        r = np.asarray(rows)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("rows must be integer rows of (src_frame, dst_frame, x, y, w, h)")
        r = np.ascontiguousarray(r.astype(np.int32).reshape(-1, 6))
        p = TrackParams()
        load_library().vj_track_default(C.byref(p))
        p.tmpl, p.radius = int(tmpl), int(radius)
        p.sx, p.sy = float(scale[0]), float(scale[1])
        return imgs, n, keep, r, p

    @staticmethod
    def track_layout(frames, rows, tmpl: int = 32, radius: int = 8, scale=(1.0, 1.0), color: bool = False):
        """vj_track_layout (host only): what track() will match -> ((n, 5) int32 rows (src_frame, x0, y0, w0, h0) of the templates'
        mapped source regions; (n, 5) int32 rows (dst_frame, X, Y, Wm, Hm) of the search patches'; the scratch bytes of the call run
        as one slice).  The regions may lie outside their frames."""
        imgs, n, keep, r, p = Environment._track_args(frames, rows, tmpl, radius, scale, color)
        tr, sr = np.zeros((len(r), 5), np.int32), np.zeros((len(r), 5), np.int32)
        nbytes = C.c_uint64(0)
        _check(load_library().vj_track_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), tr.ctypes.data, sr.ctypes.data, C.byref(nbytes)),
               "vj_track_layout")
        return tr, sr, int(nbytes.value)

    def track(self, frames, rows, tmpl: int = 32, radius: int = 8, scale=(1.0, 1.0), color: bool = False) -> np.ndarray:
        """vj_track: block matching on the device.  Row (src_frame, dst_frame, x, y, w, h): the box, mapped with
        scale = (sx, sy) as extract() maps it, is cut from src_frame as a tmpl x tmpl gray patch and looked for in dst_frame at the
        (2 radius + 1)^2 displacements of -radius .. radius patch pixels around its own position, by the sum of absolute differences;
        on equal sums the shorter move wins.  frames: as paint() takes them, read-only arrays included; they are not written.
        Returns a TRACK_RESULT_DTYPE array: dx, dy (patch pixels), sad, sad0 (the sum at (0, 0)) and the box x, y, w, h in dst_frame,
        in SOURCE pixels (what paint() takes with scale = (1, 1))."""
        imgs, n, keep, r, p = self._track_args(frames, rows, tmpl, radius, scale, color)
        out = np.zeros(len(r), TRACK_RESULT_DTYPE)
        _order_after_torch(self._device)       # work queued on the frames (a decoder, a copy_) has written them before they are read
        _check(load_library().vj_track(self._h, imgs, n, r.ctypes.data, len(r), C.byref(p), out.ctypes.data), "vj_track")
        return out

    def track_timing(self):
        """vj_track_timing: device time of the last track() call (events around its copies and launches) and of its match launches
        alone -> (ms, match_ms)."""
        ms, match = C.c_float(0), C.c_float(0)
        _check(load_library().vj_track_timing(self._h, C.byref(ms), C.byref(match)), "vj_track_timing")
        return float(ms.value), float(match.value)

    @staticmethod
    def _yuv_layout_id(layout) -> int:
        if isinstance(layout, str):
            if layout.lower() not in YUV_LAYOUTS:
                raise ValueError('layout must be "nv12", "nv21" or "i420"')
            return YUV_LAYOUTS[layout.lower()]
        return int(layout)

    @staticmethod
    def _yuv_images(frames, layout):
        """4:2:0 frames -> (ctypes array of vj_yuv_image, n, arrays to keep alive).  frames: YuvFrames;
        a numpy (n, h * 3 // 2, w) uint8 array of stacked frames (what OpenCV and the decoders hand out: the Y plane, the chroma
        below it), or one (h * 3 // 2, w) frame; a tuple of a frame's planes (y, uv) or (y, u, v), 2-D uint8 arrays whose rows may be
        strided views; or a list of any of these, of differing sizes.  layout: of the host frames (a YuvFrames carries its own)."""
        lay = Environment._yuv_layout_id(layout)
        keep, imgs = [], []

        def plane(a):
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2:
                raise ValueError("a plane must be a 2-D uint8 array")
            g = a if a.strides[1] == 1 else np.ascontiguousarray(a)
            keep.append(g)
            return g

        def stacked(a):
            if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] % 3 != 0 or a.shape[0] < 3:
                raise ValueError("a stacked 4:2:0 frame is a (h * 3 // 2, w) uint8 array")
            h, w = a.shape[0] * 2 // 3, a.shape[1]
            if lay == VJ_YUV_I420:   # the U and V planes are runs of w / 2 * h / 2 bytes: the rows must follow each other
                g = plane(np.ascontiguousarray(a))
                base = g.ctypes.data + w * h
                imgs.append(_YuvImage(g.ctypes.data, base, base + (w // 2) * (h // 2), w, h, w, w // 2, lay, 0))
            else:
                g = plane(a)
                imgs.append(_YuvImage(g.ctypes.data, g.ctypes.data + h * g.strides[0], None, w, h, g.strides[0], g.strides[0], lay, 0))

        if isinstance(frames, (YuvFrames, tuple)) or (isinstance(frames, np.ndarray) and frames.ndim == 2):
            frames = [frames]
        for f in list(frames):
            if isinstance(f, YuvFrames):
                imgs += [_YuvImage(f.ptr_y + i * f.frame_bytes, f.ptr_c0 + i * f.frame_bytes, (f.ptr_c1 + i * f.frame_bytes) if f.ptr_c1 else None,
                                   f.width, f.height, f.y_stride, f.c_stride, f.layout, 1) for i in range(f.n)]
            elif isinstance(f, tuple):
                if len(f) != (3 if lay == VJ_YUV_I420 else 2):
                    raise ValueError("planes: (y, uv) for nv12 / nv21, (y, u, v) for i420")
                p = [plane(a) for a in f]
                if any(q.strides[0] != p[1].strides[0] for q in p[1:]):
                    raise ValueError("the u and v planes share one row stride")
                imgs.append(_YuvImage(p[0].ctypes.data, p[1].ctypes.data, p[2].ctypes.data if len(p) > 2 else None, p[0].shape[1], p[0].shape[0],
                                      p[0].strides[0], p[1].strides[0], lay, 0))
            elif isinstance(f, np.ndarray) and f.ndim == 3:
                for a in f:
                    stacked(a)
            elif isinstance(f, np.ndarray):
                stacked(f)
            else:
                raise ValueError("a frame must be YuvFrames, a stacked (h * 3 // 2, w) uint8 array or a tuple of planes")
        arr = (_YuvImage * max(len(imgs), 1))(*imgs)
        return arr, len(imgs), keep

    @staticmethod
    def _yuv_params(channels: int, rgb: bool) -> "YuvParams":
        p = YuvParams()
        load_library().vj_yuv_default(C.byref(p))
        p.channels = int(channels)
        p.flags = VJ_YUV_RGB_ORDER if rgb else 0
        return p

    @staticmethod
    def _out_tensor(out, nbytes: int, device: int):
        import torch
        if out is None:
            out = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=torch.device("cuda", device))
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous torch.uint8 tensor in device memory")
        return out

    @staticmethod
    def yuv_to_bgr_layout(frames, alpha: bool = False, rgb: bool = False, layout="nv12"):
        """vj_yuv_to_bgr_layout (host only): where yuv_to_bgr() puts every image -> ([(offset, width, height, stride)], bytes)."""
        imgs, n, keep = Environment._yuv_images(frames, layout)
        p = Environment._yuv_params(4 if alpha else 3, rgb)
        out = (_Image * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(load_library().vj_yuv_to_bgr_layout(imgs, n, C.byref(p), out, C.byref(nbytes)), "vj_yuv_to_bgr_layout")
        return [(int(out[i].data or 0), out[i].width, out[i].height, out[i].stride) for i in range(n)], int(nbytes.value)

    def yuv_to_bgr(self, frames, alpha: bool = False, rgb: bool = False, out=None, layout="nv12") -> list:
        """vj_yuv_to_bgr: a decoder's NV12 / NV21 / I420 frames to interleaved BGR (alpha=True: BGRA with alpha 255; rgb=True: RGB /
        RGBA) on the device, OpenCV's 8-bit BT.601 limited-range arithmetic with nearest chroma.  frames: see
        _yuv_images; layout names the layout of host arrays.  Returns what preprocess() returns: ONE DeviceFrames of n frames
        when the sizes agree — extract(), extract_affine() and paint() take it as it is —, else one per frame.  out: as preprocess()."""
        imgs, n, keep = self._yuv_images(frames, layout)
        p = self._yuv_params(4 if alpha else 3, rgb)
        lib = load_library()
        res = (_Image * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(lib.vj_yuv_to_bgr_layout(imgs, n, C.byref(p), res, C.byref(nbytes)), "vj_yuv_to_bgr_layout")
        out = self._out_tensor(out, nbytes.value, self._device)
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_yuv_to_bgr(self._h, imgs, n, C.byref(p), C.c_void_p(out.data_ptr()), out.numel(), res), "vj_yuv_to_bgr")
        if n == 0:
            return []
        ch = p.channels
        r = [DeviceFrames(int(res[i].data), 1, res[i].height, res[i].width, res[i].stride, ch, 0, out) for i in range(n)]
        if all((f.width, f.height) == (r[0].width, r[0].height) for f in r):
            return [DeviceFrames(r[0].ptr, n, r[0].height, r[0].width, r[0].stride, ch, (r[1].ptr - r[0].ptr) if n > 1 else 0, out)]
        return r

    @staticmethod
    def _bgr_images(frames):
        if isinstance(frames, (np.ndarray, DeviceFrames)):
            return Environment._images(frames, True)
        return Environment._mixed_images(frames)

    @staticmethod
    def bgr_to_yuv_layout(frames, layout="nv12", rgb: bool = False):
        """vj_bgr_to_yuv_layout (host only): where bgr_to_yuv() puts every frame ->
        ([(y offset, c0 offset, c1 offset, width, height, y_stride, c_stride)], bytes)."""
        imgs, n, keep = Environment._bgr_images(frames)
        p = Environment._yuv_params(3, rgb)
        out = (_YuvImage * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(load_library().vj_bgr_to_yuv_layout(imgs, n, C.byref(p), Environment._yuv_layout_id(layout), out, C.byref(nbytes)), "vj_bgr_to_yuv_layout")
        return [(int(o.y or 0), int(o.c0 or 0), int(o.c1 or 0), o.width, o.height, o.y_stride, o.c_stride) for o in out[:n]], int(nbytes.value)

    def bgr_to_yuv(self, frames, layout="nv12", rgb: bool = False, out=None):
        """vj_bgr_to_yuv: BGR / BGRA frames (rgb=True: RGB / RGBA; alpha is ignored) to NV12 / NV21 / I420 on the device — what an
        encoder takes —, OpenCV's 8-bit BT.601 limited-range arithmetic, chroma from the top-left pixel of each 2 x 2 block
        (DESIGN.md §4.21).  frames: DeviceFrames, e.g. what yuv_to_bgr() returned and paint() changed; an (n, h, w, 3 | 4) array; or a
        list as detect_mixed() takes it.  Every output frame is stacked: the Y plane at a pitch of the width rounded up to 4, the
        chroma below it.  Returns ONE YuvFrames of n frames when the sizes agree, else a list of one per frame.  out: as preprocess()."""
        lay = self._yuv_layout_id(layout)
        imgs, n, keep = self._bgr_images(frames)
        p = self._yuv_params(3, rgb)
        lib = load_library()
        res = (_YuvImage * max(n, 1))()
        nbytes = C.c_uint64(0)
        _check(lib.vj_bgr_to_yuv_layout(imgs, n, C.byref(p), lay, res, C.byref(nbytes)), "vj_bgr_to_yuv_layout")
        out = self._out_tensor(out, nbytes.value, self._device)
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_bgr_to_yuv(self._h, imgs, n, C.byref(p), lay, C.c_void_p(out.data_ptr()), out.numel(), res), "vj_bgr_to_yuv")
        if n == 0:
            return []
        r = [YuvFrames(int(o.y), int(o.c0), int(o.c1 or 0), 1, o.height, o.width, o.y_stride, o.c_stride, lay, 0, out) for o in res[:n]]
        if all((f.width, f.height) == (r[0].width, r[0].height) for f in r):
            return YuvFrames(r[0].ptr_y, r[0].ptr_c0, r[0].ptr_c1, n, r[0].height, r[0].width, r[0].y_stride, r[0].c_stride, lay,
                             (r[1].ptr_y - r[0].ptr_y) if n > 1 else 0, out)
        return r

    def yuv_timing(self) -> float:
        """vj_yuv_timing: device time of the last yuv_to_bgr() or bgr_to_yuv() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_yuv_timing(self._h, C.byref(ms)), "vj_yuv_timing")
        return float(ms.value)

    @staticmethod
    def _affine_args(frames, affines, size, gray, planar, color):
        """-> (ctypes array of vj_image, n, arrays to keep alive, AFFINE_DTYPE array, vj_affine_params).  frames: as preprocess().
        affines: an AFFINE_DTYPE array or (n, 7) float64 rows of (frame, m0 .. m5)."""
        if color or isinstance(frames, (np.ndarray, DeviceFrames)):
            imgs, n, keep = Environment._images(frames, color)
        else:
            imgs, n, keep = Environment._mixed_images(frames)
        if isinstance(affines, np.ndarray) and affines.dtype.names is not None:
            a = np.ascontiguousarray(affines, AFFINE_DTYPE).reshape(-1)
        else:
            rows = np.asarray(affines, np.float64).reshape(-1, 7)
            if rows.size and not (np.isfinite(rows[:, 0]).all() and (rows[:, 0] == np.floor(rows[:, 0])).all() and (np.abs(rows[:, 0]) < 2**31).all()):
                raise ValueError("the first column of affines is the frame index: an integer")
            a = np.zeros(len(rows), AFFINE_DTYPE)
            a["frame"] = rows[:, 0].astype(np.int32)
            a["m"] = rows[:, 1:]
        p = AffineParams()
        load_library().vj_affine_default(C.byref(p))
        p.out_w, p.out_h = int(size[0]), int(size[1])
        p.flags = (VJ_EXTRACT_GRAY if gray else 0) | (VJ_EXTRACT_PLANAR if planar else 0)
        return imgs, n, keep, a, p

    @staticmethod
    def extract_affine_layout(frames, affines, size, gray: bool = False, planar: bool = False, color: bool = False):
        """vj_extract_affine_layout (host only): what extract_affine() will write -> (channels of the output, bytes of the output)."""
        imgs, n, keep, a, p = Environment._affine_args(frames, affines, size, gray, planar, color)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(load_library().vj_extract_affine_layout(imgs, n, a.ctypes.data, len(a), C.byref(p), C.byref(ch), C.byref(nbytes)),
               "vj_extract_affine_layout")
        return int(ch.value), int(nbytes.value)

    def extract_affine(self, frames, affines, size, gray: bool = False, planar: bool = False, color: bool = False, out=None):
        """vj_extract_affine: one affine warp per region, all to one fixed size, on the device — aligned crops for a
        recognition network (align_transforms), or whole frames rotated (one affine per frame, size = the frame's).  Row
        (frame, m0 .. m5) maps OUTPUT pixel (x, y) to the source pixel (m0 x + m1 y + m2, m3 x + m4 y + m5) of that frame, pixel
        coordinates used directly (no half-pixel offset: a scaling matrix is not extract()'s resize; affine_from_rect adds the offset
        that aligns pixel centres); the four neighbours are blended with 1/32-pixel weights, the frame's border replicated (never
        clipped).  gray=True: one channel, the taps through BGR2GRAY first.  frames: as extract().  affines: (n, 7) float64 rows or
        an AFFINE_DTYPE array.  Returns a torch.uint8 device tensor of shape (n, h, w, C), or (n, C, h, w) with planar=True.  out: a
        contiguous torch.uint8 tensor on this device with that many elements; None: one is allocated."""
        import torch
        imgs, n, keep, a, p = self._affine_args(frames, affines, size, gray, planar, color)
        lib = load_library()
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(lib.vj_extract_affine_layout(imgs, n, a.ctypes.data, len(a), C.byref(p), C.byref(ch), C.byref(nbytes)), "vj_extract_affine_layout")
        shape = (len(a), ch.value, p.out_h, p.out_w) if planar else (len(a), p.out_h, p.out_w, ch.value)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self._device))
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous torch.uint8 tensor in device memory")
        if out.numel() != int(nbytes.value):
            raise ValueError(f"out must hold {int(nbytes.value)} bytes, the shape {shape}; it holds {out.numel()}")
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_extract_affine(self._h, imgs, n, a.ctypes.data, len(a), C.byref(p), C.c_void_p(out.data_ptr()), out.numel()),
               "vj_extract_affine")
        return out.view(shape)

    def extract_affine_timing(self) -> float:
        """vj_extract_affine_timing: device time of the last extract_affine() call (events around its copies and launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_extract_affine_timing(self._h, C.byref(ms)), "vj_extract_affine_timing")
        return float(ms.value)

    @staticmethod
    def _extract_yuv_args(frames, rects, size, scale, margin, gray, planar, alpha, rgb, layout):
        """-> (ctypes array of vj_yuv_image, n, arrays to keep alive, (n, 5) int32 regions, vj_extract_params, vj_yuv_params).
        frames: as yuv_to_bgr(); rects: as extract(), in luma pixels."""
        imgs, n, keep = Environment._yuv_images(frames, layout)
        _, _, _, r, p = Environment._extract_args(np.zeros((0, 1, 1), np.uint8), rects, size, scale, margin, gray, planar, False)
        return imgs, n, keep, r, p, Environment._yuv_params(4 if alpha else 3, rgb)

    @staticmethod
    def extract_yuv_layout(frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False,
                           alpha: bool = False, rgb: bool = False, layout="nv12"):
        """vj_extract_yuv_layout (host only): what extract_yuv() will cut -> ((n, 5) int32 rows of the mapped source regions
        (frame, x, y, w, h) in luma pixels, which may lie outside their frames; channels of the output; bytes of the output)."""
        imgs, n, keep, r, p, yp = Environment._extract_yuv_args(frames, rects, size, scale, margin, gray, planar, alpha, rgb, layout)
        src = np.zeros((len(r), 5), np.int32)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(load_library().vj_extract_yuv_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), C.byref(yp), src.ctypes.data, C.byref(ch),
                                                    C.byref(nbytes)), "vj_extract_yuv_layout")
        return src, int(ch.value), int(nbytes.value)

    def _crops_out(self, out, n, ch, p, planar, nbytes):
        """The destination tensor of extract_yuv() / extract_affine_yuv(), as extract()'s -> (tensor, shape)."""
        import torch
        shape = (n, ch, p.out_h, p.out_w) if planar else (n, p.out_h, p.out_w, ch)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self._device))
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()):
            raise ValueError("out must be a contiguous torch.uint8 tensor in device memory")
        if out.numel() != int(nbytes):
            raise ValueError(f"out must hold {int(nbytes)} bytes, the shape {shape}; it holds {out.numel()}")
        return out, shape

    def extract_yuv(self, frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False,
                    alpha: bool = False, rgb: bool = False, out=None, layout="nv12"):
        """vj_extract_yuv: extract() of yuv_to_bgr(frames, alpha, rgb), byte for byte, without the BGR copy of the frames (DESIGN.md
        §4.25): every tap is decoded from the 4:2:0 planes where they lie (nearest chroma, BT.601 limited range), then resized per
        channel.  frames: as yuv_to_bgr() — YuvFrames, stacked host arrays, tuples of planes or a list of these; layout names the
        layout of host arrays.  rects, size, scale, margin, planar: as extract(), the rectangles in luma pixels.  alpha=True: four
        channels, alpha 255; rgb=True: RGB order; gray=True: one channel, BGR2GRAY of every decoded tap (crops of the Y plane itself
        are extract(yuv.luma(), ...), which differ in range).  Returns a torch.uint8 device tensor (n, h, w, C), or (n, C, h, w) with
        planar=True.  out: as extract()."""
        imgs, n, keep, r, p, yp = self._extract_yuv_args(frames, rects, size, scale, margin, gray, planar, alpha, rgb, layout)
        lib = load_library()
        src = np.zeros((len(r), 5), np.int32)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(lib.vj_extract_yuv_layout(imgs, n, r.ctypes.data, len(r), C.byref(p), C.byref(yp), src.ctypes.data, C.byref(ch), C.byref(nbytes)),
               "vj_extract_yuv_layout")
        out, shape = self._crops_out(out, len(r), ch.value, p, planar, nbytes.value)
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_extract_yuv(self._h, imgs, n, r.ctypes.data, len(r), C.byref(p), C.byref(yp), C.c_void_p(out.data_ptr()), out.numel()),
               "vj_extract_yuv")
        return out.view(shape)

    @staticmethod
    def _affine_yuv_args(frames, affines, size, gray, planar, alpha, rgb, layout):
        """-> (ctypes array of vj_yuv_image, n, arrays to keep alive, AFFINE_DTYPE array, vj_affine_params, vj_yuv_params)."""
        imgs, n, keep = Environment._yuv_images(frames, layout)
        _, _, _, a, p = Environment._affine_args(np.zeros((0, 1, 1), np.uint8), affines, size, gray, planar, False)
        return imgs, n, keep, a, p, Environment._yuv_params(4 if alpha else 3, rgb)

    @staticmethod
    def extract_affine_yuv_layout(frames, affines, size, gray: bool = False, planar: bool = False, alpha: bool = False, rgb: bool = False,
                                  layout="nv12"):
        """vj_extract_affine_yuv_layout (host only): what extract_affine_yuv() will write -> (channels, bytes of the output)."""
        imgs, n, keep, a, p, yp = Environment._affine_yuv_args(frames, affines, size, gray, planar, alpha, rgb, layout)
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(load_library().vj_extract_affine_yuv_layout(imgs, n, a.ctypes.data, len(a), C.byref(p), C.byref(yp), C.byref(ch), C.byref(nbytes)),
               "vj_extract_affine_yuv_layout")
        return int(ch.value), int(nbytes.value)

    def extract_affine_yuv(self, frames, affines, size, gray: bool = False, planar: bool = False, alpha: bool = False, rgb: bool = False,
                           out=None, layout="nv12"):
        """vj_extract_affine_yuv: extract_affine() of yuv_to_bgr(frames, alpha, rgb), byte for byte, without the BGR copy (DESIGN.md
        §4.25): the four taps of every output pixel are decoded from the 4:2:0 planes, then blended per channel.  frames, alpha, rgb,
        gray, layout: as extract_yuv(); affines, size, planar, out and the result: as extract_affine(), source coordinates in luma
        pixels (align_transforms' rows fit as they are)."""
        imgs, n, keep, a, p, yp = self._affine_yuv_args(frames, affines, size, gray, planar, alpha, rgb, layout)
        lib = load_library()
        ch, nbytes = C.c_int(0), C.c_uint64(0)
        _check(lib.vj_extract_affine_yuv_layout(imgs, n, a.ctypes.data, len(a), C.byref(p), C.byref(yp), C.byref(ch), C.byref(nbytes)),
               "vj_extract_affine_yuv_layout")
        out, shape = self._crops_out(out, len(a), ch.value, p, planar, nbytes.value)
        _order_after_torch(self._device)       # after the allocation, as in preprocess()
        _check(lib.vj_extract_affine_yuv(self._h, imgs, n, a.ctypes.data, len(a), C.byref(p), C.byref(yp), C.c_void_p(out.data_ptr()),
                                         out.numel()), "vj_extract_affine_yuv")
        return out.view(shape)

    def extract_yuv_timing(self) -> float:
        """vj_extract_yuv_timing: device time of the last extract_yuv() or extract_affine_yuv() call (events around its copies and
        launches), ms."""
        ms = C.c_float(0)
        _check(load_library().vj_extract_yuv_timing(self._h, C.byref(ms)), "vj_extract_yuv_timing")
        return float(ms.value)

    def mixed_info(self) -> MixedInfo:
        """vj_mixed_info_get: atlases (count and the largest one's size), batched calls on original frames, frames by route, grid
        positions of the atlas passes and the pack launches' device time of the last detect_mixed / detect_opencv_mixed call."""
        info = MixedInfo()
        _check(load_library().vj_mixed_info_get(self._h, C.byref(info)), "vj_mixed_info_get")
        return info

    def detect(self, cascade: Cascade, frames, params: Params | None = None, color: bool = False) -> DetectResult:
        """frames: 2-D uint8 array, 3-D (n, h, w) array, list of 2-D arrays, or
        DeviceFrames (frames already resident in HBM).  color=True: every frame is (h, w, 3 | 4) BGR / BGRA
        (one 3-D array, a 4-D batch or a list) and is converted to gray on the device."""
        p = params or default_params()
        imgs, n, keep = self._images(frames, color, self._device)
        res = _Result()
        lib = load_library()
        _check(lib.vj_detect(self._h, cascade._h, imgs, n, C.byref(p), C.byref(res)), "vj_detect")
        return self._result(lib, res, cascade)

    @staticmethod
    def _result(lib, res, cascade) -> DetectResult:
        try:
            if res.count:
                buf = (C.c_char * (RECT_DTYPE.itemsize * res.count)).from_address(res.rects)
                rects = np.frombuffer(buf, RECT_DTYPE, res.count).copy()
            else:
                rects = np.zeros(0, RECT_DTYPE)
            k, t = res.counters, res.timing
            return DetectResult(rects, int(k.windows), int(k.stump_evals), int(k.gather_bytes),
                                [int(v) for v in k.stage_entered[:cascade.info.n_stages]],
                                float(t.integral_ms), float(t.cascade_ms), float(t.total_ms),
                                int(t.n_cascade_launches),
                                [(int(t.pass_stage_begin[i]), int(t.pass_stage_end[i]), float(t.pass_ms[i]))
                                 for i in range(min(int(t.n_cascade_launches), VJ_MAX_PASSES))],
                                [dict(kind=LAUNCH_KINDS.get(int(l.kind), "?"), lds_class=int(l.lds_class),
                                      stage_begin=int(l.stage_begin), stage_end=int(l.stage_end), ms=float(l.ms),
                                      lds_bytes=int(l.lds_bytes),
                                      scales=[k for k in range(127) if (l.scale_mask[k >> 6] >> (k & 63)) & 1],
                                      stage_entered=[int(v) for v in l.stage_entered[:cascade.info.n_stages]])
                                 for l in list(t.launch)[:int(t.n_launches)]], float(t.tile_split),
                                int(t.balance_state), int(t.balance_calls))
        finally:
            lib.vj_result_free(C.byref(res))

    def close(self):
        if self._h:
            load_library().vj_env_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrameStream:
    """vj_stream: double-buffered upload of host frame batches overlapped with the previous batch's kernels."""

    def __init__(self, env: Environment, cascade: Cascade, width: int, height: int, max_batch: int, params: Params, channels: int = 1):
        self._env, self._cascade = env, cascade
        h = C.c_void_p()
        _check(load_library().vj_stream_create(env._h, cascade._h, width, height, channels, max_batch, C.byref(params), C.byref(h)),
               "vj_stream_create")
        self._h = h
        self._keep = []

    def submit(self, frames, color: bool = False):
        imgs, n, keep = Environment._images(frames, color, self._env._device)
        _check(load_library().vj_stream_submit(self._h, imgs, n), "vj_stream_submit")
        self._keep.append((imgs, keep))

    def collect(self) -> DetectResult:
        res = _Result()
        lib = load_library()
        _check(lib.vj_stream_collect(self._h, C.byref(res)), "vj_stream_collect")
        if self._keep:
            self._keep.pop(0)
        return Environment._result(lib, res, self._cascade)

    def close(self):
        if self._h:
            load_library().vj_stream_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class DeviceFrames:
    """A batch of equal-size 8-bit frames already resident in device memory
    (e.g. a torch.uint8 CUDA tensor's data_ptr()); rows `stride` bytes apart,
    frames `frame_bytes` bytes apart (0: stride * height); channels = 1 (gray), 3 (BGR) or 4 (BGRA), interleaved.
    owner: whatever keeps the memory alive (Environment.preprocess puts its tensor there).
    Every call that is given one first waits for torch's current stream on the environment's device (_order_after_torch), so work
    queued there — a copy_, a decoder's kernels — has written the frames; producers on other streams are the caller's to wait for."""
    ptr: int
    n: int
    height: int
    width: int
    stride: int
    channels: int = 1
    frame_bytes: int = 0
    owner: object = None

    def frame_ptr(self, i: int) -> int:
        return self.ptr + i * (self.frame_bytes or self.stride * self.height)

    @classmethod
    def from_torch(cls, t) -> "DeviceFrames":
        """(n, h, w) gray or (n, h, w, 3 | 4) BGR / BGRA uint8 CUDA tensor."""
        assert t.is_cuda and t.dtype.itemsize == 1 and t.dim() in (3, 4) and t.is_contiguous()
        if t.dim() == 4:
            n, h, w, ch = t.shape
            assert ch in (3, 4)
            return cls(t.data_ptr(), n, h, w, w * ch, ch)
        n, h, w = t.shape
        return cls(t.data_ptr(), n, h, w, w)


@dataclass
class YuvFrames:
    """A batch of equal-size 4:2:0 frames resident in device memory, as a hardware decoder writes them and an encoder reads them.
    layout: VJ_YUV_NV12 / VJ_YUV_NV21 (ptr_c0: the plane of U, V / V, U byte pairs; ptr_c1 = 0) or VJ_YUV_I420 (ptr_c0, ptr_c1: the
    U and V planes).  Rows of the Y plane are y_stride bytes apart, rows of the chroma planes c_stride; frame i's planes lie
    i * frame_bytes behind frame 0's (planes that are allocated apart have no default for it: with n > 1 it must be given).  owner:
    whatever keeps the memory alive.  Ordered after torch's current stream like DeviceFrames."""
    ptr_y: int
    ptr_c0: int
    ptr_c1: int
    n: int
    height: int
    width: int
    y_stride: int
    c_stride: int
    layout: int = VJ_YUV_NV12
    frame_bytes: int = 0
    owner: object = None

    def __post_init__(self):
        if self.n > 1 and not self.frame_bytes:
            raise ValueError("YuvFrames of more than one frame need frame_bytes")

    @classmethod
    def from_torch(cls, t, layout="nv12") -> "YuvFrames":
        """(n, h * 3 // 2, w) uint8 CUDA tensor of stacked frames: the Y plane, the chroma below it (I420: the U plane, then the V
        plane, w / 2 * h / 2 bytes each)."""
        assert t.is_cuda and t.dtype.itemsize == 1 and t.dim() == 3 and t.is_contiguous() and t.shape[1] % 3 == 0
        lay = Environment._yuv_layout_id(layout)
        n, rows, w = t.shape
        h = rows * 2 // 3
        y = t.data_ptr()
        if lay == VJ_YUV_I420:
            return cls(y, y + w * h, y + w * h + (w // 2) * (h // 2), n, h, w, w, w // 2, lay, rows * w, t)
        return cls(y, y + w * h, 0, n, h, w, w, w, lay, rows * w, t)

    def luma(self) -> "DeviceFrames":
        """vj_yuv_luma: the Y planes as gray frames (COLOR_YUV2GRAY_NV12) — what preprocess() and every detect call take."""
        return DeviceFrames(self.ptr_y, self.n, self.height, self.width, self.y_stride, 1, self.frame_bytes, self.owner)


def yuv_to_bgr_layout(frames, alpha: bool = False, rgb: bool = False, layout="nv12"):
    """vj_yuv_to_bgr_layout: the host-only twin of Environment.yuv_to_bgr (no environment, no device) ->
    ([(offset, width, height, stride) per frame], bytes of the destination buffer)."""
    return Environment.yuv_to_bgr_layout(frames, alpha, rgb, layout)


def bgr_to_yuv_layout(frames, layout="nv12", rgb: bool = False):
    """vj_bgr_to_yuv_layout: the host-only twin of Environment.bgr_to_yuv ->
    ([(y offset, c0 offset, c1 offset, width, height, y_stride, c_stride) per frame], bytes of the destination buffer)."""
    return Environment.bgr_to_yuv_layout(frames, layout, rgb)


def preprocess_layout(frames, size=None, fx=None, fy=None, equalize: bool = False, color: bool = False):
    """vj_preprocess_layout: the host-only twin of Environment.preprocess (no environment, no device) ->
    ([(offset, width, height, stride) per frame], bytes of the destination buffer)."""
    return Environment.preprocess_layout(frames, size, fx, fy, equalize, color)


def extract_layout(frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False, color: bool = False):
    """vj_extract_layout: the host-only twin of Environment.extract (no environment, no device) ->
    (mapped source regions as (n, 5) int32 rows, channels, bytes)."""
    return Environment.extract_layout(frames, rects, size, scale, margin, gray, planar, color)


def paint_layout(frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
                 ellipse: bool = False, color: bool = False):
    """vj_paint_layout: the host-only twin of Environment.paint (no environment, no device) ->
    (clipped rectangles as (n, 5) int32 rows, sizes as (n,) int32, scratch bytes)."""
    return Environment.paint_layout(frames, rects, mode, size, rel, scale, margin, ellipse, color)


def paint_yuv_layout(frames, rects, mode="blur", size: int = 0, rel: float = 0.25, scale=(1.0, 1.0), margin: float = 0.0,
                     ellipse: bool = False, layout="nv12"):
    """vj_paint_yuv_layout: the host-only twin of Environment.paint_yuv (no environment, no device) ->
    (K rows, Kc rows, luma sizes, chroma sizes, scratch bytes)."""
    return Environment.paint_yuv_layout(frames, rects, mode, size, rel, scale, margin, ellipse, layout)


def extract_yuv_layout(frames, rects, size, scale=(1.0, 1.0), margin: float = 0.0, gray: bool = False, planar: bool = False,
                       alpha: bool = False, rgb: bool = False, layout="nv12"):
    """vj_extract_yuv_layout: the host-only twin of Environment.extract_yuv (no environment, no device) ->
    (mapped source regions in luma pixels, channels, bytes)."""
    return Environment.extract_yuv_layout(frames, rects, size, scale, margin, gray, planar, alpha, rgb, layout)


def extract_affine_yuv_layout(frames, affines, size, gray: bool = False, planar: bool = False, alpha: bool = False, rgb: bool = False,
                              layout="nv12"):
    """vj_extract_affine_yuv_layout: the host-only twin of Environment.extract_affine_yuv -> (channels, bytes)."""
    return Environment.extract_affine_yuv_layout(frames, affines, size, gray, planar, alpha, rgb, layout)


def track_layout(frames, rows, tmpl: int = 32, radius: int = 8, scale=(1.0, 1.0), color: bool = False):
    """vj_track_layout: the host-only twin of Environment.track (no environment, no device) ->
    (template regions as (n, 5) int32 rows, search regions as (n, 5) int32 rows, scratch bytes)."""
    return Environment.track_layout(frames, rows, tmpl, radius, scale, color)


def _box_iou(a, b) -> float:
    """Intersection over union of two (x, y, w, h) boxes."""
    iw = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
    ih = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = float(iw) * float(ih)
    return inter / (float(a[2]) * float(a[3]) + float(b[2]) * float(b[3]) - inter)


def bridge_detections(env, frames, rects, max_age: int = 2, iou: float = 0.3, max_mad: float = 12.0, tmpl: int = 32, radius: int = 8,
                      scale=(1.0, 1.0), color: bool = False, track=None):
    """Fills the gaps a detector leaves in a video with Environment.track: host bookkeeping around at most 2 * max_age device calls.
    frames: consecutive frames in index order, as track() takes them; rects: the detections of all frames, a RECT_DTYPE array or
    integer rows of (frame, x, y, w, h), in the detector's coordinates — scale = (sx, sy) takes them to the frames' pixels, as in
    extract() and paint().

    Forward round a = 1 .. max_age: every box of age a - 1 (age 0: a detected box) in a frame f that is not the last, for which no box
    of frame f + 1 — detected or carried — has an intersection over union of at least `iou`, becomes a row f -> f + 1; all rows of a
    round are ONE track call.  A row is accepted when its sad <= max_mad * tmpl^2 (a mean absolute difference of max_mad gray
    levels); its result box then joins frame f + 1 with age a.  The backward rounds do the same towards f - 1 with ages -1 ..
    -max_age; they are seeded by detected boxes only, and the boxes of the forward pass count as present.  A round without rows ends
    its pass.  max_mad is the caller's knob: its default of 12 gray levels is a guess that nobody has measured on real video.

    Returns (rects, age): (n, 5) int32 rows of (frame, x, y, w, h) in the input's coordinates — the input's rows in their order, then
    the carried boxes in the order they were found, each the result box divided by scale and rounded half to even (cvRound) — and
    the (n,) int32 ages.  track: a callable with Environment.track's signature, default env.track."""
    if isinstance(rects, np.ndarray) and rects.dtype.names is not None:
        r = np.stack([np.asarray(rects[k], np.int32).reshape(-1) for k in ("frame", "x", "y", "w", "h")], axis=1)
    else:
        r = np.asarray(rects)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("rects must be a RECT_DTYPE array or integer rows of (frame, x, y, w, h)")
        r = r.astype(np.int32).reshape(-1, 5)
    if track is None:
        track = env.track
    n_frames = Environment._paint_images(frames, color, write=False)[1]       # as track() counts them: a DeviceFrames holds .n frames
    sx, sy = (float(v) or 1.0 for v in scale)
    boxes = [tuple(int(v) for v in row) for row in r]
    ages = [0] * len(boxes)
    limit = float(max_mad) * int(tmpl) * int(tmpl)
    for step in (1, -1):
        for a in range(1, int(max_age) + 1):
            seeds = [b for b, g in zip(boxes, ages) if g == step * (a - 1) and 0 <= b[0] + step < n_frames]
            rows = [(b[0], b[0] + step) + b[1:] for b in seeds
                    if not any(o[0] == b[0] + step and _box_iou(b[1:], o[1:]) >= iou for o in boxes)]
            if not rows:
                break
            res = track(frames, np.asarray(rows, np.int32).reshape(-1, 6), tmpl=tmpl, radius=radius, scale=scale, color=color)
            for row, m in zip(rows, res):
                if float(m["sad"]) <= limit:
                    boxes.append((row[1], int(np.rint(float(m["x"]) / sx)), int(np.rint(float(m["y"]) / sy)),
                                  max(int(np.rint(float(m["w"]) / sx)), 1), max(int(np.rint(float(m["h"]) / sy)), 1)))
                    ages.append(step * a)
    return np.asarray(boxes, np.int32).reshape(-1, 5), np.asarray(ages, np.int32)


def extract_affine_layout(frames, affines, size, gray: bool = False, planar: bool = False, color: bool = False):
    """vj_extract_affine_layout: the host-only twin of Environment.extract_affine (no environment, no device) -> (channels, bytes)."""
    return Environment.extract_affine_layout(frames, affines, size, gray, planar, color)


def affine_from_rect(x: float, y: float, w: float, h: float, size) -> np.ndarray:
    """vj_affine_from_rect (host only): the matrix (6 float64) that scales the box (x, y, w, h) to size = (out_w, out_h) with pixel
    centres aligned: {w / out_w, 0, x + 0.5 w / out_w - 0.5, 0, h / out_h, y + 0.5 h / out_h - 0.5}."""
    m = (C.c_double * 6)()
    _check(load_library().vj_affine_from_rect(float(x), float(y), float(w), float(h), int(size[0]), int(size[1]), m), "vj_affine_from_rect")
    return np.array(m[:], np.float64)


def affine_from_eyes(lx: float, ly: float, rx: float, ry: float, size, eye_pos=(0.3, 0.7, 0.35)) -> np.ndarray:
    """vj_affine_from_eyes (host only): the similarity (6 float64) that puts the left eye (lx, ly) at output pixel
    (ex_l out_w, ey out_h) and the right eye (rx, ry) at (ex_r out_w, ey out_h); eye_pos = (ex_l, ex_r, ey)."""
    m = (C.c_double * 6)()
    _check(load_library().vj_affine_from_eyes(float(lx), float(ly), float(rx), float(ry), int(size[0]), int(size[1]), float(eye_pos[0]),
                                              float(eye_pos[1]), float(eye_pos[2]), m), "vj_affine_from_eyes")
    return np.array(m[:], np.float64)


def align_transforms(faces, eyes, size, eye_pos=(0.3, 0.7, 0.35), scale=(1.0, 1.0)):
    """The matrices that cut every face of a two-cascade call aligned by its eyes -> (affines, paired): an AFFINE_DTYPE array with
    one row per face, for Environment.extract_affine, and a bool array.  faces, eyes: the two results of detect_opencv_chain or
    detect_chain (or their RECT_DTYPE arrays): eyes' `frame` indexes faces' rectangles and its x, y are relative to that region.
    scale = (sx, sy) takes detector coordinates to the pixels of the frames the crops are cut from.

    The pairing rule, for face k = (x, y, w, h): the candidates are the second-cascade rectangles with frame == k whose centre
    (e.x + e.w / 2, e.y + e.h / 2) has its y below h / 2 (the upper half of the face).  The left eye is the candidate with centre x
    below w / 2 and the greatest weight, the right eye likewise among those with centre x at or above w / 2; ties go to the lowest
    index.  An eye's centre in the frame is (x + e.x + e.w / 2) * sx, (y + e.y + e.h / 2) * sy in f64, not rounded.  A face with both
    eyes gets affine_from_eyes(left, right, size, eye_pos) and paired[k] = True; any other face gets affine_from_rect of its box times
    scale and paired[k] = False — so every face has a crop."""
    fr = np.asarray(getattr(faces, "rects", faces))
    er = np.asarray(getattr(eyes, "rects", eyes))
    sx, sy = float(scale[0]), float(scale[1])
    out = np.zeros(len(fr), AFFINE_DTYPE)
    paired = np.zeros(len(fr), bool)
    for k, f in enumerate(fr):
        x, y, w, h = (float(f[n]) for n in ("x", "y", "w", "h"))
        best = [None, None]                                            # (weight, centre x, centre y) of the left and the right eye
        for e in er[er["frame"] == k] if len(er) else ():
            cx, cy = float(e["x"]) + float(e["w"]) / 2, float(e["y"]) + float(e["h"]) / 2
            if not cy < h / 2:
                continue
            side = 0 if cx < w / 2 else 1
            if best[side] is None or float(e["weight"]) > best[side][0]:
                best[side] = (float(e["weight"]), cx, cy)
        out["frame"][k] = int(f["frame"])
        if best[0] is not None and best[1] is not None:
            out["m"][k] = affine_from_eyes((x + best[0][1]) * sx, (y + best[0][2]) * sy, (x + best[1][1]) * sx, (y + best[1][2]) * sy, size, eye_pos)
            paired[k] = True
        else:
            out["m"][k] = affine_from_rect(x * sx, y * sy, w * sx, h * sy, size)
    return out, paired


def _pixel_contiguous(img: np.ndarray) -> np.ndarray:
    """(h, w, c) view whose pixels and channels are contiguous (rows may be strided: ROI views stay views)."""
    c = img.shape[2]
    return img if img.strides[2] == 1 and img.strides[1] == c else np.ascontiguousarray(img)


def group_rectangles(rects: np.ndarray, group_threshold: int, eps: float = 0.2) -> np.ndarray:
    """filterResult / cv::groupRectangles on a RECT_DTYPE array sorted by frame (host logic)."""
    buf = np.ascontiguousarray(rects, RECT_DTYPE).copy()
    n = C.c_uint32(len(buf))
    _check(load_library().vj_group_rectangles(buf.ctypes.data if len(buf) else None, C.byref(n), int(group_threshold),
                                              float(eps)), "vj_group_rectangles")
    return buf[:n.value]


def group_rectangles_levels(rects: np.ndarray, levels, weights, group_threshold: int, eps: float = 0.2):
    """groupRectangles(rectList, rejectLevels, levelWeights, groupThreshold, eps) (tempcv.cpp:255-258) on a RECT_DTYPE array sorted
    by frame with its reject levels and level weights (host logic).  Returns (rects, levels, weights) of the kept classes."""
    buf = np.ascontiguousarray(rects, RECT_DTYPE).copy()
    lv = np.ascontiguousarray(levels, np.int32).copy()
    lw = np.ascontiguousarray(weights, np.float64).copy()
    if not (len(buf) == len(lv) == len(lw)):
        raise VjError(1, "group_rectangles_levels", "rects, levels and weights must have one length")
    n = load_library().vj_group_rectangles_levels(buf.ctypes.data if len(buf) else None, lv.ctypes.data if len(buf) else None,
                                                  lw.ctypes.data if len(buf) else None, len(buf), int(group_threshold), float(eps))
    if n < 0:
        _check(-n, "vj_group_rectangles_levels")
    return buf[:n], lv[:n], lw[:n]


# ------------------------------------------------- reference-named entry points
def clodInitEnvironment(device_index: int = 0) -> Environment:
    """clod.h:61-62 / clod.cpp:72-100."""
    return Environment(device_index)


def clodInitBuffers(env: Environment, image_size, batch: int = 1):
    """clod.h:67-69 / clod.cpp:102-163; image_size = (width, height) like CvSize."""
    env.reserve(int(image_size[0]), int(image_size[1]), batch)


def clodReleaseBuffers(env: Environment):
    """clod.h:70-71: buffers are owned by the environment here; nothing to do."""


def clodReleaseEnvironment(env: Environment):
    """clod.h:64-65 / clod.cpp:173-180."""
    env.close()


def clifIntegral(source: np.ndarray, env: Environment, use_opencl: bool = True):
    """clif.h:63-66 / clif.cpp:273-316: returns (sum CV_32S-as-uint32, square_sum as
    uint64), both (h+1, w+1) — cvIntegral's layout."""
    if not use_opencl:
        raise VjError(4, "clifIntegral", "this package has no CPU path; the reference's CPU branch is cvIntegral")
    return env.integral(source)


def clodDetectObjects(image, cascade: Cascade, env: Environment, min_window_size=(0, 0), max_window_size=(0, 0),
                      min_neighbors: int = 0, flags: int = 0, use_opencl: bool = True,
                      vj_flags: int = 0) -> DetectResult:
    """clod.h:72-81 / clod.cpp:1339-1356 with use_opencl=CL_TRUE → clodDetectObjectsOpenCL
    (clod.cpp:1176-1336).  `image` may also be a batch (see Environment.detect).  At the reference's own signature a cascade
    with tilted features behaves as in the reference — precomputeFeatures never reads the flag (clod.cpp:448-492), the
    rectangles count as upright ones — where Environment.detect refuses it unless VJ_FLAG_TILTED_AS_UPRIGHT is given."""
    vj_flags |= VJ_FLAG_TILTED_AS_UPRIGHT
    if not use_opencl:
        # the reference's CPU evaluators (clod.cpp:1358-1499) return the skip-thinned window set; the device computes the
        # same set.  The block variant (clod.cpp:821-1173) keeps `step` in double: two more grids (VJ_FLAG_GRID_F64).
        vj_flags |= VJ_FLAG_SKIP_LIST if flags & CLOD_PER_STAGE_ITERATIONS else VJ_FLAG_SKIP_ROW
        if flags & CLOD_BLOCK_IMPLEMENTATION:
            vj_flags |= VJ_FLAG_GRID_F64
    p = default_params(min_w=int(min_window_size[0]), min_h=int(min_window_size[1]),
                       max_w=int(max_window_size[0]), max_h=int(max_window_size[1]),
                       min_neighbors=int(min_neighbors), flags=int(vj_flags))
    return env.detect(cascade, image, p)


def cvHaarDetectObjects(image, cascade: Cascade, env: Environment, scale_factor: float = 1.1, min_neighbors: int = 3,
                        flags: int = 0, min_size=(0, 0), vj_flags: int = 0) -> DetectResult:
    """The reference demo's OpenCV leg (main.cpp:145: cvHaarDetectObjects(img, cascade, storage, 1.1, ...)) as
    tempcv.cpp:1188-1456 specifies its scale-cascade path, on the device (OpenCV arithmetic profile).  `flags`:
    0 or CV_HAAR_DO_CANNY_PRUNING.  The values CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT and CV_HAAR_DO_ROUGH_SEARCH are refused
    in `flags` only: their paths are reached through `vj_flags`, which this function forwards — VJ_FLAG_CV_SCALE_IMAGE for the
    scale-image branch (tempcv.cpp:1257-1329), VJ_FLAG_CV_FIND_BIGGEST (| VJ_FLAG_CV_ROUGH_SEARCH) for the find-biggest search
    (tempcv.cpp:1353-1490) — or through Environment.detect_opencv(flags=...)."""
    if flags & ~CV_HAAR_DO_CANNY_PRUNING:
        raise VjError(4, "cvHaarDetectObjects", "only flags 0 and CV_HAAR_DO_CANNY_PRUNING (the scale-cascade path) are taken in `flags`; "
                      "CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT and CV_HAAR_DO_ROUGH_SEARCH are reached through vj_flags")
    if flags & CV_HAAR_DO_CANNY_PRUNING:
        vj_flags |= VJ_FLAG_CV_CANNY_PRUNING
    return env.detect_opencv(cascade, image, min_size, scale_factor, min_neighbors, vj_flags)


def cvHaarDetectObjectsForROC(image, cascade: Cascade, env: Environment, scale_factor: float = 1.1, min_neighbors: int = 3,
                              flags: int = CV_HAAR_SCALE_IMAGE, min_size=(0, 0), max_size=(0, 0)) -> DetectResult:
    """cvHaarDetectObjectsForROC(image, cascade, storage, rejectLevels, levelWeights, scale_factor, min_neighbors, flags, min_size,
    max_size, outputRejectLevels = true) (tempcv.hpp:282-286; tempcv.cpp:1188-1503), on the device: the result's .reject_levels and
    .level_weights are the two vectors the reference fills.  `flags` takes the CV_HAAR_* values; without CV_HAAR_SCALE_IMAGE, or
    with CV_HAAR_FIND_BIGGEST_OBJECT, the call is refused (Environment.detect_opencv_roc says why)."""
    vj_flags = 0
    for cv_bit, vj_bit in ((CV_HAAR_DO_CANNY_PRUNING, VJ_FLAG_CV_CANNY_PRUNING), (CV_HAAR_SCALE_IMAGE, VJ_FLAG_CV_SCALE_IMAGE),
                           (CV_HAAR_FIND_BIGGEST_OBJECT, VJ_FLAG_CV_FIND_BIGGEST), (CV_HAAR_DO_ROUGH_SEARCH, VJ_FLAG_CV_ROUGH_SEARCH)):
        if flags & cv_bit:
            vj_flags |= vj_bit
    return env.detect_opencv_roc(cascade, image, min_size, max_size, scale_factor, min_neighbors, vj_flags)

def _window_args(windows, scales, scale_dtype, start_stage):
    """The window list as contiguous vj_window rows, the scales as a 1-D array of scale_dtype; ValueError for what is neither."""
    w = np.asarray(windows)
    if w.dtype != WINDOW_DTYPE:
        if not np.issubdtype(w.dtype, np.integer) and w.size:
            raise ValueError("windows must be integer rows of (frame, x, y, scale)")
        if w.size and (w.ndim != 2 or w.shape[1] != 4):
            raise ValueError("windows must be rows of (frame, x, y, scale)")
        if w.size and (w.min() < -2**31 or w.max() >= 2**31):
            raise ValueError("window members must fit an int32")
        w = w.reshape(-1, 4).astype(np.int32)
    w = np.ascontiguousarray(w)
    sc = np.ascontiguousarray(np.atleast_1d(np.asarray(scales, scale_dtype)))
    if sc.ndim != 1:
        raise ValueError("scales must be a 1-D list of factors")
    if start_stage != int(start_stage):
        raise ValueError("start_stage must be an integer")
    return w, sc


# C function, scale dtype, result dtype and the result fields returned, of the two window-list calls
_CV_WINDOWS = ("vj_run_windows_opencv", np.float64, WINDOW_RESULT_DTYPE, ("result", "stage_sum"))
_CLOD_WINDOWS = ("vj_run_windows", np.float32, CLOD_WINDOW_RESULT_DTYPE, ("result", "stage_sum", "variance"))


def _run_windows(fn, scale_dtype, result_dtype, fields, env, cascade: Cascade, frames, windows, scales, start_stage, color, flags=None):
    """One window-list call (`flags`: for the C function that takes them); the result's `fields` as arrays of their own."""
    w, sc = _window_args(windows, scales, scale_dtype, start_stage)
    if flags is not None and (flags != int(flags) or not 0 <= int(flags) < 2**32):
        raise ValueError("flags must be an unsigned 32-bit integer")
    n = int(w.shape[0])
    imgs, nf, keep = Environment._images(frames, color, env._device if env is not None else None)
    out = np.zeros(n, result_dtype)
    _check(getattr(load_library(), fn)(env._h if env is not None else None, cascade._h, imgs, nf, sc.ctypes.data, len(sc), w.ctypes.data, n, int(start_stage),
                                       *(() if flags is None else (int(flags),)), out.ctypes.data), fn)
    return tuple(out[f].copy() for f in fields)


def run_windows_opencv(frames, cascade: Cascade, env: Environment, windows, scales, start_stage: int = 0, color: bool = False):
    """cvSetImagesForHaarClassifierCascade + cvRunHaarClassifierCascade on a list of windows, on the device (vj_run_windows_opencv).
    windows: rows of (frame, x, y, scale) with `scale` an index into `scales` (any finite factors > 0).  Returns (results int32[n],
    stage_sums float64[n]) in the order of `windows`: result -1 at the border, 1 on a pass, -i on a reject at stage i of a linear
    cascade (0 at stage 0), 0 on every reject of a stage tree; stage_sum is the f64 sum of the stage whose verdict ended the run
    (0.0 with result -1 and with start_stage >= the stage count).  frames: 2-D uint8 arrays of one size, (h, w, 3|4) BGR / BGRA
    arrays with color=True, or DeviceFrames.  The arguments are checked before the environment is used."""
    return _run_windows(*_CV_WINDOWS, env, cascade, frames, windows, scales, start_stage, color)


def cvRunHaarClassifierCascade(gray, cascade: Cascade, env: Environment, pt, scale: float = 1.0, start_stage: int = 0) -> int:
    """cvRunHaarClassifierCascade(cascade, pt, start_stage) (tempcv.cpp:974-984) after cvSetImagesForHaarClassifierCascade(cascade,
    sum, sqsum, tilted, scale) on `gray`'s integral images: one window through run_windows_opencv; pt = (x, y)."""
    res, _ = run_windows_opencv(gray, cascade, env, [(0, int(pt[0]), int(pt[1]), 0)], [float(scale)], start_stage, color=np.ndim(gray) == 3)
    return int(res[0])


def run_windows(frames, cascade: Cascade, env: Environment, windows, scales, start_stage: int = 0, flags: int = 0, color: bool = False):
    """runCascade (clod.cpp:736-787) with computeVariance (:418-446) on a list of windows, on the device (vj_run_windows): the clod
    profile's arithmetic.  windows: rows of (frame, x, y, scale) with `scale` an index into `scales` (the reference's current_scale,
    float32: any finite values > 0).  Returns (results int32[n], stage_sums float32[n], variances float32[n]) in the order of
    `windows`: result VJ_WINDOW_OUTSIDE for a window that does not lie inside its frame (x >= 0, y >= 0, x + sw <= W, y + sh <= H),
    1 on a pass, -i on a reject at stage i of a linear cascade (0 at stage 0), 0 on every reject of a stage tree; stage_sum is the
    f32 sum of the stage whose verdict ended the run (0.0 outside and with start_stage >= the stage count); variance is the norm
    factor of every inside window.  flags: VJ_FLAG_SIGNED_MEAN, VJ_FLAG_TILTED_AS_UPRIGHT.  frames: 2-D uint8 arrays of one size,
    (h, w, 3|4) BGR / BGRA arrays with color=True, or DeviceFrames.  The arguments are checked before the environment is used."""
    return _run_windows(*_CLOD_WINDOWS, env, cascade, frames, windows, scales, start_stage, color, flags)


def runCascade(gray, cascade: Cascade, env: Environment, pt, scale: float = 1.0) -> int:
    """runCascade (clod.cpp:736-787) for the window at pt = (x, y) of `gray` at current_scale `scale`: one window through
    run_windows, tilted features read as upright rectangles as clodDetectObjects reads them; returns exit_stage."""
    res, _, _ = run_windows(gray, cascade, env, [(0, int(pt[0]), int(pt[1]), 0)], [float(scale)], 0, VJ_FLAG_TILTED_AS_UPRIGHT,
                            color=np.ndim(gray) == 3)
    return int(res[0])
