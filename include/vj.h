/*
 * vj.h — C ABI of the MI355X-native Viola–Jones detect path (libvjhip.so).
 *
 * This is the drop-in boundary for the reference's clif/clod detect path
 * (GabrieleCocco/CLFaceDetection).  Every entry point names the reference
 * interface it replaces (file:line, relative to CLFaceDetection/).  The
 * reference's own boundary is C++ with OpenCV/OpenCL types; neither exists on
 * the target, so this header uses plain pointers, sizes and POD structs only
 * (no torch types, no C++ types).  Errors are integer return codes — the
 * reference calls exit() through clCheckOrExit (clod.cpp:114…); this library
 * never exits the process.
 *
 * There is NO CPU fallback behind these calls: every function that computes on
 * images runs hand-written HIP kernels on a gfx950 device and fails with
 * VJ_ERR_NO_DEVICE when none is usable.  Host-only helpers (cascade loading,
 * scale planning, feature-table construction) are the reference's host logic
 * (clod.cpp:371-415, 529-578) and run on the CPU in the reference too.
 */
#ifndef VJ_H_
#define VJ_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(VJ_BUILDING) && defined(__GNUC__)
#pragma GCC visibility push(default)   /* only the names declared here are exported */
#endif

/* ------------------------------------------------------------------ errors */
enum {
    VJ_OK = 0,
    VJ_ERR_ARG = 1,         /* null / out-of-range argument                      */
    VJ_ERR_IO = 2,          /* file cannot be opened / read / written            */
    VJ_ERR_PARSE = 3,       /* malformed cascade file                            */
    VJ_ERR_UNSUPPORTED = 4, /* e.g. tilted features (clod ignores them; we refuse) */
    VJ_ERR_NO_DEVICE = 5,   /* no usable HIP device                              */
    VJ_ERR_HIP = 6,         /* a HIP runtime call failed (see vj_last_error)     */
    VJ_ERR_NOMEM = 7,
    VJ_ERR_LIMIT = 8        /* image / batch exceeds an addressing limit         */
};
const char* vj_strerror(int code);
/* Thread-local detail string for the last failing call on this thread. */
const char* vj_last_error(void);

/* ----------------------------------------------------------------- cascade */
/* Replaces cvLoad(xml) → CvHaarClassifierCascade* (main.cpp:36; loader spec
 * tempcv.cpp:1749-2089, struct layout tempcv.hpp:70-112).                      */
typedef struct vj_cascade vj_cascade;

typedef struct vj_cascade_info {
    int32_t win_w, win_h;      /* orig_window_size                              */
    int32_t n_stages, n_trees, n_nodes, n_alpha;
    int32_t max_trees_per_stage, max_nodes_per_tree;
    int32_t n_tilted;          /* nodes with <tilted>1                          */
    int32_t n_three_rect;      /* nodes with 3 rectangles                       */
    int32_t is_stump_based;    /* every tree has exactly one node               */
    int32_t is_stage_tree;     /* some stage has next != -1                     */
} vj_cascade_info;

typedef struct vj_stage_desc {  /* CvHaarStageClassifier (tempcv.hpp:95-105)    */
    int32_t first_tree, n_trees;
    float   threshold;
    int32_t parent, next, child;
} vj_stage_desc;

typedef struct vj_rect_desc { int32_t x, y, w, h; float weight; } vj_rect_desc;

typedef struct vj_node_desc {   /* one node of a CvHaarClassifier (tempcv.hpp:81-93) */
    int32_t n_rects;            /* 2 or 3 (rects with weight != 0)              */
    int32_t tilted;
    float   threshold;
    int32_t left, right;        /* >0: node index inside the tree; <=0: alpha[-v] */
    vj_rect_desc rect[3];
} vj_node_desc;

typedef struct vj_tree_desc { int32_t first_node, n_nodes, first_alpha; } vj_tree_desc;

/* OpenCV old-format XML (<opencv_storage><NAME type_id="opencv-haar-classifier">). */
int  vj_cascade_load_xml(const char* path, vj_cascade** out);
/* Compact binary form shipped under clfacedetection_amd/data (*.vjc). */
int  vj_cascade_load(const char* path, vj_cascade** out);
int  vj_cascade_save(const vj_cascade* c, const char* path);
/* A cascade the caller already holds in memory — the reference's callers get a CvHaarClassifierCascade*
 * from cvLoad (main.cpp:36; struct layout tempcv.hpp:70-112) and hand it to clodDetectObjects unchanged
 * (clod.h:72-81).  The arrays are copied and validated; stage `child` links are derived as
 * icvReadHaarClassifier does (tempcv.cpp:2080-2083) when every child is -1.  INTEGRATION.md shows the
 * CvHaarClassifierCascade -> arrays walk that keeps clodDetectObjects' signature.                       */
int  vj_cascade_from_arrays(int win_w, int win_h, const vj_stage_desc* stages, int n_stages,
                            const vj_tree_desc* trees, int n_trees, const vj_node_desc* nodes, int n_nodes,
                            const float* alpha, int n_alpha, vj_cascade** out);
void vj_cascade_free(vj_cascade* c);
int  vj_cascade_get_info(const vj_cascade* c, vj_cascade_info* out);
/* Read-only views into the flat arrays (valid until vj_cascade_free). */
const vj_stage_desc* vj_cascade_stages(const vj_cascade* c);
const vj_tree_desc*  vj_cascade_trees(const vj_cascade* c);
const vj_node_desc*  vj_cascade_nodes(const vj_cascade* c);
const float*         vj_cascade_alpha(const vj_cascade* c);
const char*          vj_cascade_notice(const vj_cascade* c);  /* license text of the source XML */

/* ------------------------------------------------------------------ params */
/* Arguments of clodDetectObjects (clod.h:72-81) that are not the image/cascade. */
enum {
    VJ_FLAG_COUNTERS     = 1u << 0, /* fill vj_result.counters + stage_entered   */
    VJ_FLAG_SIGNED_MEAN  = 1u << 1, /* reproduce clod.cpp:426 literally: window
                                       pixel sum read through int* (differs from
                                       the default unsigned read only when the
                                       sum >= 2^31)            */
    /* The reference's CPU variants thin the window grid with a data-dependent skip ("P2");
     * its OpenCL kernel — the default contract here, "P1" — evaluates every grid window.  Linear cascades. */
    VJ_FLAG_SKIP_LIST    = 1u << 2, /* CLOD_PER_STAGE_ITERATIONS CPU variant (clod.cpp:1434-1482, runSubwindow
                                       :681-734): after a stage-0 reject the next entry of the FLATTENED
                                       row-major window list is not evaluated (:729-732; crosses row ends) */
    VJ_FLAG_SKIP_ROW     = 1u << 3, /* plain CPU variant (clod.cpp:1409-1432): window positions are
                                       round(index * step) — half away from zero (:1416) instead of
                                       precomputeWindows' lrint (:514) — and the next window of the ROW is
                                       skipped after a stage-0 reject (x_incr, :1430)                      */
    VJ_FLAG_GRID_F64     = 1u << 4, /* with one of the two flags above: the same loop inside the block variant
                                       (CLOD_BLOCK_IMPLEMENTATION, clod.cpp:821-1173), which keeps `step` as a
                                       double (:862): grid ends lrint((W - w) / step) in f64 (:890-891) and
                                       positions from the f64 product — lrint in the row loop (:941-942),
                                       round() in the per-stage lists (:1034): a third and a fourth grid       */
    VJ_FLAG_TILTED_AS_UPRIGHT = 1u << 5, /* a cascade with <tilted>1 features in the clod profile: precomputeFeatures
                                       never reads the flag (clod.cpp:448-492 takes haar_feature[0]'s rectangles as they are),
                                       so the reference evaluates such rectangles as UPRIGHT ones — 12 of the 19 cascades
                                       it ships have them.  Without this flag the clod-profile entry points refuse the
                                       cascade (VJ_ERR_UNSUPPORTED: the result is not a meaningful detection); with it they
                                       reproduce the reference's arithmetic.  vj_detect_opencv evaluates tilted features on
                                       the tilted integral as OpenCV does and ignores the flag.                            */
    VJ_FLAG_CV_CANNY_PRUNING = 1u << 6, /* vj_detect_opencv only (OpenCV profile): cvHaarDetectObjects' CV_HAAR_DO_CANNY_PRUNING
                                       (tempcv.hpp:127).  One edge map per frame, cvCanny(gray, edges, 0, 50, 3) (:1337-1343, see
                                       vj_canny), and before the border rule and the cascade a test per visited window (:1147-1158,
                                       :1385-1400): with (w, h) the scaled window, s = the edge map's sum and sq = the frame's own
                                       sum over [x + cvRound(0.15 w), + cvRound(0.7 w)) x [y + cvRound(0.15 h), + cvRound(0.7 h)),
                                       both int; s < 100 || sq < 20 prunes the window: not evaluated, and the walk skips the next
                                       position as after a reject.  counters.windows counts pruned windows, stage_entered[0] does
                                       not.  The clod-profile entry points ignore the flag.                                   */
    VJ_FLAG_CV_SCALE_IMAGE = 1u << 7,   /* vj_detect_opencv only (OpenCV profile): cvHaarDetectObjects' CV_HAAR_SCALE_IMAGE branch
                                       (tempcv.hpp:128; tempcv.cpp:1257-1329, invoker :989-1113).  The IMAGE is scaled, not the
                                       cascade: for factor = 1, scale_factor, ... the frame is resized to (cvRound(W / factor),
                                       cvRound(H / factor)) (cvResize CV_INTER_LINEAR, see vj_resize_linear), integrated, and the
                                       cascade runs at its base size (cvSetImagesForHaarClassifierCascade with scale 1) on EVERY
                                       position x, y = 0, ystep, ... < size - window with ystep = factor > 2 ? 1 : 2 — a reject
                                       skips nothing, the border rule cannot fire.  A pass reports (cvRound(x * factor),
                                       cvRound(y * factor), cvRound(win_w * factor), cvRound(win_h * factor)).  The loop ends at the
                                       first level smaller than the window or whose scaled window exceeds the frame; levels whose
                                       scaled window is below min_w / min_h are skipped and keep their scale_idx.
                                       counters.windows = grid positions of all evaluated levels.  VJ_FLAG_CV_CANNY_PRUNING is
                                       ignored under this flag (the reference never reads doCannyPruning in this branch): no edge
                                       map is computed.  Stumps, multi-node trees, stage trees and tilted features all run (linear cascades: large levels on LDS tiles).  A
                                       pyramid that does not fit the 32-bit offsets returns VJ_ERR_LIMIT.  The clod-profile entry
                                       points ignore the flag.                                                                */
    VJ_FLAG_CV_FIND_BIGGEST = 1u << 8,  /* vj_detect_opencv only (OpenCV profile): cvHaarDetectObjects' CV_HAAR_FIND_BIGGEST_OBJECT
                                       (tempcv.hpp:129; tempcv.cpp:1353-1490).  VJ_FLAG_CV_SCALE_IMAGE and VJ_FLAG_CV_CANNY_PRUNING
                                       are ignored under this flag (:1227, :1254).  The factors are counted as on the plain path and
                                       then walked DOWN from the largest by repeated multiplication with 1 / scale_factor; the loop
                                       breaks at the first window below min_w / min_h.  After every scale a frame that has
                                       candidates and no object yet groups all of them (groupRectangles(max(min_neighbors, 1),
                                       0.2)); the first group of strictly greatest area becomes maxRect, is appended to the
                                       candidates, and from then on the frame is searched only inside scanROI = maxRect widened by
                                       cvRound(0.2 w), cvRound(0.2 h) (clamped to the frame, :1445-1448), with minSize =
                                       cvRound(0.4 w), cvRound(0.4 h).  At the end all candidates are grouped and the first group of
                                       strictly greatest area is the result: at most ONE vj_rect per frame, sorted by frame, weight
                                       = its neighbors, scale_idx = -1; min_neighbors 0 counts as 1.  The search state of every
                                       frame lives on the device and steers the kernels: one round per scale, all enqueued up
                                       front, no host round trip in between.  counters.windows = positions the walks
                                       visited over all evaluated scales of all frames.  vj_timing: integral_ms and cascade_ms as
                                       always (cascade_ms covers all rounds), n_cascade_launches the true count, n_launches = 0 —
                                       the path leaves no per-launch records: it has more launches than VJ_MAX_LAUNCHES.  A frame
                                       that gathers more than 2048 candidates before its first grouped object returns
                                       VJ_ERR_LIMIT.  The clod-profile entry points ignore the flag.                          */
    VJ_FLAG_CV_ROUGH_SEARCH = 1u << 9,  /* vj_detect_opencv only (OpenCV profile): cvHaarDetectObjects' CV_HAAR_DO_ROUGH_SEARCH
                                       (tempcv.hpp:130), read only by the find-biggest search (:1450): minSize after the first
                                       grouped object is cvRound(0.6 w), cvRound(0.6 h) instead of 0.4.  Without
                                       VJ_FLAG_CV_FIND_BIGGEST it changes nothing.  The clod-profile entry points ignore it.    */
    VJ_FLAG_CV_CHAIN_DEVICE = 1u << 10, /* vj_detect_opencv_chain only, and only in p_first->flags: the first cascade's rectangles
                                       become the second one's regions and work units ON THE DEVICE, and the host
                                       waits once per sub-batch, after both cascades.  Taken when both flag words are otherwise
                                       within VJ_FLAG_COUNTERS; next to a flag that sends the chain through the two public calls
                                       it is ignored.  The results — rectangles, order, counters — are those of the call without
                                       it.  Not the default yet: what it gains is measured and recorded in DESIGN.md 4.10.
                                       Every other entry point ignores the bit; no plan is keyed on it.                         */
    VJ_FLAG_EQUALIZE_HIST = 1u << 11,   /* cvtColor -> equalizeHist -> detect on the device: every frame is equalized
                                       on its own — cv::equalizeHist on the gray image vj_grayscale returns, the image
                                       vj_equalize_hist returns — right after it is staged, and the call goes on with the equalized
                                       gray frames.  The result — rectangles, order, counters, reject levels — is that of the same
                                       call without the flag on the images vj_equalize_hist returns for its frames.  Valid in
                                       vj_params.flags, vj_cv_params.flags and vj_cv_roc_params.flags; honoured by vj_detect (skip
                                       modes and grouping included), vj_detect_opencv (with every other flag of its profile),
                                       vj_detect_opencv_roc, vj_detect_mixed and vj_detect_opencv_mixed (an atlas is packed through
                                       its frames' look-up tables).  Every other entry point that takes frames and flags — the
                                       region and chain calls of both profiles, vj_run_windows, vj_stream_create — returns
                                       VJ_ERR_UNSUPPORTED and vj_last_error names the flag: none ignores it, an un-equalized result
                                       would look plausible.  No plan or cache is keyed on it; vj_timing.integral_ms includes
                                       the stage.                                                                               */
};

typedef struct vj_params {
    int32_t  min_w, min_h;     /* min_window_size (0 = none)                    */
    int32_t  max_w, max_h;     /* max_window_size (0 = unlimited, clod.cpp:394) */
    float    scale_factor;     /* reference hard-codes 1.1f (clod.cpp:1184)     */
    uint32_t min_neighbors;    /* 0 = raw candidates (the parity contract); else grouped */
    uint32_t flags;
    uint64_t scale_mask[2];    /* bit k set = evaluate scale index k (k < 127); both
                                  words 0 = every scale; bit 127 (VJ_SCALE_MASK_NONE
                                  in word 1) = no scale at all: an empty share, the
                                  call returns no rectangles.  Shards one frame's
                                  scales across GPUs; no counterpart in the reference. */
} vj_params;
#define VJ_SCALE_MASK_NONE (1ull << 63)   /* in scale_mask[1]: what vj_shard_scales gives a rank that gets no scale */
void vj_params_default(vj_params* p);   /* {0,0,0,0,1.1f,0,0,{0,0}} */

/* ------------------------------------------------------ host scale planning */
/* setupScale + scale enumeration (clod.cpp:371-415, 1198-1204). */
typedef struct vj_scale_info {
    int32_t  scale_idx;        /* k in s_k = fl32(s_{k-1} * scale_factor)       */
    float    scale;            /* s_k                                           */
    float    step;             /* (float)MAX(2.0, s)                            */
    int32_t  win_w, win_h;     /* scaled_window_size                            */
    int32_t  equ_x, equ_y, equ_w, equ_h;  /* equ_rect                           */
    uint32_t area;             /* scaled_window_area                            */
    int32_t  nx, ny;           /* end_point: window grid is [0,nx) x [0,ny)     */
    int32_t  accepted;         /* 0 when setupScale returned -1                 */
} vj_scale_info;
/* Writes up to cap entries (all enumerated scales, accepted or not); *n = count. */
int vj_plan_scales(const vj_cascade* c, int width, int height, const vj_params* p,
                   vj_scale_info* out, int cap, int* n);

/* precomputeKernelCascade (clod.cpp:529-578) for one scale: per node, 3 rects of
 * {left_top, right_top, left_bottom, right_bottom element offsets, weight}.
 * `offsets` receives n_nodes*12 uint32, `weights` n_nodes*3 floats.            */
int vj_plan_feature_table(const vj_cascade* c, int width, const vj_scale_info* s,
                          uint32_t* offsets, float* weights);

/* The LDS-tile side of the plan that a fresh environment (shipped settings) builds for a call of n_frames
 * frames: which scales run on image tiles, in which shapes.  Host only, read only, no device needed.
 * One entry per accepted scale with windows, in scale order.                                           */
typedef struct vj_tile_info {
    int32_t  scale_idx;
    float    scale, step;
    int32_t  nx, ny;
    int32_t  lds_class;        /* LDS class of the scale's own tile shape; -1: the scale stays on the
                                  global-gather chain (the fields below are then 0)                   */
    int32_t  tile_w, tile_h;   /* windows per tile row / window rows per tile                         */
    int32_t  pitch, rows;      /* the staged image tile: dwords per row, rows                         */
    int32_t  reach_x, reach_y; /* how far right / below a window's origin its features read           */
    int32_t  lead_scale_idx;   /* scale group: the member whose tile the frame's tile list stages for
                                  all of them (its class, shape and class block); itself: not grouped.
                                  The region pass stages every scale in its own shape.                */
    int32_t  tile_row_end;     /* window rows [0, tile_row_end) run on tiles; the chain balance gave the
                                  rest to the global-gather chain                                     */
} vj_tile_info;
typedef struct vj_tile_plan_info {
    uint32_t header_bytes;          /* LDS a tile workgroup holds in front of its image tile           */
    uint32_t gather_reserve_bytes;  /* LDS per CU left to the global-gather chain's workgroup          */
    uint32_t max_tile_windows;      /* most windows a tile may hold (a tile holds at least 64)         */
    uint32_t n_classes;
    uint32_t class_lds[4];          /* dynamic LDS of each class launch (0: the class has no tiles)    */
    int32_t  class_per_cu[4];       /* workgroups of the class that share a CU (0: a fixed budget)     */
    uint32_t class_tiles[4];        /* tiles per frame of each class launch                            */
} vj_tile_plan_info;
#define VJ_PLAN_TILES_FORMER_SHAPES 1u  /* shapes as chosen before the tiles grew into the LDS of the former
                                           stump-parallel finish (a diagnostic: tools/plan_dump.py)   */
#define VJ_PLAN_TILES_NO_GROUPS     2u  /* one tile per scale (what VJ_TILE_GROUP=1 gives)              */
int vj_plan_tiles(const vj_cascade* c, int width, int height, const vj_params* p, int n_frames,
                  uint32_t flags, vj_tile_plan_info* info, vj_tile_info* out, int cap, int* n);
/* vj_plan_tiles at a chain balance of the caller's choice: what a call runs after
 * vj_env_configure("tile_split", ...) or where the balance feedback has walked to.  tile_split < 0: the shipped value
 * of that batch size (exactly what vj_plan_tiles gives).  `cut` (may be NULL) says how the plan divides a frame's
 * windows between the two chains: tile windows are the sum of nx * tile_row_end over the tile scales, the rest must
 * be covered by the first-pass units of the global-gather chain.  `gather_windows` (may be NULL; cap entries, one per
 * entry of `out`) receives the windows of each scale those units cover.  Host only, read only, like vj_plan_tiles. */
typedef struct vj_tile_cut_info {
    float    tile_split;            /* the chain balance the plan was built with                       */
    uint32_t gather_units;          /* first-pass units of the global-gather chain, per frame          */
    uint64_t gather_windows;        /* windows those units cover (each clipped to its scale's grid)    */
    uint64_t plan_windows;          /* windows per frame of the whole plan (vj_count_windows)          */
} vj_tile_cut_info;
int vj_plan_tiles_split(const vj_cascade* c, int width, int height, const vj_params* p, int n_frames,
                        uint32_t flags, float tile_split, vj_tile_plan_info* info, vj_tile_cut_info* cut,
                        vj_tile_info* out, uint64_t* gather_windows, int cap, int* n);

/* ------------------------------------------------------------- environment */
/* clodInitEnvironment/clodReleaseEnvironment (clod.h:61-65, clod.cpp:72-100,
 * 173-180) — one env per device; not thread-safe (neither is the reference).   */
typedef struct vj_env vj_env;
int  vj_env_create(int device_index, vj_env** out);
void vj_env_destroy(vj_env* e);
/* clodInitBuffers + clifInitBuffers (clod.cpp:102-163, clif.cpp:105-224):
 * pre-size device buffers; optional — vj_detect grows them on demand.          */
int  vj_env_reserve(vj_env* e, int max_w, int max_h, int max_batch);
int  vj_env_device_name(const vj_env* e, char* buf, size_t cap);
/* Tunables — speed only: results never depend on them (tests/test_gpu_tunable_parity.py runs every key at values other than
 * its default against the oracle, and fails when a key has no row in its table).  One line per group here; every key
 * with its values, default and the measurement behind the default is in DESIGN.md §7.  Lists are comma-separated.
 *   launch structure   pass_split, pass_cut_nodes, blocks_per_cu, concurrent, concurrent_blocks_per_cu, max_subbatch, det_cap
 *   LDS tiles          tile_classes_kb, tile_lds_reserve_kb, tile_min_windows, tile_accept_windows, tile_end, tile_min_lanes,
 *                      tile_max_dwords_per_window, tile_repack
 *   tile finish        tile_sp_begin, tile_ws_min, tile_ws_max
 *   chain balance      tile_split ("small,mid,large" or one value: static), auto_balance (1 / 0 / "reset": feedback on the
 *                      first calls of a batch workload, keyed by cascade content, frame size, parameters and batch-size class),
 *                      balance_export / balance_import (value: a file path; the found balances as text, for another environment
 *                      or process — import AFTER setting auto_balance, which clears the table)
 *   global-gather      grid_block_w, gather_waves, gather_pairs, sp_tail_max, wide_tail, min_chunk, q_slices,
 *                      q_band_px, q_group_units, q_band_min_frames (band-major first-pass units and queue pass)
 *   stage trees        general_prefix, tile_segments, seg_cut2, tree_split_queues
 *   regions / chain    rois_on_device, roi_tiles, group_max
 *   OpenCV profile     cv_tiles, cv_row_blocks, cv_tile_min_windows, cv_tile_min_windows0, cv_tile_ws_max, cv_row_blocks_tree,
 *                      cv_tile_min_windows_tree, cv_tree_chains, cv_tree_chunk, cv_tree_chain_blocks, cv_tail_max,
 *                      cv_row_band_px, cv_tree2, cv_tiles_tilted,
 *                      cv_tree_queue_cap (tests)
 *   single frames      one_pass_max_frames (the gather chain in one pass for calls of few large frames; 0 = off)
 *   integral           integral_rows (0 one wave per band of rows, 1 a band's chunks side by side, 2 by call size)
 *   housekeeping       plan_cache_max, defaults (value ignored: every tunable back to what vj_env_create set, the found
 *                      chain balances and cached plans dropped)
 * Unknown keys return VJ_ERR_ARG.                                               */
int  vj_env_configure(vj_env* e, const char* key, const char* value);
/* The current value of a vj_env_configure key, written to buf in the syntax configure accepts (configure(key, query(key))
 * changes nothing).  VJ_ERR_ARG for unknown keys, for the actions defaults / balance_export / balance_import, and when
 * cap is too small.                                                              */
int  vj_env_query(const vj_env* e, const char* key, char* buf, size_t cap);

/* --------------------------------------------------------------- integral */
/* clifIntegral (clif.h:63-66, clif.cpp:273-285 → cvIntegral layout):
 * sum u32 and sqsum u64, both (h+1) x (w+1) row-major, row 0 / col 0 zero.
 * `gray`, `sum`, `sqsum` are HOST pointers (the reference returns host CvMat).  */
int vj_integral(vj_env* e, const uint8_t* gray, int w, int h, int stride,
                uint32_t* sum, uint64_t* sqsum);

/* Page-locked host memory for frames (what clodInitBuffers / clifInitBuffers pre-allocate in the reference,
 * clod.cpp:102-163): frames that live in it are uploaded by DMA without a staging copy.                  */
int  vj_host_alloc(vj_env* e, size_t bytes, void** out);
void vj_host_free(vj_env* e, void* p);

/* ----------------------------------------------------------------- detect */
struct vj_image;
/* clifGrayscaleIntegral (clif.h:67-70, clif.cpp:326-335): gray conversion + both integrals of one image
 * (host or device pointer, 1 / 3 / 4 channels); outputs as vj_integral.                       */
int  vj_integral_image(vj_env* e, const struct vj_image* image, uint32_t* sum, uint64_t* sqsum);
/* The integral images as vj_detect and vj_stream keep them on the device for a batch of equal-sized frames: sum as above and
 * the squared sum as u32, the values mod 2^32 (what the detect path's readers rebuild exact window sums from).  HOST outputs,
 * dense: n_frames x (h+1) x (w+1) each.                                                                        */
int  vj_integral_batch_sq32(vj_env* e, const struct vj_image* frames, int n_frames, uint32_t* sum, uint32_t* sqsum32);
/* clifGrayscale (clif.h:55-58, clif.cpp:226-271 -> cvCvtColor BGR2GRAY): the 8-bit gray image the integral
 * kernels see, written to the HOST buffer `gray` (gray_stride bytes per row).  1-channel input is copied. */
int  vj_grayscale(vj_env* e, const struct vj_image* image, uint8_t* gray, int gray_stride);
/* The tilted integral cvIntegral(img, sum, sqsum, tilted) returns for cascades with tilted features
 * (tempcv.cpp:1335, :743-750): (h+1) x (w+1) u32, tilted(X, Y) = sum of gray(x, y) over y < Y,
 * |x - X + 1| <= Y - y - 1.  HOST output.                                                              */
int  vj_integral_tilted(vj_env* e, const struct vj_image* image, uint32_t* tilted);
/* cvCanny(gray, edges, 0, 50, 3) (OpenCV 2.4.2 imgproc; what CV_HAAR_DO_CANNY_PRUNING computes per frame, tempcv.cpp:1337-1343) on
 * the 8-bit gray image vj_grayscale returns: Sobel 3x3 with replicated borders, |dx| + |dy|, non-maximum suppression, candidates
 * m > 0, strong m > 50, and as edges every candidate 8-connected to a strong one.  255 / 0 bytes, written to the
 * HOST buffer `edges` (edges_stride bytes per row).  Host or device input, 1 / 3 / 4 channels, any row stride.                   */
int  vj_canny(vj_env* e, const struct vj_image* image, uint8_t* edges, int edges_stride);
/* cvResize(gray, dst, CV_INTER_LINEAR) for 8-bit single-channel images (OpenCV 2.4.2 imgproc; what CV_HAAR_SCALE_IMAGE computes
 * per level, tempcv.cpp:1301) on the gray image vj_grayscale returns: one level of VJ_FLAG_CV_SCALE_IMAGE's pyramid.  Fixed-point
 * bilinear with 11-bit coefficients (cvRound((1 - f) * 2048), cvRound(f * 2048)), the 2 x 2 mean (sum + 2) >> 2 when the source is
 * exactly twice the destination in both directions; the definition is DESIGN.md §4.8.  dst_w x dst_h bytes, written to the HOST
 * buffer `dst` (dst_stride bytes per row).  Host or device input, 1 / 3 / 4 channels, any row stride.                            */
int  vj_resize_linear(vj_env* e, const struct vj_image* image, int dst_w, int dst_h, uint8_t* dst, int dst_stride);
/* cv::equalizeHist for 8-bit single-channel images (OpenCV imgproc/histogram.cpp, 2.4.4 .. 4.x) on the gray image vj_grayscale
 * returns; what VJ_FLAG_EQUALIZE_HIST puts in front of a detect call.  hist[v] = pixels of value v; i = the lowest v with
 * hist[v] != 0; an image of one value is returned unchanged; else scale = 255.f / (float)(w * h - hist[i]), lut[i] = 0 and, for
 * k > i, lut[k] = saturate_cast<uchar>((float)(hist[i + 1] + .. + hist[k]) * scale) in binary32 with round-half-to-even;
 * dst = lut[gray] (the definition is DESIGN.md §4.15).  w x h bytes, written to the HOST buffer `dst` (dst_stride bytes per row).
 * Host or device input, 1 / 3 / 4 channels, any row stride.  Null arguments or dst_stride < width: VJ_ERR_ARG.                   */
int  vj_equalize_hist(vj_env* e, const struct vj_image* image, uint8_t* dst, int dst_stride);
typedef struct vj_image {
    const uint8_t* data;       /* 8-bit, interleaved channels.  Read only by every entry point but vj_paint, which WRITES the
                                  painted pixels through this pointer (the memory must be writable)            */
    int32_t width, height;
    int32_t stride;            /* bytes per row                                 */
    int32_t on_device;         /* 0: host pointer; 1: device pointer on env's GPU.  The library's streams are created with
                                  hipStreamNonBlocking: they wait for no other stream, the null stream included.  All work
                                  that writes a device-resident frame must be COMPLETE before the call that is given it (an
                                  event or stream synchronize of the caller's; queued is not enough), and nothing may write it
                                  until that call has returned (vj_stream_submit: until the batch is collected).  Every call
                                  returns after its own work is complete, so its results are ready for any stream.  What the
                                  Python wrapper does on top of this for its callers: INTEGRATION.md                       */
    int32_t channels;          /* 0 or 1: gray (the configs' contract); 3: BGR, 4: BGRA — converted on the
                                  fly with OpenCV's 8-bit BGR2GRAY, as setupImage does (clif.cpp:326-335) */
} vj_image;

typedef struct vj_rect {       /* CLODWeightedRect (clod.h:39-42) + provenance  */
    int32_t x, y, w, h;
    float   weight;            /* reference leaves it unset/0 for raw results   */
    int32_t frame;
    int32_t scale_idx;
} vj_rect;

#define VJ_MAX_STAGES 64
typedef struct vj_counters {
    uint64_t windows;          /* candidate windows enumerated                  */
    uint64_t stump_evals;      /* tree-node evaluations as SURVEY.md §8d counts them: the nodes a window's walk visits
                                  (every node of an entered stage for stumps; root + visited children for trees) */
    uint64_t gather_bytes;     /* 48*windows + 16*sum(nrects)   */
    uint64_t stage_entered[VJ_MAX_STAGES]; /* windows entering each stage       */
} vj_counters;

#define VJ_MAX_PASSES 8
#define VJ_MAX_LAUNCHES 16
enum { VJ_LAUNCH_GRID = 0,   /* first pass, windows enumerated from the grid, L2 gathers */
       VJ_LAUNCH_QUEUE = 1,  /* later pass over the survivor queue, L2 gathers           */
       VJ_LAUNCH_TILE = 2,   /* whole cascade on image tiles staged in LDS               */
       VJ_LAUNCH_BLOCK = 3 };/* no longer produced (was: 2-D window blocks, L2 gathers)   */
typedef struct vj_launch {
    int32_t  kind;             /* VJ_LAUNCH_*                                   */
    int32_t  lds_class;        /* tile launches: LDS size class                 */
    int32_t  stage_begin, stage_end;  /* stages it may run (tile launches: up to stage_end) */
    float    ms;               /* HIP-event time, summed over sub-batches       */
    uint32_t lds_bytes;
    uint64_t scale_mask[2];    /* scale indices it covers, wholly or in part (queue passes: all) */
    uint64_t stage_entered[VJ_MAX_STAGES];  /* VJ_FLAG_COUNTERS: windows this launch took into each stage */
} vj_launch;
typedef struct vj_timing {     /* HIP-event times of the last vj_detect, ms     */
    float integral_ms;         /* the three integral launches (vj_detect_opencv with VJ_FLAG_CV_SCALE_IMAGE: and the pyramid
                                  launch; with VJ_FLAG_CV_CANNY_PRUNING: and the Canny
                                  and edge-integral launches before them)                                                */
    float cascade_ms;          /* all cascade passes                            */
    float total_ms;            /* first kernel start → last kernel end          */
    int32_t n_cascade_launches;
    float pass_ms[VJ_MAX_PASSES];            /* each cascade pass (its launches) */
    int32_t pass_stage_begin[VJ_MAX_PASSES]; /* stages [begin, end) it ran      */
    int32_t pass_stage_end[VJ_MAX_PASSES];
    int32_t n_launches;                      /* kernel launches of the cascade  */
    vj_launch launch[VJ_MAX_LAUNCHES];       /* each with its own HIP events    */
    float tile_split;          /* vj_detect: scales' worth of tile work the plan of this call gave to the global-gather
                                  chain ("tile_split"; found per workload by feedback unless configured) */
    int32_t balance_state;     /* 0: static balance (no feedback for this call); 1: the workload's feedback search is still
                                  running; 2: finished — the workload runs its best split from now on */
    int32_t balance_calls;     /* calls the search has measured so far for this workload (at most 40) */
} vj_timing;

typedef struct vj_result {
    vj_rect*   rects;          /* sorted by (frame, scale_idx, y, x)            */
    uint32_t   count;
    vj_counters counters;      /* valid when VJ_FLAG_COUNTERS                   */
    vj_timing  timing;
} vj_result;

/* clodDetectObjects(image, cascade, data, min, max, min_neighbors, flags, CL_TRUE)
 * (clod.h:72-81, clod.cpp:1176-1336), batched over n_frames frames of equal size (frames of differing
 * sizes: vj_detect_mixed, vj_detect_opencv_mixed below). */
int  vj_detect(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
               const vj_params* p, vj_result* out);
void vj_result_free(vj_result* r);

/* ------------------------------------------------ OpenCV arithmetic profile */
/* cvHaarDetectObjects(image, cascade, storage, scale_factor, min_neighbors, flags = 0, min_size)
 * (call site main.cpp:145; scale-cascade path as tempcv.cpp:1188-1456 keeps it, scalar branches —
 * CV_HAAR_USE_SSE is commented out at :28-36): f64 variance and stage sums; node sums as
 * cvRunHaarClassifierCascadeSum writes them — an f64 product per rectangle in stump stages flagged
 * two_rects (:872-888), otherwise int * float, i.e. a BINARY32 product widened to double before it is
 * accumulated (:907-911, icvEvalHidHaarClassifier :783-788); stage threshold - 0.0001f; cvRound-ed
 * rectangles and grid; ystep = max(2, factor); the skip after a reject (stage 0 for linear cascades, any
 * stage for stage trees, which return 0 on every reject: :834-861, :1163); the window-touches-border
 * rule; stage trees; tilted features on the tilted integral (:731, :743-750).  Raw candidates
 * (min_neighbors = 0) or cv::groupRectangles.  counters.windows = positions the sequential walk
 * visits.  Parity: against the oracle's restatement of the same lines — OpenCV itself cannot be run
 * here (unpinned).                                                                                */
typedef struct vj_cv_params {
    int32_t  min_w, min_h;     /* minSize (0 = none)                              */
    double   scale_factor;     /* 1.1                                             */
    uint32_t min_neighbors;
    uint32_t flags;            /* VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING (CV_HAAR_DO_CANNY_PRUNING),
                                  VJ_FLAG_CV_SCALE_IMAGE (CV_HAAR_SCALE_IMAGE: the other branch of
                                  cvHaarDetectObjects), VJ_FLAG_CV_FIND_BIGGEST (CV_HAAR_FIND_BIGGEST_OBJECT) and
                                  VJ_FLAG_CV_ROUGH_SEARCH (CV_HAAR_DO_ROUGH_SEARCH), each described at the flag:
                                  every flag of the function */
} vj_cv_params;
void vj_cv_params_default(vj_cv_params* p);
int  vj_detect_opencv(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
                      const vj_cv_params* p, vj_result* out);
/* cvHaarDetectObjectsForROC(image, cascade, storage, rejectLevels, levelWeights, scale_factor, min_neighbors, flags, min_size,
 * max_size, outputRejectLevels = true) (tempcv.hpp:282-286, :389-395; tempcv.cpp:1188-1503) — the function cvHaarDetectObjects wraps
 * (:1505-1516), with the two things only it has:
 *   reject levels  In the CV_HAAR_SCALE_IMAGE branch every grid window that passes the cascade of n stages, or fails one of its last
 *                  three stages n-3, n-2, n-1, is reported (:1084-1095) with the stage it reached (n for a pass) and stage_sum of the
 *                  last stage evaluated — the f64 sum the verdict compared, bit for bit.  Stage trees return 0 on every reject
 *                  (:834-861): only accepted windows are reported, with level n and the sum of the stage whose pass ended the walk.
 *   max_w, max_h   maxSize: the level loop ends at the first window larger than it (:1285); a zero member means the frame (:1230).
 * min_neighbors != 0 groups each frame with groupRectangles' level overload (vj_group_rectangles_levels, threshold min_neighbors —
 * not max(min_neighbors, 1)).  flags: VJ_FLAG_CV_SCALE_IMAGE must be set; VJ_FLAG_COUNTERS fills the counters vj_detect_opencv fills
 * for the same frames; VJ_FLAG_CV_CANNY_PRUNING and VJ_FLAG_CV_ROUGH_SEARCH are ignored, as the branch ignores them.  Refused with
 * VJ_ERR_UNSUPPORTED, `out` left empty, each because the reference's answer is not a meaningful result:
 *   without VJ_FLAG_CV_SCALE_IMAGE    the scale-cascade invoker (:1116-1185) never pushes a level: empty lists, or, once grouped
 *                                     against them, nothing at all;
 *   with VJ_FLAG_CV_FIND_BIGGEST      it clears scale-image (:1227) and then indexes an empty rweights (:1486);
 *   a cascade of fewer than 4 stages  n + result < 4 holds for rejects at stage 0: the result is every grid position.
 * Batches, sub-batches, BGR / BGRA and device-resident frames as in vj_detect_opencv.  The buffer of reported windows starts at
 * the configured "det_cap" and grows on overflow.                                                                              */
typedef struct vj_cv_roc_params {
    int32_t  min_w, min_h, max_w, max_h;   /* 0 = none / frame size */
    double   scale_factor;
    uint32_t min_neighbors;
    uint32_t flags;                        /* must hold VJ_FLAG_CV_SCALE_IMAGE; VJ_FLAG_COUNTERS optional */
} vj_cv_roc_params;
typedef struct vj_roc_result {
    vj_result r;              /* rects sorted by (frame, scale_idx, y, x); raw: weight 0; grouped: scale_idx -1, weight 0 */
    int32_t*  reject_levels;  /* r.count entries, parallel to r.rects */
    double*   level_weights;  /* r.count entries */
} vj_roc_result;
void vj_cv_roc_params_default(vj_cv_roc_params* p);   /* scale_factor 1.1, flags VJ_FLAG_CV_SCALE_IMAGE, the rest 0 */
int  vj_detect_opencv_roc(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
                          const vj_cv_roc_params* p, vj_roc_result* out);
void vj_roc_result_free(vj_roc_result* r);
/* cvSetImagesForHaarClassifierCascade(cascade, sum, sqsum, tilted, scale) + cvRunHaarClassifierCascade(cascade, pt, start_stage)
 * (tempcv.cpp:549-768, :974-984 -> cvRunHaarClassifierCascadeSum :795-972) on a caller's list of windows:
 * out[i] is the verdict on windows[i] — the window at (x, y) of frame `frame`, the cascade set to scales[scale] — in the caller's
 * order; nothing is sorted or deduplicated.
 *   result      the function's return value: -1 when the border rule holds (:817-820: x < 0, y < 0, x + real_w >= W + 1 or
 *               y + real_h >= H + 1, real = cvRound(orig * scale)); 1 on a pass; -i on a reject at stage i of a linear cascade (so
 *               a reject at stage 0 is 0); 0 on every reject of a stage tree (:834-861).
 *   stage_sum   the f64 the function leaves in stage_sum, bit for bit: the sum of the stage whose verdict ended the run (for a
 *               pass the last stage evaluated); 0.0 where it is never written (result -1, or start_stage >= the stage count,
 *               which returns 1).
 * start_stage: linear cascades start there (:864, :952); a stage tree asserts 0 (:837): anything else is VJ_ERR_ARG, as is a
 * negative value.  scales: any finite value > 0, not only members of a factor chain; any number of them per call (each has a node
 * table of its own, cached per (cascade, frame width, bits of the scale) next to the other plans).  A scale whose window exceeds
 * the frame gives -1 for every window; that is no error.  Frames: one size, gray / BGR / BGRA, host or device-resident; integrated
 * once per call (per sub-batch when the call splits), the tilted integral only for cascades with tilted nodes.  n_windows == 0 is
 * VJ_OK (whatever the other arguments, a null environment included; only the cascade and start_stage are checked first); a frame
 * or scale index out of range is VJ_ERR_ARG with `out` untouched.  At most 2^27 windows per call, and a frame whose sqsum image
 * fits one 4 GiB buffer descriptor (VJ_ERR_LIMIT). */
typedef struct vj_window        { int32_t frame, x, y, scale; } vj_window;          /* scale: index into scales[] */
typedef struct vj_window_result { int32_t result, reserved; double stage_sum; } vj_window_result;
int  vj_run_windows_opencv(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
                           const double* scales, int n_scales, const vj_window* windows, uint32_t n_windows,
                           int start_stage, vj_window_result* out /* n_windows entries, caller's */);
/* The clod profile's twin: runCascade (clod.cpp:736-787) on what setupScale (:371-415), computeVariance (:418-446) and
 * precomputeFeatures / precomputeKernelCascade (:448-492, :529-578) give, on a caller's list of windows: out[i] is
 * the verdict on windows[i] — the window at (x, y) of frame `frame`, at scales[scale] — in the caller's order; nothing is sorted or
 * deduplicated.  scales[k] is the reference's current_scale, a binary32: any finite value > 0, not only members of the 1.1f chain.
 * From it, as setupScale writes them: sw = (uint)round(win_w * s) and sh likewise (int x f32 product, rounded half away from zero),
 * equ = {round(s), round(s), round((win_w - 2) * s), round((win_h - 2) * s)}, area = equ.w * equ.h; sw and sh are clamped at 2^20.
 * setupScale's step, grid ends and min / max / image-size rejections belong to the detector's loop and play no part.  A scale with
 * sw, sh or area equal to 0 is VJ_ERR_ARG (the reference would divide by zero).
 *   inside      in 64 bits on the caller's int32 coordinates: a window is evaluated iff x >= 0, y >= 0, x + sw <= W and y + sh <= H
 *               (x = W - sw is evaluated, x = W - sw + 1 is not: there the reference reads outside the image and has no answer).
 *               Any other window gets (VJ_WINDOW_OUTSIDE, 0.0f, 0.0f) and performs no image read; a scale whose window exceeds the
 *               frame gives that for every window and builds no table: no error.
 *   variance    computeVariance's value: mean = (float)S / (float)area, var = (float)Q / (float)area - mean * mean, variance =
 *               var >= 0 ? sqrtf(var) : 1; S read unsigned, or through int* with VJ_FLAG_SIGNED_MEAN exactly as vj_detect does.
 *               Written for every inside window, whatever start_stage.
 *   result      runCascade's return value: 1 on a pass; -i on a reject at stage i of a linear cascade (stumps, or multi-node trees
 *               walked as tempcv.cpp:771-792 in clod arithmetic, as vj_detect runs them), so a reject at stage 0 is 0; for a stage
 *               tree — which the reference's clod path does not know — the walk of tempcv.cpp:834-861: 1 on a pass, 0 on every reject.
 *   stage_sum   the f32 running sum (one accumulator, added in tree order, clod.cl:81) of the stage whose verdict ended the run, for
 *               a pass the last stage evaluated; compared with the stage threshold WITHOUT OpenCV's bias.  0.0f where no stage runs:
 *               outside windows, and start_stage >= the stage count, which returns 1.
 * start_stage: linear cascades start there; a stage tree accepts only 0; anything else, or a negative value, is VJ_ERR_ARG.
 * flags: VJ_FLAG_SIGNED_MEAN is honoured; VJ_FLAG_TILTED_AS_UPRIGHT works as in vj_detect (a cascade with tilted features is refused
 * with VJ_ERR_UNSUPPORTED without it); any other bit is VJ_ERR_ARG — a window list has no skip mode, grid or counters.
 * n_windows == 0 is VJ_OK (whatever the other arguments, a null environment included; only the cascade, start_stage and flags are
 * checked first); a frame or scale index out of range is VJ_ERR_ARG with `out` untouched.  Frames: one size, gray / BGR / BGRA,
 * host or device-resident, integrated once per call (per sub-batch when the call splits).  At most 2^27 windows per call; a frame
 * whose sqsum image exceeds one 4 GiB buffer descriptor, or a scale whose features reach beyond the frame allocation (the check of
 * the other clod paths, per scale slot), is VJ_ERR_LIMIT.  Node tables are cached per (cascade, frame width, bits of the scale,
 * tilted-as-upright) next to the other plans. */
#define VJ_WINDOW_OUTSIDE INT32_MIN
typedef struct vj_clod_window_result { int32_t result; float variance; float stage_sum; int32_t reserved; } vj_clod_window_result;
int  vj_run_windows(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
                    const float* scales, int n_scales, const vj_window* windows, uint32_t n_windows,
                    int start_stage, uint32_t flags, vj_clod_window_result* out /* n_windows entries, caller's */);
/* Device times of the environment's last run-windows call of either profile (vj_run_windows_opencv or vj_run_windows) that ran a
 * pass, summed over its sub-batches: the integral images (with the tilted integral, where built) and the window-list kernel alone
 * (hipEvents around the launch).  Either may be NULL. */
int  vj_run_windows_timing(const vj_env* e, float* integral_ms, float* pass_ms);
/* What vj_detect_opencv's plan for (c, width x height, p, a batch of n_frames) holds, with the environment's
 * current settings: the LDS-tile scales and, for stage trees on tiles, the survivors' tree queue.  The
 * queue's shift and split belong to the plan: they record what earlier calls with that plan did.        */
typedef struct vj_cv_plan_info {
    uint64_t tile_windows;     /* grid windows per frame of the scales on LDS tiles                      */
    uint32_t n_tile_scales;
    uint32_t tree_prefix;      /* stage trees: leading stages the tiles run (0: linear cascade)          */
    int32_t  tree_queue;       /* stage trees on tiles: 1 one sub-queue per scale (chain pass), 2 one
                                  flat queue (tree walk); 0 the rows take the tree                        */
    int32_t  tq_shift;         /* the queue holds 1 / 2^shift of the tile windows (-1: no call yet)      */
    int32_t  tq_split_frames;  /* frames per sub-batch a call last split its batch to so that the queue
                                  fits in 2^28 entries (0: no call had to)                               */
    int32_t  reserved;
} vj_cv_plan_info;
int  vj_cv_plan_info_get(vj_env* e, const vj_cascade* c, int width, int height, int n_frames,
                         const vj_cv_params* p, vj_cv_plan_info* out);

/* A second cascade on regions of interest (BASELINE config 5: haarcascade_eye inside every face;
 * the reference's caller would hand clodDetectObjects a sub-image header: pointer + widthStep).
 * ROIs are views into `frames`.  In the result, rect.frame is the ROI's index and x / y are relative
 * to the ROI's origin.  Frames of one size: the frames' integral images are computed once and ALL
 * regions, of whatever sizes, run in one pass on them (a rectangle sum does not depend on where the
 * integral image starts; vj_detect_chain's region pass with an uploaded list; stage trees and scale
 * masks included).  Otherwise (frames of different sizes, skip modes): one vj_detect call per region
 * size on the sub-images.  Same result either way.                                               */
typedef struct vj_roi { int32_t frame, x, y, w, h; } vj_roi;
int  vj_detect_rois(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames,
                    const vj_roi* rois, int n_rois, const vj_params* p, vj_result* out);

/* Two cascades back to back with the hand-off on the device (BASELINE config 5): `first`
 * runs on the frames as vj_detect does; what it finds becomes a DEVICE-resident list of regions of interest
 * (built by kernels from the detection buffer), and `second` runs on those regions reading the frames'
 * integral images in place — rectangle sums over a region do not depend on where the integral image starts,
 * so the result equals running `second` on the sub-image (vj_detect_rois) — before anything returns to the
 * host.  p_first->min_neighbors == 0: every raw candidate is a region.  != 0: the candidates are grouped ON
 * THE DEVICE (cv::groupRectangles per frame, as vj_detect groups them on the host: same classes, same
 * averages, same order) and the grouped faces are the regions.  out_first: as vj_detect with the same
 * parameters.  out_second: rect.frame = index of the region in out_first->rects, x / y relative to the
 * region's origin.  `second` may be any cascade of upright features (stumps, trees, stage trees);
 * p_second->scale_mask selects scales by index as in vj_detect.  With a skip mode (VJ_FLAG_SKIP_ROW / _LIST) on
 * either cascade the hand-off goes through the host: vj_detect, then vj_detect_rois on the sub-images.     */
int  vj_detect_chain(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames,
                     int n_frames, const vj_params* p_first, const vj_params* p_second, vj_result* out_first,
                     vj_result* out_second);

/* The same two in the OpenCV arithmetic profile: every cascade vj_detect_opencv runs — stumps, multi-node
 * trees, stage trees, tilted features — as the second one.
 *
 * vj_detect_opencv_rois: the result equals what vj_detect_opencv returns for region i given as a sub-image of its frame,
 * {data + y * stride + x * channels, w, h, stride, on_device, channels} — what an OpenCV caller gets from cvSetImageROI or a
 * sub-image header: rect.frame = i, x / y relative to the region's origin, scale_idx = the factor's index in THAT call's
 * enumeration; with min_neighbors != 0 every region is grouped on its own; counters are the sums over the regions; rectangles sorted
 * by (frame, scale_idx, y, x).  Everything cvHaarDetectObjects derives from the image size comes from the region's w x h
 * (tempcv.cpp:1344-1373, :817-820): the number of factors (factor * win < size - 10), endX / endY, the border rule x + win_w >= w + 1,
 * y + win_h >= h + 1.  Regions too small for any scale contribute nothing; n_rois == 0 is VJ_OK with no rectangles; a region that
 * is not inside its frame or has w <= 0 or h <= 0 is VJ_ERR_ARG.  Which route a call takes, by p->flags:
 *   0, VJ_FLAG_COUNTERS         frames of one size: they are uploaded and integrated ONCE (sum, sqsum, and the tilted integral when
 *                               the cascade has tilted nodes) and all regions of all frames run in ONE region pass on those
 *                               integral images (a rectangle sum does not depend on where the integral image starts; a tilted
 *                               rectangle's four corners give the sum over the same pixels in the frame's tilted integral as in the
 *                               crop's).  Frames of differing sizes: the route below.
 *   VJ_FLAG_CV_SCALE_IMAGE      (with or without VJ_FLAG_COUNTERS; VJ_FLAG_CV_CANNY_PRUNING and VJ_FLAG_CV_ROUGH_SEARCH beside it are not
 *                               read, as in vj_detect_opencv) frames of one size: a resized crop is not a crop of the resized frame,
 *                               so every region gets level images of its own — cvResize of the crop for every level the region's
 *                               w x h takes — but all of them, for all regions of a sub-batch, are written by ONE launch into one
 *                               canvas, integrated once, and walked by one exhaustive-grid pass (a canvas holds a fixed number of
 *                               pixels; regions beyond it start another one; a region too large for an empty canvas takes the
 *                               route below).  Frames of differing sizes, and calls with more than 32 regions per distinct
 *                               region size on average (measured faster there): the route below.
 *   VJ_FLAG_CV_CANNY_PRUNING    } one vj_detect_opencv call per region size on the sub-images: the Canny map of a crop is not the
 *   VJ_FLAG_CV_FIND_BIGGEST     } crop of the Canny map (replicated borders, hysteresis connectivity), and the find-biggest search
 *                               } keeps its state per image (it clears VJ_FLAG_CV_SCALE_IMAGE).
 *   any other bit               the same route (vj_detect_opencv ignores what it does not know).
 * The result is the same either way, by definition.                                                                              */
int  vj_detect_opencv_rois(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                           const vj_cv_params* p, vj_result* out);
/* What the environment's last vj_detect_opencv_rois call did (zeroed when a call begins; a chain call that runs "the two public
 * calls" makes one). */
typedef struct vj_cv_rois_info {
    int32_t  route;               /* 0 no call yet; 1 one pass on the frames' integral images; 2 one pass on level canvases
                                     (VJ_FLAG_CV_SCALE_IMAGE); 3 one vj_detect_opencv call per region size; 4 route 2 with some
                                     regions, too large for a canvas, sent through route 3                                       */
    int32_t  canvases;            /* route 2 / 4: canvases of level images the call made                                          */
    uint32_t canvas_w, canvas_h;  /* ... the size of the largest (by pixels)                                                      */
    uint64_t regions;             /* regions of the call                                                                          */
    uint64_t level_images;        /* route 2 / 4: (region, level) pairs the level loop evaluates (the few without a grid
                                     position included: they have no level image)                                               */
    uint64_t windows;             /* grid positions of the pass (routes 1, 2, 4: of what ran there); 0 on route 3                 */
    float    pyramid_ms;          /* device time of the pyramid launches (events), summed over canvases                          */
    int32_t  reserved;
} vj_cv_rois_info;
int  vj_cv_rois_info_get(const vj_env* e, vj_cv_rois_info* out);   /* a null argument: VJ_ERR_ARG */
/* vj_detect_opencv_chain mirrors vj_detect_chain: out_first is what vj_detect_opencv(first, p_first) returns, and its rectangles are
 * the regions — the raw candidates when p_first->min_neighbors == 0, the grouped objects otherwise; out_second is what
 * vj_detect_opencv_rois(second, those regions, p_second) returns, rect.frame indexing out_first->rects.  Both flag words within
 * VJ_FLAG_COUNTERS: the frames are uploaded and integrated once for both cascades (per sub-batch when the batch is split; with the
 * tilted integral when either cascade has tilted nodes), and `second` runs in the region pass before the sub-batch's images are
 * replaced; the rectangle list travels through the host in between.  Any other flag: the two public calls back to back.
 * With VJ_FLAG_CV_CHAIN_DEVICE in p_first->flags (and both words otherwise within VJ_FLAG_COUNTERS) the list stays on the device:
 * kernels turn the first cascade's records into regions — bucketed by frame, or grouped per frame by the device's groupRectangles
 * when p_first->min_neighbors != 0 — and into the region pass's units, the region pass runs behind them, and the host waits once
 * per sub-batch.  The buffers of that route start at the configured "det_cap" (first-cascade detections and so regions,
 * second-cascade detections, 4 x det_cap units) and grow to what the device counted, the sub-batch being enqueued again; a frame
 * with more candidates to group than "group_max" sends its sub-batch through the host as above.  Same results either way.        */
int  vj_detect_opencv_chain(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames, int n_frames,
                            const vj_cv_params* p_first, const vj_cv_params* p_second, vj_result* out_first, vj_result* out_second);
/* What the environment's last vj_detect_opencv_chain call did, whichever route it took (zeroed when a call begins). */
typedef struct vj_cv_chain_info {
    int32_t  handoff;             /* 0 no call yet; 1 on the device (VJ_FLAG_CV_CHAIN_DEVICE); 2 through the host; 3 the two
                                     public calls back to back (units / windows stay 0: they run no common region pass)          */
    int32_t  sub_batches;         /* sub-batches of the call ...                                                                  */
    int32_t  sub_batches_device;  /* ... and how many of them handed off on the device (the others: more candidates in a frame
                                     than "group_max", redone through the host)                                                   */
    int32_t  reruns;              /* times a sub-batch's chain was enqueued again because a buffer was short                      */
    uint64_t regions;             /* regions handed to the second cascade                                                         */
    uint64_t units;               /* window rows of the region pass: one per (region, factor, row)                                */
    uint64_t windows;             /* grid positions of those rows                                                                 */
    float    handoff_ms;          /* device time of the hand-off kernels (events), summed over sub-batches; 0 on the host routes  */
    int32_t  reserved;
} vj_cv_chain_info;
int  vj_cv_chain_info_get(const vj_env* e, vj_cv_chain_info* out);   /* a null argument: VJ_ERR_ARG */

/* ------------------------------------------------- batches of frames of differing sizes */
/* vj_detect and vj_detect_opencv take frames of ONE size.  These two take frames of any sizes — a folder of photographs, thumbnails,
 * crops from another detector — in one call.  The result is, by definition, the concatenation over i of what
 * vj_detect / vj_detect_opencv returns for frames[i] ALONE with the same parameters: rect.frame = i, x / y in the frame, scale_idx the
 * index in that frame's own enumeration, min_neighbors != 0 groups every frame on its own, counters and timings are sums, the list is
 * sorted by (frame, scale_idx, y, x).  Frames may differ in width, height, stride and channels (1, 3 or 4); host and device-resident
 * frames may be mixed.  A frame too small for any scale contributes nothing; n_frames == 0 is VJ_OK; a frame with null data, w <= 0,
 * h <= 0, another channel count or stride < w * channels is VJ_ERR_ARG, and vj_last_error names the frame.
 * How a call runs: frames are grouped by (w, h, channels).  A group with at least own_call_px pixels in total goes through ONE batched
 * vj_detect / vj_detect_opencv call on the original frames (large or many equal frames run best there).  The gray images of all
 * other frames are written by ONE launch (atlas_pack, vj_atlas.hip) into an atlas — shelf-packed, no gaps but the rounding of slot
 * widths to 4 columns, dimensions from a short ladder so that plans repeat —, the atlas is integrated ONCE as one frame (with the
 * tilted integral when the cascade has tilted nodes) and every frame runs as a region of it in one region pass (what
 * vj_detect_opencv_rois / vj_detect_rois do for one device-resident frame: a rectangle sum does not depend on where the integral
 * image starts).  Frames beyond the atlas's pixel budget, or beyond the configured "max_subbatch" frames, start the next atlas; a
 * frame whose slot exceeds an empty atlas takes a call of its own.  An atlas stays inside the 32-bit offsets of a frame's sum image.
 * Flags whose result needs the image alone send EVERY group through its own batched call, and no atlas is made: VJ_FLAG_SKIP_ROW /
 * VJ_FLAG_SKIP_LIST (clod profile); VJ_FLAG_CV_CANNY_PRUNING without VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_CV_FIND_BIGGEST, and bits
 * vj_detect_opencv does not know (OpenCV profile).  VJ_FLAG_CV_SCALE_IMAGE runs from the atlas on level canvases
 * (vj_detect_opencv_rois' route 2, the atlas as its one device-resident gray frame).  Same result either way.
 * The options are a call argument, not vj_env_configure keys; like those they change speed only, never a result.               */
typedef struct vj_mixed_opts {     /* NULL = defaults */
    uint64_t atlas_px;             /* pixel budget of one atlas: the frame slots it holds, in total (0 = default: 2^24)          */
    uint64_t own_call_px;          /* a group of frames of one (w, h, channels) with at least this many pixels in total gets a
                                      batched call of its own; 0 = default: 2^19 (measured), UINT64_MAX = never */
} vj_mixed_opts;
int  vj_detect_mixed(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_params* p,
                     const vj_mixed_opts* opts, vj_result* out);
int  vj_detect_opencv_mixed(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_cv_params* p,
                            const vj_mixed_opts* opts, vj_result* out);
/* The packing alone, next to vj_grayscale: the first atlas a mixed call with this budget would make of `frames` if none of them took
 * a call of its own (frames in order while the budget and "max_subbatch" hold; frames too large for an empty atlas are passed over),
 * written to the HOST buffer `atlas` (atlas_stride bytes per row).  *atlas_w, *atlas_h: its size; origins_xy[2 i], [2 i + 1]: where
 * frame i's gray image lies, -1 -1 when it is not in this atlas.  A frame's slot is its width rounded up to 4 columns; those pad
 * columns and whatever no slot covers are 0 here (the detect calls never clear them).  atlas == NULL: nothing is packed, only the
 * size and the origins are written — what a caller needs to allocate `atlas`; otherwise atlas_stride >= *atlas_w, or VJ_ERR_ARG.
 * n_frames == 0, or no frame that fits: VJ_OK with a 0 x 0 atlas.                                                               */
int  vj_pack_frames(vj_env* e, const vj_image* frames, int n_frames, uint64_t atlas_px, uint8_t* atlas, int atlas_stride,
                    int* atlas_w, int* atlas_h, int32_t* origins_xy);
/* What the environment's last vj_detect_mixed / vj_detect_opencv_mixed call did (zeroed when a call begins). */
typedef struct vj_mixed_info {
    int32_t  atlases;             /* atlases made ...                                                                              */
    int32_t  own_calls;           /* ... and batched calls on original frames (one per group sent there)                           */
    uint32_t atlas_w, atlas_h;    /* the size of the largest atlas (by pixels)                                                     */
    uint64_t frames;              /* frames of the call                                                                            */
    uint64_t frames_atlas;        /* ... that ran on atlases                                                                       */
    uint64_t frames_own_calls;    /* ... that the own_call_px rule, or a flag, sent through calls of their own                     */
    uint64_t frames_oversized;    /* ... too large for an empty atlas (they take calls of their own too)                          */
    uint64_t windows;             /* grid positions of the atlas passes                                                            */
    float    pack_ms;             /* device time of the pack launches (events), summed over atlases                               */
    int32_t  reserved;
} vj_mixed_info;
int  vj_mixed_info_get(const vj_env* e, vj_mixed_info* out);   /* a null argument: VJ_ERR_ARG */

/* ------------------------------------------------- the front end of a detect call, on the device */
/* What every OpenCV caller of a Haar cascade runs first — cvtColor(BGR2GRAY), resize(INTER_LINEAR) to the detection size,
 * equalizeHist — as ONE batched call, device in, device out.  It adds no arithmetic: out[i] holds, byte for byte,
 * vj_grayscale(frames[i]), then vj_resize_linear to the destination size (the identity when that is the source's size), then, with
 * VJ_PREP_EQUALIZE, vj_equalize_hist — of the RESIZED image: its histogram is the destination's own, total = its width * height.
 * Every frame is processed on its own.  Third-party arithmetic throughout, parity unpinned, like its parts.
 * The records it returns have on_device = 1, so every entry point takes them as they are — also the ones that refuse
 * VJ_FLAG_EQUALIZE_HIST (vj_detect_rois, vj_detect_chain, vj_detect_opencv_rois, vj_detect_opencv_chain, vj_run_windows) and
 * vj_run_windows_opencv, which has no flags; outputs of differing sizes go to vj_detect_mixed / vj_detect_opencv_mixed.  Rectangles
 * come back in the resized frame's coordinates: the caller scales them, as OpenCV's facedetect sample does.
 * Layout of the destination buffer: image i has a row stride of its width rounded up to 4 and starts at a multiple of 256 bytes;
 * the pad columns are written as 0 (and never counted in a histogram).                                                        */
enum { VJ_PREP_EQUALIZE = 1u << 0 };
typedef struct vj_prep {
    int32_t  dst_w, dst_h;   /* both > 0: every frame is resized to this size                                                   */
    double   fx, fy;         /* else both > 0: frame i goes to cvRound(w_i * fx) x cvRound(h_i * fy) (round half to even of the
                                f64 product), at least 1 x 1; else (all four 0): no resize                                      */
    uint32_t flags;          /* VJ_PREP_EQUALIZE                                                                                */
    uint32_t reserved;       /* must be 0                                                                                       */
} vj_prep;
void vj_prep_default(vj_prep* p);                       /* all 0 */
/* Host only, no environment: where each output image lies and how many bytes the buffer needs.  out[i] is what vj_preprocess will
 * return for frame i, with data = (const uint8_t*)offset in the buffer; *bytes is the end of the last image.  Errors as below.  */
int  vj_preprocess_layout(const vj_image* frames, int n_frames, const vj_prep* p, vj_image* out, uint64_t* bytes);
/* frames: host or device-resident, 1 / 3 / 4 channels, any strides, sizes may differ.  d_dst: device memory of at least the layout's
 * `bytes` (dst_bytes says how many there are); all work of the caller's that reads or writes it must be complete before the call
 * (the library's streams are non-blocking, see vj_image.on_device).  out[i]: gray, on_device = 1, data inside d_dst.  Returns after
 * the work is complete.
 * All checks come before the device is used.  VJ_ERR_ARG, with vj_last_error naming the frame or the field: null arguments; a frame
 * with null data, w <= 0, h <= 0, another channel count or stride < w * channels; one of dst_w / dst_h, or of fx / fy, set without
 * the other; negative sizes, negative or non-finite factors; unknown flag bits, reserved != 0; dst_bytes below the layout's bytes;
 * d_dst not a multiple of 4 (device allocations are); a device-resident source that overlaps [d_dst, d_dst + bytes).  VJ_ERR_LIMIT: a source or destination side above 65535 (the taps'
 * 16-bit indices), or more work units than a 32-bit index holds.  n_frames == 0 is VJ_OK.  Calls of more frames than the configured
 * "max_subbatch" run in slices.                                                                                                 */
int  vj_preprocess(vj_env* e, const vj_image* frames, int n_frames, const vj_prep* p, uint8_t* d_dst, uint64_t dst_bytes,
                   vj_image* out);
/* Device time of the environment's last vj_preprocess call: events around its copies and launches, in ms.  A null argument: VJ_ERR_ARG. */
int  vj_preprocess_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- rectangles back into pixels, on the device */
/* What every consumer of a detector does next — cut the boxes out of the frames and bring them to one fixed size — as ONE batched
 * call, device in, device out.  It adds no arithmetic: the resize is vj_resize_linear's, per channel (the 2 x 2
 * mean where the crop is exactly twice the output on both axes, the identity where the sizes are equal); parity unpinned at the
 * OpenCV boundary, like vj_preprocess.  For region k = (frame, x, y, w, h):
 *   1. the sample's mapping to source pixels: x0 = cvRound(x * sx), y0 = cvRound(y * sy), w0 = max(cvRound(w * sx), 1),
 *      h0 = max(cvRound(h * sy), 1) (round half to even of the f64 product), then mx = cvRound(w0 * margin), my = cvRound(h0 * margin)
 *      and the source region (x0 - mx, y0 - my, w0 + 2 mx, h0 + 2 my);
 *   2. a virtual crop with replicated border: crop[i][j] = frame[clamp(y0 - my + i, 0, H - 1)][clamp(x0 - mx + j, 0, W - 1)], so a
 *      region is never clipped (a box keeps its aspect) and one partly or wholly outside its frame is defined;
 *   3. out[k] = cv::resize(crop, (out_w, out_h), INTER_LINEAR) per channel: the taps clamp at the CROP's edges, not the frame's.
 * Channels: without flags all frames the regions name share a channel count, which is C (BGRA's alpha is resized like any
 * channel); VJ_EXTRACT_GRAY gives C = 1, colour sources going through the ingest BGR2GRAY tap by tap and then the resize — the
 * order of vj_preprocess, so a whole-frame region with this flag and no margin is vj_preprocess without equalization, byte for
 * byte.  Layout of the destination: n_regions x out_h x out_w x C bytes, interleaved like a cv::Mat; VJ_EXTRACT_PLANAR gives
 * n_regions x C x out_h x out_w (an NCHW batch).        No padding anywhere.                                                      */
enum { VJ_EXTRACT_GRAY = 1u << 0, VJ_EXTRACT_PLANAR = 1u << 1 };
typedef struct vj_extract_params {
    int32_t  out_w, out_h;   /* both > 0: the size of every output                                                              */
    double   sx, sy;         /* the regions' coordinates times these are source pixels; 0 means 1                               */
    double   margin;         /* the mapped region grows by cvRound(side * margin) on each of its four sides                     */
    uint32_t flags;          /* VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR                                                              */
    uint32_t reserved;       /* must be 0                                                                                       */
} vj_extract_params;
void vj_extract_default(vj_extract_params* p);          /* sx = sy = 1, margin = 0, sizes 0: the caller must set them */
/* Host only, no environment: src_regions[k] is the mapped source region of region k (it may lie outside its frame), *channels is
 * C and *bytes the size of the output.  Errors as below.                                                                        */
int  vj_extract_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                       vj_roi* src_regions, int* channels, uint64_t* bytes);
/* frames: host or device-resident, 1 / 3 / 4 channels, any strides, sizes may differ.  d_dst: device memory of at least the
 * layout's `bytes` (dst_bytes says how many there are), at any address; all work of the caller's that reads or writes it must be
 * complete before the call (the library's streams are non-blocking, see vj_image.on_device).  Returns after the work is complete.  All checks come
 * before the device is used.  VJ_ERR_ARG, with vj_last_error naming the row or the field: null arguments; a frame that breaks
 * vj_detect_mixed's rules; a region's frame index out of range, w <= 0 or h <= 0; out_w or out_h <= 0; negative or non-finite sx, sy
 * or margin; unknown flag bits, reserved != 0; frames of differing channel counts without VJ_EXTRACT_GRAY; dst_bytes below the
 * layout's bytes; a device-resident source that overlaps [d_dst, d_dst + bytes).  VJ_ERR_LIMIT: an output side or a mapped region
 * side above 65535 (the taps' 16-bit indices), a mapped coordinate beyond +-2^24, or more work units than a 32-bit index holds.
 * n_regions == 0 is VJ_OK.  With "max_subbatch" configured a call runs in slices of regions that name at most that many frames.  */
int  vj_extract(vj_env* e, const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions,
                const vj_extract_params* p, uint8_t* d_dst, uint64_t dst_bytes);
/* Device time of the environment's last vj_extract call: events around its copies and launches, in ms.  A null argument: VJ_ERR_ARG. */
int  vj_extract_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- aligned crops: one affine warp per region, on the device */
/* What a recognition or landmark network is fed: regions rotated and scaled so the eyes sit at fixed places — or, with one affine
 * per frame and the frame's size as the output, whole frames rotated — as ONE batched call, device in, device out.
 * The arithmetic is laid out after the 8-bit INTER_LINEAR path of cv::warpAffine(..., WARP_INVERSE_MAP, BORDER_REPLICATE); parity
 * is unpinned at the OpenCV boundary, the definition here and in DESIGN.md 4.19 is authoritative.  For affine k = (frame, m[6]) the
 * matrix maps OUTPUT pixel (x, y) to a source pixel, in f64, pixel coordinates used directly (no half-pixel offset: a scaling
 * matrix is NOT vj_extract's resize — vj_affine_from_rect adds the offset that aligns the pixel centres):
 *   src_x = m0 x + m1 y + m2,   src_y = m3 x + m4 y + m5
 * With rne(v) = cvRound(v), round half to even of an f64 to int32, and no contraction anywhere:
 *   ax[x] = rne((m0 * x) * 1024.0)               bx[x] = rne((m3 * x) * 1024.0)
 *   X0[y] = rne((m1 * y + m2) * 1024.0) + 16     Y0[y] = rne((m4 * y + m5) * 1024.0) + 16
 *   X = (X0[y] + ax[x]) >> 5, Y = (Y0[y] + bx[x]) >> 5 (arithmetic shifts of int32);  sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31
 *   w00 = (32 - fx)(32 - fy) 32, w01 = fx (32 - fy) 32, w10 = (32 - fx) fy 32, w11 = fx fy 32        (they sum to 32768)
 *   p_ij = frame[clamp(sy + i, 0, H - 1)][clamp(sx + j, 0, W - 1)] per channel: the border is replicated, nothing is clipped, a
 *   region wholly outside its frame is defined;   out = (p00 w00 + p01 w01 + p10 w10 + p11 w11 + 16384) >> 15
 * Channels and layout are vj_extract's: all named frames share a channel count C; VJ_EXTRACT_GRAY takes the four taps through the
 * ingest BGR2GRAY first, then blends them, C = 1; the output is dense n x out_h x out_w x C, VJ_EXTRACT_PLANAR n x C x out_h x out_w. */
typedef struct vj_affine { int32_t frame; int32_t reserved; double m[6]; } vj_affine;   /* reserved must be 0 */
typedef struct vj_affine_params {
    int32_t  out_w, out_h;   /* both > 0: the size of every output                                                              */
    uint32_t flags;          /* VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR                                                              */
    uint32_t reserved;       /* must be 0                                                                                       */
} vj_affine_params;
void vj_affine_default(vj_affine_params* p);            /* all 0: the caller must set the sizes */
/* Host only, no environment: *channels is C and *bytes the size of the output.  Errors as vj_extract_affine's.                  */
int  vj_extract_affine_layout(const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                              int* channels, uint64_t* bytes);
/* frames and d_dst: as vj_extract.  Returns after the work is complete.  All checks come before the device is used.  VJ_ERR_ARG,
 * with vj_last_error naming the row and the field: null arguments; a frame that breaks vj_detect_mixed's rules; an affine's frame
 * index out of range, reserved != 0 or a non-finite matrix entry; out_w or out_h <= 0; unknown flag bits, reserved != 0; frames of
 * differing channel counts without VJ_EXTRACT_GRAY; dst_bytes below the layout's bytes; a device-resident source that overlaps
 * [d_dst, d_dst + bytes).  VJ_ERR_LIMIT: an output side above 65535; more work units than a 32-bit index holds; any of
 * |m0| (out_w - 1), |m3| (out_w - 1), |m1 y + m2|, |m4 y + m5| at y in {0, out_h - 1} above 2^19 (under that bound no rne saturates
 * and X0 + ax stays inside int32).  n == 0 is VJ_OK.  With "max_subbatch" configured a call runs in slices like vj_extract's.     */
int  vj_extract_affine(vj_env* e, const vj_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                       uint8_t* d_dst, uint64_t dst_bytes);
/* Device time of the environment's last vj_extract_affine call: events around its copies and launches, in ms.  A null argument: VJ_ERR_ARG. */
int  vj_extract_affine_timing(const vj_env* e, float* ms);
/* Host only.  The box (x, y, w, h) scaled to the output with pixel centres aligned:
 *   m = {w / out_w, 0, x + 0.5 * w / out_w - 0.5, 0, h / out_h, y + 0.5 * h / out_h - 0.5}
 * VJ_ERR_ARG: null m, non-finite input, w <= 0, h <= 0, out_w <= 0 or out_h <= 0.                                                */
int  vj_affine_from_rect(double x, double y, double w, double h, int out_w, int out_h, double m[6]);
/* Host only.  The similarity that puts the left eye (lx, ly) at output pixel (ex_l * out_w, ey * out_h) and the right eye (rx, ry)
 * at (ex_r * out_w, ey * out_h).  With d = (ex_r - ex_l) * out_w, a = (rx - lx) / d, b = (ry - ly) / d, cxl = ex_l * out_w,
 * cy = ey * out_h, in exactly this order of f64 operations:
 *   m = {a, -b, lx - a * cxl + b * cy, b, a, ly - b * cxl - a * cy}
 * VJ_ERR_ARG: null m, non-finite input, out_w <= 0 or out_h <= 0, ex_r <= ex_l, or coincident eyes.                              */
int  vj_affine_from_eyes(double lx, double ly, double rx, double ry, int out_w, int out_h, double ex_l, double ex_r, double ey,
                         double m[6]);

/* ------------------------------------------------- rectangles painted into the frames, on the device */
/* The other consumers of a detector's rectangles write into the frames themselves: redaction (every face blurred or pixelated
 * before a video is stored or shown) and the reference sample's own last step, cvRectangle around every result (main.cpp:155,
 * :181) — as ONE batched call that changes the pixels inside, or around, the rectangles IN PLACE.  This is the
 * only entry point that writes through vj_image.data.  All arithmetic is on integers; parity is unpinned at the OpenCV boundary,
 * the definition here and in DESIGN.md 4.20 is authoritative.  For region k = (frame, x, y, w, h):
 *   1. M = (X0, Y0, Wm, Hm): step 1 of vj_extract (cvRound of the coordinates times sx, sy, then the margin), the same limits.
 *      K = M ∩ frame = [cx0, cx1) x [cy0, cy1).  A region whose K is empty paints nothing and is no error.
 *   2. s = size when size > 0, else max(cvRound(min(Wm, Hm) * rel), 1).  OUTLINE: the thickness t = s.  PIXELATE: the cell side s.
 *      BLUR: the kernel side kk = max(s | 1, 3), r = kk >> 1.  FILL ignores it.
 *   3. The shape: M; with VJ_PAINT_ELLIPSE the ellipse inscribed in M: pixel (px, py) of M is in it iff
 *      (2 (px - X0) + 1 - Wm)^2 Hm^2 + (2 (py - Y0) + 1 - Hm)^2 Wm^2 <= Wm^2 Hm^2, in 64-bit integers.
 *   4. The painted set P_k.  FILL, PIXELATE, BLUR: shape ∩ K.  OUTLINE: the shape of M minus the shape of M shrunk by t on each
 *      of its four sides, ∩ K; a shrunk rectangle with a side <= 0: the whole shape.  The outline follows M, not K: a box that
 *      leaves the frame draws no line along the frame's edge.
 *   5. The value, per channel c (alpha like any other); F is the frame AS IT WAS BEFORE THE CALL.  FILL, OUTLINE: color[c].
 *      PIXELATE: cells anchored at (cx0, cy0), cell (i, j) = [cx0 + i s, min(cx0 + (i + 1) s, cx1)) x [cy0 + j s, min(cy0 + (j + 1) s, cy1));
 *      every pixel of a cell takes (sum of F over the cell + n / 2) / n, n the cell's pixel count, the divisions flooring.
 *      BLUR: (sum over dy, dx in -r .. r of F[clamp(py + dy, cy0, cy1 - 1)][clamp(px + dx, cx0, cx1 - 1)][c] + kk^2 / 2) / kk^2,
 *      flooring: the border is replicated at the edge of K, as cv::blur on the ROI does, so a region reads only its own pixels.
 *   6. A pixel in several painted sets of one frame takes the value of the HIGHEST-INDEX region among them — as if the regions
 *      were painted in order, but every value comes from the original frame, never from another region's output.  Bytes in no
 *      painted set are never written; there is no gray conversion.                                                              */
enum { VJ_PAINT_FILL = 0, VJ_PAINT_OUTLINE = 1, VJ_PAINT_PIXELATE = 2, VJ_PAINT_BLUR = 3 };   /* vj_paint_params.mode  */
enum { VJ_PAINT_ELLIPSE = 1u << 0 };                                                           /* vj_paint_params.flags */
typedef struct vj_paint_params {
    int32_t  mode;
    uint32_t flags;
    double   sx, sy, margin;   /* the mapping of vj_extract_params: 0 means 1 for sx, sy                                        */
    int32_t  size;             /* pixels; 0: take it from rel                                                                    */
    double   rel;              /* fraction of the mapped region's shorter side                                                   */
    uint8_t  color[4];         /* FILL, OUTLINE: channel c of a frame takes color[c]; gray frames: color[0]                      */
    uint32_t reserved;         /* must be 0                                                                                      */
} vj_paint_params;
void vj_paint_default(vj_paint_params* p);   /* mode BLUR, sx = sy = 1, margin 0, size 0, rel 0.25, color 0 */
/* Host only, no environment: clipped[k] is K of region k (w = h = 0 when it is empty), sizes[k] its t, s or kk (0 for FILL) and
 * *scratch_bytes what the phase between reading and writing the frames keeps of the call run as one slice (its largest): per
 * region with a K, rounded up to 16 bytes — BLUR: 2 bytes per byte of K; PIXELATE: one byte per cell and channel.  Errors as
 * vj_paint's.                                                                                                                   */
int  vj_paint_layout(const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                     vj_roi* clipped, int32_t* sizes, uint64_t* scratch_bytes);
/* frames: vj_detect_mixed's rules — host or device-resident, 1 / 3 / 4 channels, any strides, sizes may differ — and the call
 * WRITES through vj_image.data: nothing else may read or write the frames until it returns, and all work of the caller's on
 * device-resident frames must be complete before it (see vj_image.on_device).  Device frames: only the bytes of painted pixels are
 * stored.  Host frames: the painted pixels change; other bytes of K's span of a touched row may be rewritten with their own
 * values; a row's padding and rows outside K are never written.  Returns after the work is complete.
 * All checks come before the device is used.  VJ_ERR_ARG, with vj_last_error naming the row or the field: the null, frame and
 * region errors of vj_extract; an unknown mode, unknown flag bits, reserved != 0, size < 0; negative or non-finite sx, sy, margin;
 * size == 0 with a rel that is not finite or <= 0; two frames of the call whose memory overlaps (ownership is decided per frame).
 * VJ_ERR_LIMIT: vj_extract's mapping limits; a mapped side above 32767 (the ellipse's products stay below 2^60); BLUR with
 * kk > 255 (a column sum fits 16 bits); PIXELATE with s > 4096 (a cell sum fits 32 bits); more work units than a 32-bit index
 * holds.  VJ_ERR_NOMEM names the bytes.  n_regions == 0 is VJ_OK.  With "max_subbatch" configured a call runs in slices of whole
 * frames, at most that many each.                                                                                               */
int  vj_paint(vj_env* e, const vj_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p);
/* Device time of the environment's last vj_paint call: events around its copies and launches, in ms.  A null argument: VJ_ERR_ARG. */
int  vj_paint_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- decoder frames: NV12 / NV21 / I420 to BGR and back, on the device */
/* Hardware decoders write 4:2:0 YCbCr and encoders read it; vj_extract and vj_paint work on interleaved BGR.  These two batched
 * calls close the loop on the device:
 *   decoder -> vj_yuv_luma -> vj_preprocess / detect -> vj_yuv_to_bgr -> vj_extract / vj_paint -> vj_bgr_to_yuv -> encoder.
 * (vj_paint_yuv and vj_extract_yuv / vj_extract_affine_yuv below do the painting and the cropping on the 4:2:0 frames directly.)
 * The arithmetic is OpenCV imgproc's 8-bit fixed-point BT.601 limited-range pair, cvtColor(COLOR_YUV2BGR_NV12 / _NV21 / _I420) and
 * cvtColor(COLOR_BGR2YUV_I420); parity is unpinned at the OpenCV boundary, the definition here and in DESIGN.md 4.21 is
 * authoritative.  All values are int32, >> is the arithmetic (flooring) shift, sat(t) = min(max(t, 0), 255), H = 1 << 19.
 * Decode: pixel (x, y) takes Y = luma[y][x] and the chroma sample (x >> 1, y >> 1) — nearest, no interpolation:
 *     yy = max(Y - 16, 0) * 1220542;  u = U - 128;  v = V - 128
 *     B = sat((yy + H + 2116026 * u) >> 20)
 *     G = sat((yy + H -  852492 * v - 409993 * u) >> 20)
 *     R = sat((yy + H + 1673527 * v) >> 20)
 *   and with four output channels alpha = 255.
 * Encode (alpha, if present, is ignored): for every pixel
 *     Y = (269484 R + 528482 G + 102760 B + H + (16 << 20)) >> 20
 *   and from the TOP-LEFT pixel of each 2 x 2 block (even x, even y; no averaging)
 *     U = (-155188 R - 305135 G + 460324 B + H + (128 << 20)) >> 20
 *     V = ( 460324 R - 385875 G -  74448 B + H + (128 << 20)) >> 20
 *   No clamp is needed: the outputs span 16 .. 240.
 * Layouts: NV12 — a Y plane and one plane of interleaved U, V byte pairs at half resolution; NV21 — the same with pairs V, U;
 * I420 — three planes Y, U, V, the chroma planes w/2 x h/2.  Every plane has its own pointer; width and height are even.      */
enum { VJ_YUV_NV12 = 0, VJ_YUV_NV21 = 1, VJ_YUV_I420 = 2 };   /* vj_yuv_image.layout                                           */
enum { VJ_YUV_RGB_ORDER = 1u << 0 };                          /* vj_yuv_params.flags: the BGR side is RGB / RGBA (R and B swapped) */
typedef struct vj_yuv_image {
    const uint8_t* y;          /* the Y plane: height rows of width bytes, y_stride bytes apart.  The planes are read only by every
                                  entry point but vj_paint_yuv, which WRITES the painted samples through all three pointers (the
                                  memory must be writable)                                                                       */
    const uint8_t* c0;         /* NV12 / NV21: the pair plane, height / 2 rows of width bytes; I420: the U plane, height / 2 rows
                                  of width / 2 bytes.  Rows c_stride bytes apart                                                 */
    const uint8_t* c1;         /* I420: the V plane (c_stride too); NV12 / NV21: ignored                                         */
    int32_t width, height;     /* even, 2 .. 65534                                                                               */
    int32_t y_stride, c_stride;
    int32_t layout;            /* VJ_YUV_NV12 / _NV21 / _I420                                                                    */
    int32_t on_device;         /* as vj_image.on_device, for all planes of the frame                                            */
} vj_yuv_image;
typedef struct vj_yuv_params {
    int32_t  channels;         /* of the BGR side: 3, or 4 (BGRA)                                                               */
    uint32_t flags;            /* VJ_YUV_RGB_ORDER                                                                               */
    uint32_t reserved;         /* must be 0                                                                                      */
} vj_yuv_params;
void vj_yuv_default(vj_yuv_params* p);   /* channels 3, flags 0 */
/* Host only, no environment: where each BGR image lies and how many bytes the buffer needs.  out[i] is what vj_yuv_to_bgr will
 * return for frame i, with data = (const uint8_t*)offset in the buffer.  The layout is vj_preprocess's: a row pitch of
 * width * channels rounded up to 4, every image at a multiple of 256 bytes; *bytes is the end of the last image.              */
int  vj_yuv_to_bgr_layout(const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, vj_image* out, uint64_t* bytes);
/* frames: host or device-resident, any strides, any addresses, sizes may differ.  d_dst: device memory of at least the layout's
 * bytes, as vj_preprocess's.  out[i]: on_device = 1, channels = p->channels, data inside d_dst — every entry point, vj_paint
 * included, takes them as they are.  The pad bytes inside the pitch are written as 0.  Returns after the work is complete.
 * All checks come before the device is used.  VJ_ERR_ARG, with vj_last_error naming the frame or the field: null arguments; a null
 * plane that the layout needs; odd or non-positive sizes; a stride below the plane's row bytes; an unknown layout; unknown flag
 * bits, reserved != 0; channels not 3 or 4; dst_bytes below the layout's bytes; d_dst not a multiple of 4; a device-resident
 * source plane that overlaps [d_dst, d_dst + bytes).  VJ_ERR_LIMIT: a side above 65534; more work units than a 32-bit index holds.
 * n_frames == 0 is VJ_OK.  Calls of more frames than the configured "max_subbatch" run in slices.                               */
int  vj_yuv_to_bgr(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_yuv_params* p, uint8_t* d_dst, uint64_t dst_bytes,
                   vj_image* out);
/* Host only: where each output frame lies.  A frame is STACKED: its Y plane at a pitch of width rounded up to 4, its chroma right
 * below — NV12 / NV21: height / 2 rows of pairs at the same pitch; I420: the U plane, then the V plane, height / 2 rows each at a
 * pitch of width / 2 rounded up to 4.  Every plane is 4-byte aligned, every frame starts at a multiple of 256 bytes, pad bytes
 * are written as 0.  out[i]: y, c0, c1 = offsets in the buffer (c1 = 0 for NV12 / NV21), y_stride, c_stride = the pitches.    */
int  vj_bgr_to_yuv_layout(const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, vj_yuv_image* out,
                          uint64_t* bytes);
/* frames: vj_detect_mixed's rules, with 3 or 4 channels (p->channels is not looked at: every frame says its own; a gray frame is
 * VJ_ERR_ARG) and even sizes.  Otherwise as vj_yuv_to_bgr, errors included.  out[i]: on_device = 1, pointers inside d_dst.     */
int  vj_bgr_to_yuv(vj_env* e, const vj_image* frames, int n_frames, const vj_yuv_params* p, int layout, uint8_t* d_dst,
                   uint64_t dst_bytes, vj_yuv_image* out);
/* Host only: the Y plane of a frame as a gray vj_image — what cvtColor(COLOR_YUV2GRAY_NV12) returns; vj_preprocess and every
 * detect call take it.  VJ_ERR_ARG: null arguments, a null Y plane, non-positive sizes, y_stride < width.                       */
int  vj_yuv_luma(const vj_yuv_image* frame, vj_image* out);
/* Device time of the environment's last vj_yuv_to_bgr or vj_bgr_to_yuv call: events around its copies and launches, in ms.      */
int  vj_yuv_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- rectangles painted into 4:2:0 frames where they lie, on the device */
/* Redaction between a decoder and an encoder: vj_paint on the BGR copy re-quantizes the whole picture on the way back
 * (vj_bgr_to_yuv of vj_yuv_to_bgr is not the identity) and needs a copy twice the frames' size.  vj_paint_yuv paints the rectangles
 * into NV12 / NV21 / I420 frames IN PLACE, as ONE batched call; parity is unpinned, the definition here and in
 * DESIGN.md 4.23 is authoritative.  regions are in LUMA pixels; p is vj_paint's struct: the same modes, VJ_PAINT_ELLIPSE, sx, sy,
 * margin, size, rel.
 *   Colour.  FILL, OUTLINE: color[0..2] are B, G, R, color[3] is ignored; the host converts them once with the encode formulas
 *     above to (Yc, Uc, Vc).
 *   Luma.  The Y plane after the call is exactly what vj_paint (items 1 to 6 above) makes of it as a one-channel frame with
 *     color[0] = Yc.  M, K = [cx0, cx1) x [cy0, cy1), s, the shape and the painted set P_k are that definition's.
 *   Chroma.  The chroma image is W/2 x H/2 with two components, U and V — interleaved in either order (NV12 / NV21) or two planes
 *     (I420); both are treated alike.  For region k with a non-empty K:
 *     - Kc = [cx0 >> 1, (cx1 + 1) >> 1) x [cy0 >> 1, (cy1 + 1) >> 1): the chroma samples that K touches.
 *     - The painted chroma set Pc_k: sample (u, v) of Kc is in it iff at least one of the four luma pixels (2u + a, 2v + b),
 *       a, b in {0, 1}, is in P_k — "any of four", so that no painted luma pixel keeps its original chroma.  The price: a luma pixel
 *       just outside K (or outside the ellipse, or inside the outline) may keep its Y and take new chroma.
 *     - Sizes: PIXELATE sc = (s + 1) >> 1; BLUR kkc = max((kk >> 1) | 1, 3), rc = kkc >> 1.
 *     - Values, from the chroma image AS IT WAS BEFORE THE CALL, per component: FILL, OUTLINE: Uc, Vc.  PIXELATE, BLUR: item 5 of
 *       vj_paint with Kc for K, sc for s and kkc for kk: cells anchored at Kc's corner and clipped to Kc, taps clamped to Kc, the
 *       same rounding and flooring.  A region reads only chroma samples of its own Kc.
 *     - A chroma sample in several Pc_k of one frame takes the value of the HIGHEST-INDEX region among them.  Two regions whose K
 *       are disjoint can share a chroma sample (x ranges [2, 7) and [7, 12) share sample 3): overlap is decided on Kc, not on K.
 *   Bytes of chroma samples in no Pc_k, and luma bytes in no P_k, are never written on device frames.                             */
/* Host only, no environment: clipped[k] is K of region k and chroma[k] its Kc, in chroma samples (w = h = 0 when K is empty);
 * sizes[k] its t, s or kk (0 for FILL) and chroma_sizes[k] its t, sc or kkc; *scratch_bytes what the phase between reading and
 * writing the planes keeps of the call run as one slice: per region with a K, vj_paint_layout's bytes of the Y plane (one channel,
 * K, the luma size) plus twice those of one chroma component (one channel, Kc, the chroma size), each rounded up to 16.  Errors as
 * vj_paint_yuv's.                                                                                                                */
int  vj_paint_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p,
                         vj_roi* clipped, vj_roi* chroma, int32_t* sizes, int32_t* chroma_sizes, uint64_t* scratch_bytes);
/* frames: as vj_yuv_to_bgr takes them — host or device-resident, any strides, any addresses, sizes and layouts may differ — and
 * the call WRITES through the planes' pointers: nothing else may read or write the frames until it returns, and all work of the
 * caller's on device-resident frames must be complete before it.  Device frames: only the bytes of painted samples are stored.
 * Host frames, per plane as vj_paint's host frames: the painted samples change; other bytes of the rectangle's span (K, Kc) of a
 * touched row may be rewritten with their own values; a row's padding and rows outside the rectangle are never written.  Returns
 * after the work is complete.
 * All checks come before the device is used.  VJ_ERR_ARG, with vj_last_error naming the frame, the row or the field: null
 * arguments; the frame errors of vj_yuv_to_bgr (a null plane that the layout needs, odd or non-positive sizes, a stride below the
 * plane's row bytes, an unknown layout); the region and parameter errors of vj_paint; any two planes of the call whose byte
 * extents overlap, planes of the same frame included.  VJ_ERR_LIMIT: vj_paint's limits; a side above 65534.  VJ_ERR_NOMEM names the
 * bytes.  n_regions == 0 is VJ_OK; a region whose K is empty paints nothing.  With "max_subbatch" configured a call runs in slices
 * of whole frames, at most that many each.                                                                                       */
int  vj_paint_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_paint_params* p);
/* Device time of the environment's last vj_paint_yuv call: events around its copies and launches, in ms.  A null argument: VJ_ERR_ARG. */
int  vj_paint_yuv_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- crops cut straight out of 4:2:0 frames, on the device */
/* Colour crops for a network without the BGR copy of the whole batch.  ONE sentence defines both calls:
 *   vj_extract_yuv(env, frames, n_frames, regions, n_regions, p, yp, d_dst, dst_bytes) writes exactly the bytes that vj_extract
 *   writes for the same `regions` and `p` when its frames are what vj_yuv_to_bgr(frames, yp) returns.
 *   vj_extract_affine_yuv(env, frames, n_frames, affines, n, p, yp, d_dst, dst_bytes) relates to vj_extract_affine in the same way.
 * Nothing new is stated: the arithmetic is the decode above, then vj_extract's or vj_extract_affine's steps on the decoded bytes;
 * parity stays unpinned at the OpenCV boundary, as for those.  Spelled out:
 *   - frames: as vj_yuv_to_bgr takes them — NV12, NV21, I420, host or device-resident, any strides, any addresses, sizes and
 *     layouts may differ within a call.  regions and the affines' source coordinates are in LUMA pixels.
 *   - p is vj_extract's / vj_extract_affine's struct; yp is vj_yuv_to_bgr's: channels 3 or 4 and VJ_YUV_RGB_ORDER.
 *   - A tap at the clamped source pixel (cx, cy) is decode(Y[cy][cx], U[cy >> 1][cx >> 1], V[cy >> 1][cx >> 1]), through sat, with
 *     alpha 255 when channels = 4.  The crop-edge clamp (vj_extract's steps 2 and 3) and the frame clamp act on the luma
 *     coordinate; the chroma sample follows from the clamped coordinate.
 *   - DECODE FIRST, then the resize per channel on the decoded bytes (the 2 x 2 mean, the bilinear integer arithmetic or the
 *     copy), or vj_extract_affine's blend.  Blending Y, U and V and decoding afterwards is a different function.
 *   - VJ_EXTRACT_GRAY is the composition too: the ingest BGR2GRAY of each decoded tap (its three bytes in the order yp gives
 *     them), then the blend, C = 1.  Crops of the Y plane itself are vj_extract on vj_yuv_luma's images, which differ in range.
 *   - C = 1 with VJ_EXTRACT_GRAY, else yp->channels; VJ_EXTRACT_PLANAR and the dense layout are vj_extract's; d_dst at any address. */
/* Host only, no environment: as vj_extract_layout / vj_extract_affine_layout.  Errors as below.                                 */
int  vj_extract_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions, const vj_extract_params* p,
                           const vj_yuv_params* yp, vj_roi* src_regions, int* channels, uint64_t* bytes);
int  vj_extract_affine_yuv_layout(const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n, const vj_affine_params* p,
                                  const vj_yuv_params* yp, int* channels, uint64_t* bytes);
/* d_dst: as vj_extract.  Return after the work is complete.  All checks come before the device is used.  VJ_ERR_ARG, with
 * vj_last_error naming the frame, the row or the field: null arguments (yp included); the frame errors of vj_yuv_to_bgr (a null
 * plane that the layout needs, odd or non-positive sizes, a stride below the plane's row bytes, an unknown layout); yp->channels
 * not 3 or 4, unknown flag bits or reserved != 0 in yp; the region, affine and parameter errors of vj_extract / vj_extract_affine;
 * dst_bytes below the layout's bytes; a device-resident source plane that overlaps [d_dst, d_dst + bytes).  VJ_ERR_LIMIT: a frame
 * side above 65534; the mapping and output limits of vj_extract / vj_extract_affine.  n == 0 is VJ_OK.  With "max_subbatch"
 * configured a call runs in slices of regions that name at most that many frames, like vj_extract's.                            */
int  vj_extract_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_roi* regions, int n_regions,
                    const vj_extract_params* p, const vj_yuv_params* yp, uint8_t* d_dst, uint64_t dst_bytes);
int  vj_extract_affine_yuv(vj_env* e, const vj_yuv_image* frames, int n_frames, const vj_affine* affines, int n,
                           const vj_affine_params* p, const vj_yuv_params* yp, uint8_t* d_dst, uint64_t dst_bytes);
/* Device time of the environment's last vj_extract_yuv or vj_extract_affine_yuv call: events around its copies and launches, in
 * ms.  A null argument: VJ_ERR_ARG.                                                                                             */
int  vj_extract_yuv_timing(const vj_env* e, float* ms);

/* ------------------------------------------------- boxes carried from frame to frame, on the device */
/* A cascade drops a face for a frame or two; every video pipeline bridges that by looking for the box of frame f in frame f +- 1.
 * vj_track is that search as ONE batched call: block matching of fixed-size gray patches, integer arithmetic only (DESIGN.md
 * 4.22); parity unpinned, like the other stages around the detector.  For row k = (src_frame, dst_frame, x, y, w, h), with
 * t = tmpl and r = radius:
 *   1. T is what vj_extract writes for region (src_frame, x, y, w, h) with out_w = out_h = t, the call's sx, sy, margin = 0 and
 *      VJ_EXTRACT_GRAY: a t x t gray patch;
 *   2. S is what vj_extract writes for region (dst_frame, x, y, w, h) with out_w = out_h = t + 2 r, the same sx, sy,
 *      margin = (double)r / t and VJ_EXTRACT_GRAY: the same box grown by the search radius, at (nearly) the same pixel size.
 *      (X, Y, Wm, Hm) is its mapped source region, (x0, y0, w0, h0) the mapped region without margin.  The call adds no
 *      resampling arithmetic of its own: the replicated border, the crop-edge taps and the BGR2GRAY order are vj_extract's;
 *   3. for dy, dx in -r .. r: sad(dx, dy) = sum over i, j < t of |T[i][j] - S[i + r + dy][j + r + dx]|, integers of at most
 *      64 * 64 * 255 = 1 044 480;
 *   4. the best displacement has the smallest tuple (sad, dx * dx + dy * dy, dy, dx), compared lexicographically: on equal sums the
 *      shorter move wins, then the smaller dy, then the smaller dx — a flat patch stays where it is.  sad0 = sad(0, 0);
 *   5. the output box: x = x0 + cvRound(dx * (double)Wm / (t + 2 r)), y = y0 + cvRound(dy * (double)Hm / (t + 2 r)), w = w0,
 *      h = h0 (cvRound: round half to even of the f64 value, as everywhere else).
 * The two frames of a row may differ in size, stride, channel count and residency; a row may name the same frame twice.         */
typedef struct vj_track_row { int32_t src_frame, dst_frame, x, y, w, h; } vj_track_row;
typedef struct vj_track_params {
    int32_t  tmpl;      /* t: side of the template in patch pixels; a multiple of 4 in 8 .. 64                                */
    int32_t  radius;    /* r: displacements -r .. r on both axes, in patch pixels; 1 .. 16                                    */
    double   sx, sy;    /* vj_extract_params' mapping; 0 means 1                                                               */
    uint32_t flags;     /* none yet: must be 0                                                                                 */
    uint32_t reserved;  /* must be 0                                                                                           */
} vj_track_params;
typedef struct vj_track_result {
    int32_t  dx, dy;        /* the best displacement, patch pixels                                                             */
    uint32_t sad, sad0;     /* its sum of absolute differences, and the one at (0, 0)                                          */
    int32_t  x, y, w, h;    /* the box in dst_frame, in SOURCE pixels (what vj_paint takes with sx = sy = 1)                    */
} vj_track_result;
void vj_track_default(vj_track_params* p);                 /* tmpl 32, radius 8, the rest 0 */
/* Host only, no environment: tmpl_regions[k] = (src_frame, x0, y0, w0, h0) and search_regions[k] = (dst_frame, X, Y, Wm, Hm), the
 * mapped source regions of T and S (they may lie outside their frames); *scratch_bytes the device scratch of the call run as one
 * slice: n_rows * t * t bytes of templates, then n_rows search patches of (t + 2 r)^2 bytes, each at a multiple of 16 bytes.
 * Errors as below.                                                                                                            */
int  vj_track_layout(const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows, const vj_track_params* p,
                     vj_roi* tmpl_regions, vj_roi* search_regions, uint64_t* scratch_bytes);
/* frames: as vj_extract (host or device-resident, 1 / 3 / 4 channels, any strides, sizes may differ; work of the caller's on
 * device-resident frames must be complete).  out: n_rows records in HOST memory.  Returns after the work is complete.  All checks
 * come before the device is used.  VJ_ERR_ARG, with vj_last_error naming the row or the field: the null, frame and region errors of
 * vj_extract; src_frame or dst_frame out of range; tmpl not a multiple of 4 or outside 8 .. 64; radius outside 1 .. 16; flags or
 * reserved not 0; negative or non-finite sx, sy.  VJ_ERR_LIMIT: vj_extract's mapping limits.  VJ_ERR_NOMEM names the bytes.
 * n_rows == 0 is VJ_OK.  With "max_subbatch" configured a call runs in slices of rows that name at most that many frames (a
 * row that names more by itself is a slice of its own); the results are the same.                                              */
int  vj_track(vj_env* e, const vj_image* frames, int n_frames, const vj_track_row* rows, int n_rows,
              const vj_track_params* p, vj_track_result* out);
/* Device time of the environment's last vj_track call: events around its copies and launches (*ms), and around its match launches
 * alone (*match_ms; their sum when the call ran in slices), in ms.  A null argument: VJ_ERR_ARG.                              */
int  vj_track_timing(const vj_env* e, float* ms, float* match_ms);

/* ------------------------------------------------------------ frame streams */
/* Video-style use (the demo's per-frame loop, main.cpp:104-125): batches of host frames are uploaded into
 * one of two device buffers by DMA on a copy stream while the kernels of the previous batch run, and the
 * results come back one submit later.  submit() returns once the batch is queued (it blocks only while
 * both buffers are busy); collect() returns the oldest submitted batch (VJ_ERR_ARG when none is pending).
 * Frames must stay valid until their batch is collected; put them in vj_host_alloc memory for a copy-free
 * upload (pageable memory works, through a staging copy).  Results equal vj_detect's.                   */
typedef struct vj_stream vj_stream;
int  vj_stream_create(vj_env* e, const vj_cascade* c, int width, int height, int channels, int max_batch,
                      const vj_params* p, vj_stream** out);
int  vj_stream_submit(vj_stream* s, const vj_image* frames, int n_frames);
int  vj_stream_collect(vj_stream* s, vj_result* out);
void vj_stream_destroy(vj_stream* s);

/* filterResult (clod.cpp:182-357) as cv::groupRectangles defines it (tempcv.cpp:130-243): groups
 * `rects` (sorted by frame; grouped per frame, in place), keeps classes with more than
 * group_threshold members, weight = members, scale_idx = -1.  vj_detect applies it with
 * MAX(min_neighbors, 1) and eps 0.2 (clod.cpp:11, 1326) when min_neighbors != 0.            */
int vj_group_rectangles(vj_rect* rects, uint32_t* count, int group_threshold, double eps);
/* groupRectangles(rectList, rejectLevels, levelWeights, groupThreshold, eps) (tempcv.cpp:255-258 -> :145-243), host code, in place,
 * per frame (`rects` sorted by frame); returns the new count, or -VJ_ERR_ARG.  Per class: the greatest level of its members and,
 * among the members at that level, the greatest weight (starting from DBL_MIN); a class is kept iff its greatest LEVEL is >
 * group_threshold; the nested-rectangle filter compares that level with the OTHER class's member count (n2 = rweights[j]).  Out:
 * the averaged rectangle (weight 0, scale_idx -1), the class's level and weight.  group_threshold <= 0, literally (:147-156):
 * nothing is grouped, every level becomes 1 and the weights stay.                                                          */
int vj_group_rectangles_levels(vj_rect* rects, int32_t* levels, double* weights, int n, int group_threshold, double eps);

/* ---------------------------------------------------------------- multi-GPU */
/* One environment per device (clodInitEnvironment(device_index), clod.cpp:72-100), one rank per environment — threads of
 * one C++ host or processes.  The path shards without a data-path exchange: (frame, scale) pairs are
 * independent given a frame's integral images.  These two host helpers give every rank its share; the only collective is
 * the final all-gather of rectangles (include/vj_rccl.h: header-only, RCCL's ncclAllGather, so that this library itself
 * does not link librccl).
 * vj_shard_frames: batches with at least as many frames as ranks — contiguous blocks whose sizes differ by at most one.
 * vj_shard_scales: fewer frames than ranks (one large frame) — every rank integrates the frame and takes a subset of the
 * scales, longest-processing-time greedy on an estimated cost (windows x a per-window weight; the LDS-tile scales and the
 * global-gather scales are dealt separately so that each rank keeps both of its chains busy; integers only, ties to the
 * lower rank); the result goes into vj_params.scale_mask.  A rank that gets no scale (more ranks than scales) receives VJ_SCALE_MASK_NONE — an all-zero
 * mask would mean "every scale" and duplicate the other ranks' rectangles.                                                                                            */
int vj_shard_frames(int n_frames, int n_ranks, int rank, int* first, int* count);
int vj_shard_scales(const vj_cascade* c, int width, int height, const vj_params* p, int n_ranks, int rank,
                    uint64_t scale_mask[2]);

/* Candidate windows per frame for (cascade, size, params): sum of nx*ny over
 * accepted scales — the denominator of the windows/s metric.                   */
int vj_count_windows(const vj_cascade* c, int width, int height, const vj_params* p,
                     uint64_t* out);

#if defined(VJ_BUILDING) && defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* VJ_H_ */
