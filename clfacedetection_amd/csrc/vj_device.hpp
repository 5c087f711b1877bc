// Structures shared between the host driver (vj_env.cpp) and the gfx950 kernels
// (vj_kernels.hip).  All are plain PODs laid out for scalar (s_load) access: every
// field a wave needs is uniform across its 64 lanes.
#pragma once
#include <stdint.h>
#include "vj_cv_roi_units.hpp"
#include "vj_sq_strips.hpp"
#include "vj_gather_queue.hpp"

namespace vj {

// One accepted scale (setupScale output, clod.cpp:371-415, in device units).
struct ScaleDev {
    float    step;         // window stride in pixels (f32, as the reference keeps it)
    uint32_t nx;           // windows per grid row
    uint32_t nwin;         // nx * ny
    uint32_t e_lt;         // equ_rect left-top, ELEMENT offset from the window origin
    uint32_t e_dw;         // equ_rect width in elements
    uint32_t e_dh;         // equ_rect height * stride in elements
    float    area;         // (float)scaled_window_area
    uint32_t table_first;  // first NodeRec of this scale in the table (image-stride offsets)
    uint32_t q_base;       // first entry of this scale's segment in the survivor queues
    uint32_t q_cap;        // capacity of ONE of the segment's Q_PARTS parts (= nwin * frames per part)
    uint32_t scale_idx;    // k of s_k (for the detection record)
    uint32_t ny;           // window grid rows
    // LDS-tile path (tile_rw == 0: this scale runs on the global-gather path)
    uint32_t tile_rw;      // != 0: this scale's first pass runs on the LDS-tile kernel
    uint32_t tile_pitch;   // dwords per row of the LDS image tile
    uint32_t tile_rows;    // rows of the LDS image tile
    uint32_t tile_table_first;  // NodeRec table built with stride = tile_pitch
    uint32_t te_lt;        // equ_rect left-top in tile-pitch elements
    uint32_t te_dh;        // equ_rect height * tile_pitch
    uint32_t tiles_x;      // tiles per grid row
    uint32_t tile_tw;      // windows per tile row
    uint32_t tile_th;      // window rows per tile (tile_tw * tile_th <= TILE_WAVES * TILE_WAVE_CAP)
    uint32_t tile_row_end; // window rows [0, tile_row_end) run on the LDS-tile kernel, the rest on the global-gather path
    uint32_t tile_class;   // LDS size class of the tile launch
    uint32_t tile_half;    // != 0: step is exactly 2 and the tile rows are de-interleaved: even image columns
                           // first, odd columns from element tile_half on (window origins are all even, so a
                           // wave's gathers of one corner touch CONSECUTIVE dwords: no bank conflicts)
    int32_t  te_dw;        // equ_rect left->right distance in tile elements (signed when de-interleaved)
    uint32_t skip_base;    // P2 skip modes: first word of this scale in a frame's visited-window bitmap
    uint32_t skip_wpr;     // ... words per window row (VJ_FLAG_SKIP_ROW); 0: one flattened bit list (VJ_FLAG_SKIP_LIST)
    float    scale_f;      // s_k itself, and the scaled window: what a region of interest needs to lay out its own grid
    uint32_t win_w, win_h; // ... (setupScale, clod.cpp:371-415, evaluated on the device per region: roi_plan_units)
    uint32_t pos_base;     // != 0: window positions of this scale come from CascadeArgs::pos_tab[pos_base + index] (VJ_FLAG_GRID_F64)
    // Scale group of the tile kernel (consecutive step-2 de-interleaved scales that share one staged tile, laid out as the
    // group's largest scale lays out its own): this scale's NodeRec table and equ_rect offsets in the GROUP's pitch / half.
    // Equal to tile_table_first / te_* when the scale is not grouped or is the group's largest; the ROI pass uses its own.
    uint32_t grp_table_first;
    uint32_t grp_te_lt;
    uint32_t grp_te_dh;
    int32_t  grp_te_dw;
    // Block-transposed records of the wave-independent tail (TILE_TAIL_BLOCK_RECS NodeRec slots per block of
    // CascadeArgs::sp_blocks, see tile_wave_tail), in NodeRec units like the tables they restate: of tile_table_first (the ROI
    // pass) and of grp_table_first (the tile list).  Only filled when the plan has the tail.
    uint32_t tile_tail_first;
    uint32_t grp_tail_first;
    uint32_t sq32;         // != 0: win_w * win_h <= SQ32_MAX_AREA — the squared sum of any window of this scale is below 2^32, so
                           // the tile passes combine the LOW dwords of its four sqsum corners (mod 2^32: exact)
    uint32_t sq_strip;     // u32 layout of the squared integral (CascadeArgs::sq_u32), scales without sq32: the variance window in
                           // strips of this many elements (sq_strip_rows(e_dw) * stride, vj_sq_strips.hpp); 0 with sq32
};
static_assert(sizeof(ScaleDev) == 156, "ScaleDev is 156 bytes");

// One cascade stage with its resolved successors (tempcv.cpp:834-861 flattened).
struct StageDev {
    uint32_t first_node;   // flat node index (same for every scale)
    uint32_t n_nodes;
    float    threshold;
    int32_t  on_pass;      // next stage, or -1 accept
    int32_t  on_fail;      // next stage, or -2 reject
    uint32_t n_trees;
    uint32_t order;        // stage-tree sweep: the i-th record holds the i-th stage to visit (topological)
    uint32_t sp_first;     // wave-independent tail of a tile: index of the stage's first block in CascadeArgs::sp_blocks
    float    sp_delta;     // ... |tree-order stage sum - sequential stage sum| <= sp_delta for ANY window (see
                           //     tile_wave_tail): 4 * n * 2^-24 * sum_k max(|left_k|, |right_k|), rounded up
    uint32_t cv_f64;       // OpenCV profile: this stage multiplies in f64 (two_rects stump stage, tempcv.cpp:872-888)
    uint32_t pad[2];
};
static_assert(sizeof(StageDev) == 48, "StageDev is 48 bytes");

// One unit of first-pass work inside a frame: a run of consecutive windows of one scale.
struct UnitDev {
    uint32_t scale;        // index into ScaleDev[]
    uint32_t first;        // first window index (row-major in the scale's grid), or ix0 | iy0 << 16 of a 2-D block
    uint32_t count;        // <= UNIT_WINDOWS (2-D block: width * height); staged tile: > 1 = a scale group of this many scales from `scale` on
    uint32_t bw;           // 0: a run of consecutive windows; else the width of a 2-D block of windows
};

// Survivor record handed from one pass to the next: byte offset of the window origin
// in the batch sum image (frame included) and the window's variance.  It is the
// on-device twin of CLODSubwindowData (clod.cpp:33-38) without x/y (recoverable from
// the offset).
struct QEntry {
    uint32_t off;
    float    var;
};

// A raw detection: window origin offset + scale slot.
struct DetEntry {
    uint32_t off;
    uint32_t scale;        // index into ScaleDev[]
};

// A region of interest on the device (vj_roi's layout: frame, x, y, w, h) and one unit of work inside it.
struct RoiDev {
    int32_t frame, x, y, w, h;
};
struct RoiUnit {
    uint32_t roi;          // index into the region list
    uint32_t slot;         // scale (index into ScaleDev[])
    uint32_t first;        // first window of the unit, row-major in the region's own grid of this scale
    uint32_t count;        // <= UNIT_WINDOWS
    uint32_t nx, ny;       // the region's grid of this scale
};
struct RoiDet {
    uint32_t off;          // window origin, byte offset in the batch sum image
    uint32_t slot;
    uint32_t roi;
};
struct RoiTile {           // one LDS tile inside a region (cascade_tile_roi_pass)
    uint32_t roi;
    uint32_t slot;
    uint32_t first;        // ix0 | iy0 << 16 in the region's own grid of this scale
    uint32_t nxy;          // the region's grid: nx | ny << 16
    uint32_t twh;          // this tile's shape in windows, tw | th << 16: the region's grid cut into EQUAL parts no larger than the scale's
                           // tile (a 51 x 51 grid in 64 x 32 tiles: two tiles of 51 x 26, not 51 x 32 + 51 x 19), and only the rows / columns
                           // of the image such a tile needs are staged
};

// One block of <= 64 consecutive nodes of a stage (wave-independent tail of the tile kernel).
struct SpBlock {
    uint32_t first_node;   // flat node index
    uint32_t desc;         // jn | jb << 8 | b << 16 | nb << 20 | stage << 24
};

constexpr int UNIT_WINDOWS = 512;   // windows per wave-unit == per-wave LDS queue capacity (the linear cascade_pass above 4 waves: CascadeArgs::q_cap)
constexpr int WAVES_PER_BLOCK = 3;    // waves per workgroup of the global-gather kernels: with one workgroup per CU next to the tile
                                      // chain, 2 starve the gather chain (+12 ms); 4 made the gather chain 11 % faster and the tiles 1 %
                                      // slower (profiles/r03_notes.md #6g); single frames and stage trees run 3 (CascadeArgs::gather_waves)
constexpr int GATHER_WAVES_FULL = 4;  // the most waves with full queues: 4 KiB of LDS per wave, 16 KiB = what the tile classes leave free.  Stage
                                      // trees (a second array) stay at WAVES_PER_BLOCK; cascade_roi_pass takes up to this many
constexpr int GATHER_WAVES_MAX = 8;   // the linear cascade_pass divides the SAME 16 KiB among up to 8 waves (vj_gather_queue.hpp: 384 entries
                                      // per wave at 5, 320 at 6, 256 at 7 and 8), and the plan cuts its first-pass units to match.  Batches of
                                      // 8 frames and more run 8: the chain is 21 % faster at the same balance, the tiles 3 % slower, and the
                                      // balance moves one and a half scales further (profiles/r15_notes.md)
static_assert(GATHER_WAVES_MAX == (int)GATHER_WAVES_LIMIT && UNIT_WINDOWS == (int)GATHER_QUEUE_CAP_MAX &&
              GATHER_WAVES_FULL * UNIT_WINDOWS == (int)GATHER_LDS_ENTRIES, "vj_gather_queue.hpp describes these queues");
constexpr int MAX_SCALES = 128;
constexpr int MAX_PASSES = 8;         // == VJ_MAX_PASSES
constexpr uint32_t Q_PARTS = 8;       // parts of a scale's survivor-queue segment, by frame group (one per XCD to drain)
constexpr int TILE_WAVES = 8;        // waves per workgroup of the LDS-tile kernel (16 measured slower)
constexpr int TILE_W = 64;           // windows per tile row (= lanes of a wave)
constexpr int TILE_WAVE_CAP = 256;    // windows (= LDS queue entries) per wave of the tile kernel
constexpr int TILE_CLASSES = 3;       // LDS size classes, one launch each
constexpr int TILE_LDS_HEADER = (TILE_WAVES * TILE_WAVE_CAP * 2 + 32) * 4;  // queues + per-wave counts, bytes
constexpr int TILE_SP_MAX_WINDOWS = 256;  // windows a tile may carry into the wave-independent tail (32 per wave): entries, survivors and verdict words fit the 16 KiB queue area
constexpr int TILE_WS_MAX_WINDOWS = 512;  // wave-split finish: 8 chunks of packed entries (4 KiB) + 8 x 320 dwords of sums and verdict words
constexpr int TILE_SEG_MAX_WINDOWS = 256;  // stage-tree chains inside a tile: population + reject list (256 entries each) around the scratch
constexpr int TILE_SP_MAX_BLOCKS = 4;     // blocks of 64 stumps per stage at most (stages of <= 256 nodes)
constexpr int TILE_SP_BLOCK = 64;         // stumps evaluated per round and window (= lanes of a wave)
// The tail's copy of a block: four sub-arrays back to back — dwords 0..3 of the block's 64 records, dwords 4..7, dwords 8..11
// (16 bytes per record each, 1 KiB) and dwords 12..13 (8 bytes per record, 512 bytes) — so that a wave's load of one piece
// covers consecutive bytes; partial blocks are padded with zero records.  3584 bytes = 56 NodeRec slots.
constexpr int TILE_TAIL_BLOCK_RECS = (3 * 16 + 8) * TILE_SP_BLOCK / 64;
// SQ32_MAX_AREA, the largest window area whose squared sum always fits a dword: vj_sq_strips.hpp

struct CascadeArgs {
    const uint32_t* sum;        // batch sum images, frame f at f * frame_elems
    const uint64_t* sqsum;      // batch squared-sum images, same geometry (sq_u32: u32 elements mod 2^32 in the buffer's first half)
    const uint32_t* table;      // NodeRec[] viewed as dwords (16 per node)
    const ScaleDev* scales;
    const StageDev* stages;
    const UnitDev*  units;      // first-pass units of ONE frame (global-gather scales)
    uint32_t n_units;           // units per frame
    const UnitDev*  tile_units; // first-pass tiles of ONE frame (LDS-tile scales): first = ix0 | iy0 << 16
    uint32_t n_tile_units;
    uint32_t tile_lds_bytes;    // dynamic LDS of the tile kernel
    uint32_t* tile_ticket;      // eight ticket counters of this tile launch, one per part of the tile list (zeroed before the launch)
    uint32_t n_frames;
    uint32_t n_scales;
    uint32_t frame_elems;       // elements per frame in sum / sqsum
    uint32_t sum_bytes;         // n_frames * frame_elems * 4 (< 2^32)
    uint32_t stride;            // elements per image row (W + 1)
    uint32_t stage_begin, stage_end;  // stages [begin, end) evaluated by this pass
    uint32_t total_waves;       // gridDim.x * gather_waves
    uint32_t gather_waves;      // waves per workgroup of cascade_pass / cascade_roi_pass (linear cascade_pass: 1 ... 8; cascade_roi_pass: <= 4; stage trees: 3)
    uint32_t q_cap;             // entries of a wave's LDS queue: gather_queue_cap(gather_waves) in the linear cascade_pass, else UNIT_WINDOWS
    const QEntry*   q_in;       // survivor queue read by this pass (passes > 0)
    const uint32_t* q_in_count; // entry counts of q_in, [scale][Q_PARTS]
    uint32_t* q_ticket;         // Q_PARTS ticket counters of this pass, zeroed before the launch: a queue pass's chunks, the grid pass's units (vj_grid_parts.hpp)
    uint32_t wide_tail;         // queue passes: the stump-parallel tail keeps several windows' gathers in flight (small batches)
    uint32_t min_chunk;         // queue passes: smallest chunk of windows a wave draws (1..64)
    uint32_t q_slices;          // queue passes: a part's chunks are handed out in this many slices of every scale's range (frame-major order)
    // Band-major queue pass (batches; linear cascades): the first pass records where every unit's survivors landed in their
    // (scale, part) sub-queue (run_table[frame * n_units + unit] = {first entry, count}); the queue pass then draws GROUPS of
    // consecutive units of one (image band, scale) — the host orders a frame's units by band first — in (frame, group) order:
    // an XCD's waves work on one band of one frame across all scales before they move on (their gathers share an L2-sized
    // part of the sum image), and nothing has to be sorted.
    uint32_t* run_table;        // [n_frames * n_units][2] (null: not recorded)
    const UnitDev* q_groups;    // {scale, first unit, units, band} (null: the queue pass walks the sub-queues chunk by chunk)
    uint32_t n_q_groups;        // groups per frame
    QEntry*   q_out;            // survivor queue written by this pass (not the last)
    uint32_t* q_out_count;
    QEntry*   q_fail;           // stage trees: queue of the chain that takes this pass's rejects (else null)
    uint32_t* q_fail_count;
    // Tile launches: one survivor queue per pass boundary.  A wave sweeps the cascade one
    // pass segment at a time and leaves at boundary p — appending to queue p — as soon as
    // fewer than tile_min_lanes windows survive (or the boundary is >= tile_end).
    uint32_t  n_pass;                       // segments: [pass_begin[p], pass_begin[p+1])
    uint32_t  pass_begin[MAX_PASSES + 1];
    QEntry*   q_pass[MAX_PASSES];           // q_pass[p]: windows waiting to enter segment p (p >= 1)
    uint32_t* q_pass_count[MAX_PASSES];
    uint32_t  tile_end;                     // deepest stage a tile launch may enter
    uint32_t  tile_min_lanes;               // leave at a pass boundary when the whole tile has fewer survivors
    unsigned long long tile_repack_mask;    // bit s: re-pack the tile's survivors across its waves before stage s
    // Finish of a tile: once it is down to <= tile_ws_max windows at a re-pack point at or after tile_sp_begin, it
    // runs the rest of the cascade itself with the wave-split finish (tile_wave_split) and, below tile_ws_min windows
    // (stump cascades), the wave-independent tail (tile_wave_tail) — through the last stage.
    uint32_t  tile_sp_begin;                // >= number of stages: disabled
    uint32_t  identity_order;               // StageDev::order is 0, 1, 2, ... (every linear cascade)
    uint32_t  n_seg;                        // stage tree: chains after the linear prefix that a tile may run itself (0: none)
    uint32_t  seg_end[4];                   // ... end position (sweep order) of chain k; it starts where chain k-1 (or the prefix) ends
    uint32_t  seg_chain;                    // ... bit k: the rejects of chain k are the population of chain k+1
    uint32_t  tree2;                        // every tree has exactly two nodes, the second one the child of the first
    uint32_t  tile_ws_min;                  // the wave-split finish hands over to the wave-independent tail below this many
    uint32_t  tile_ws_max;                  // enter the wave-split finish when at most this many windows are left
    const SpBlock* sp_blocks;               // per block of <= 64 stumps, all stages in order
    uint32_t  n_sp_blocks;
    DetEntry* det;              // detections (last pass)
    uint32_t* det_count;
    uint32_t  det_cap;
    uint32_t  signed_mean;      // VJ_FLAG_SIGNED_MEAN
    unsigned long long* stage_entered;  // [VJ_MAX_STAGES] when counting, else null
    unsigned long long* tree_ctr;       // counting, multi-node trees: [0] nodes below the root that a window's walk visited, [1] their rectangles
    // P2 skip modes (VJ_FLAG_SKIP_LIST / VJ_FLAG_SKIP_ROW; clod.cpp:729-732, :1430): a bitmap of the grid windows the
    // reference's sequential CPU loops visit, built by skip_fail_bits + skip_resolve before the cascade passes;
    // null = every grid window (the OpenCL kernel's contract)
    unsigned long long* skip_bits;      // [n_frames][skip_frame_words]
    uint32_t  skip_frame_words;
    uint32_t  sp_tail_max;              // global-gather sweeps: at most this many windows left in a wave -> stump-parallel tail (0: off; <= gather_tail_max(q_cap))
    uint32_t  max_stage_nodes;          // nodes of the cascade's largest stage
    uint32_t  gather_pairs;             // global-gather sweeps evaluate two stumps per step: 0 never, 1 when the wave holds one chunk, 2 always
    uint32_t  pos_mode;                 // window_pos(): bit 0 = round half away from zero (clod.cpp:1416) instead of lrint (:514); bit 1: the block variant's f64 grid (ScaleDev::pos_base tables)
    const uint32_t* pos_tab;            // positions of the f64 grids (VJ_FLAG_GRID_F64), per scale from ScaleDev::pos_base; entry 0 is unused
    const UnitDev* skip_units;          // one per bitmap word of a frame: {scale, first window (flattened index, or ix0 | iy << 16), valid bits, word}
    uint32_t  n_skip_units;
    const UnitDev* skip_segs;           // one per recurrence domain (a window row, or a scale's whole list): {scale, first word, words, -}
    uint32_t  n_skip_segs;
    uint32_t  sq_u32;                   // != 0: sqsum holds u32 elements, the values mod 2^32 (IntegralArgs::sq_u32); scales without
                                        // ScaleDev::sq32 walk their variance window in strips (ScaleDev::sq_strip).  0: u64 elements
};

struct IntegralArgs {
    const uint8_t* gray;        // batch of frames
    uint64_t gray_frame_bytes;  // distance between frames
    uint32_t gray_stride;       // bytes per row
    uint32_t channels;          // 1: gray; 3: BGR, 4: BGRA (converted on the fly)
    uint32_t width, height;
    uint32_t n_frames;
    uint32_t n_bands;           // ceil(height / BAND_ROWS)
    uint32_t band_pitch;        // elements per band row in the band arrays (>= width, multiple of 4)
    uint32_t* band_sum;         // [frames][bands][band_pitch]  column sums of the band / exclusive prefix
    uint32_t* band_sq;          // [frames][bands][band_pitch]  column sums of squares of the band
    uint64_t* band_sq_prefix;   // [frames][bands][band_pitch]  exclusive prefix of band_sq over bands
    uint32_t* sum;              // [frames][frame_elems]
    uint64_t* sqsum;
    uint32_t frame_elems;
    uint32_t rows_mode;         // band_rows: 0 one wave walks a band's chunks; 1 the chunks side by side (band_rows_par); 2 side by side unless the call is a batch
    uint32_t sq_u32;            // != 0: the squares stay in 32 bits end to end — sqsum and band_sq_prefix are written as u32 arrays of
                                // the same element counts (the first halves of the buffers), values mod 2^32; 0: u64, the exact values
};
constexpr int BAND_ROWS = 8;

// Launch wrappers (defined in vj_kernels.hip); stream is a hipStream_t.
int launch_integral(const IntegralArgs& a, void* stream);
int launch_integral_sum(const IntegralArgs& a, void* stream);   // sum only (band_colsum_sum / band_scan_sum / band_rows_sum)
int launch_cascade_pass(const CascadeArgs& a, bool from_grid, bool trees, bool last, bool count, bool general,
                        int n_blocks, void* stream);
int launch_cascade_tile_pass(const CascadeArgs& a, bool trees, bool count, int n_blocks, void* stream);

// Regions of interest on the device (vj_detect_chain).
struct RoiArgs {
    // dets_to_rois: raw detections of a first cascade -> regions
    const DetEntry* det_in;
    const uint32_t* det_in_count;
    uint32_t det_in_cap;
    const ScaleDev* scales_in;   // the first cascade's scales (win_w / win_h)
    uint32_t frame_bytes;        // frame_elems * 4
    uint32_t stride;             // W + 1
    RoiDev* rois;                // region list (written by dets_to_rois, or supplied by the caller)
    uint32_t* n_rois;            // on the device
    uint32_t max_rois;
    // roi_plan_units: every region lays out the second cascade's grid inside itself
    uint32_t n_frames;
    int32_t  frame_w, frame_h;
    int32_t  win_w0, win_h0;     // the second cascade's base window
    int32_t  min_w, min_h, max_w, max_h;
    RoiUnit* units;
    uint32_t* n_units;
    uint32_t max_units;
    uint32_t* ticket;            // unit ticket counter of cascade_roi_pass
    // cascade_roi_pass
    RoiDet* det;
    uint32_t* det_count;
    uint32_t det_cap;
    // cascade_tile_roi_pass: (region, scale) grids of at least tile_min_windows windows on two-per-CU tile scales (null: none)
    RoiTile* tiles;
    uint32_t* n_tiles;
    uint32_t max_tiles;
    uint32_t tile_min_windows;
    uint32_t tile_blocks;        // workgroups of the launch
};
int launch_roi_chain(const RoiArgs& r, const CascadeArgs& a, bool from_dets, bool trees, bool count, bool general /* stage tree */,
                     int n_blocks, void* stream, void* stream2 /* may be null */, void* fork_ev, void* join_ev);

// Grouping of a first cascade's raw candidates on the device (vj_detect_chain with min_neighbors != 0): the grouped
// rectangles become the region list of the second cascade without a host round trip (vj_group_dev.hip).
constexpr uint32_t GROUP_MAX = 2048;   // raw candidates of ONE frame the device kernel groups; beyond that the host path runs
struct GroupArgs {
    const DetEntry* det;         // the first cascade's detection buffer (device order)
    const uint32_t* det_count;
    uint32_t det_cap;
    const ScaleDev* scales;      // the first cascade's scales (win_w / win_h)
    uint32_t frame_bytes;        // frame_elems * 4
    uint32_t stride;             // W + 1
    uint32_t n_frames;
    int32_t  threshold;          // MAX(min_neighbors, 1)
    double   eps;                // 0.2 (clod.cpp:11)
    uint32_t* frame_count;       // [n_frames]      raw candidates per frame          } one block, zeroed by the
    uint32_t* frame_cursor;      // [n_frames]      scatter cursors                   } launcher
    uint32_t* grouped_count;     // [n_frames]      grouped rectangles per frame      }
    uint32_t* overflow;          // [1]             frames with more than GROUP_MAX   }
    uint32_t* frame_first;       // [n_frames + 1]  exclusive prefix of frame_count
    uint64_t* keys;              // [det_cap]       candidates bucketed by frame: scale slot << 32 | element index in the frame
    RoiDev*   grouped;           // [det_cap]       per-frame segments (at frame_first[frame])
    uint32_t* grouped_weight;    // [det_cap]
    RoiDev*   rois;              // out: the region list, frames in order
    uint32_t* roi_weight;        // out: members of every group
    uint32_t* n_rois;            // out (device)
    uint32_t  max_rois;
    uint32_t  group_max;         // <= GROUP_MAX
};
int launch_group_rois(const GroupArgs& g, void* stream);
int prepare_group_kernels();   // per device: dynamic-LDS cap of group_frame
int launch_skip_bitmap(const CascadeArgs& a, bool trees, int n_blocks, void* stream);   // fail bits, then the visited bitmap
int prepare_tile_kernels();   // per device: raise the dynamic-LDS cap of the tile kernel's instantiations

}  // namespace vj

// ------------------------------------------------------------ OpenCV arithmetic profile (vj_cv.cpp)
namespace vj {

// One scale of cvHaarDetectObjects' scale-cascade loop (tempcv.cpp:1359-1417) with what
// cvSetImagesForHaarClassifierCascade (tempcv.cpp:549-632) derives for it.
struct CvScaleDev {
    double   ystep;        // max(2, factor)
    double   inv_area;     // weight_scale = 1 / (equ_w * equ_h)
    uint32_t win_w, win_h; // cvRound(orig * factor)
    uint32_t end_x, end_y; // window grid: ix in [0, end_x), iy in [0, end_y)
    uint32_t q0, q1, q2, q3;   // the four corners of equRect, element offsets from the window origin
    uint32_t table_first;  // first NodeRec of this scale
    uint32_t scale_idx;    // index of the factor in the enumeration (skipped scales keep their number)
    // LDS-tile path of the profile (vj_cv_tile.hip; tile_th == 0: the scale runs on cv_profile_pass)
    uint32_t tile_tw, tile_th;   // windows per tile row (64, 32 or 16: a tile row never straddles a bitmap word) and rows per tile (<= 32)
    uint32_t tile_pitch;         // dwords per row of the LDS image tile (a multiple of 4)
    uint32_t tile_rows;          // rows of the LDS image tile
    uint32_t tile_table_first;   // first CvNodeRec of this scale built with the tile's pitch
    uint32_t bits_base;          // first word of this scale in a frame's reject / visited bitmap ((end_x + 63) / 64 words per window row)
    // stage trees on tiles: the survivors of the tree's linear prefix wait in one sub-queue per scale (a chunk of the walk
    // then holds windows of ONE scale: full lanes, scalar table).  Sub-queue of this scale for n_frames frames: entries
    // [tq_first(n_frames, shift), + tq_cap(n_frames, shift)) — see cv_tq_first / cv_tq_cap
    uint32_t tq_win_first;       // grid windows of the tile scales before this one, per frame
    uint32_t tq_slot;            // this scale's number among the tile scales
};
static_assert(sizeof(CvScaleDev) == 88, "CvScaleDev is 88 bytes");
// entries of the whole tree queue at most (6 GiB of CvTreeEntry): a sub-batch whose queue would need more is split
// (vj_detect_opencv), so that every sub-queue lies inside the buffer
constexpr uint64_t CV_TQ_MAX = 1ull << 28;
// one sub-queue: 1 / 2^shift of the scale's grid windows in the batch, at least 4096 entries
VJ_HD inline uint64_t cv_tq_cap(uint32_t end_x, uint32_t end_y, uint32_t n_frames, uint32_t shift) {
    return (((uint64_t)end_x * end_y * n_frames) >> shift) + 4096u;
}
VJ_HD inline uint64_t cv_tq_first(uint32_t tq_win_first, uint32_t tq_slot, uint32_t n_frames, uint32_t shift) {
    return (((uint64_t)tq_win_first * n_frames) >> shift) + (uint64_t)tq_slot * 4096u;
}

// Node record of the OpenCV profile (64 bytes, fetched through the scalar cache like NodeRec): corner q of
// rectangle k sits at lt[k] + {0, da[k], db[k], da[k] + db[k]} bytes from the window origin — upright rectangles
// da = width, db = height * stride; tilted ones (tempcv.cpp:743-750) da = height * (stride - 1), db = width *
// (stride + 1), in the tilted integral image.
struct alignas(16) CvNodeRec {
    uint32_t lt[3], da[3], db[3];
    float    w[3];         // w[2] == 0: two rectangles
    float    thr;
    uint32_t left, right;  // f32 leaf value bits, or child node index (flags)
    uint32_t flags;        // NODE_LEFT_IS_NODE | NODE_RIGHT_IS_NODE | NODE_TREE_LAST | CV_NODE_TILTED
};
static_assert(sizeof(CvNodeRec) == 64, "CvNodeRec must be 64 bytes");
constexpr uint32_t CV_NODE_TILTED = 8u;

// A stage tree whose part after the linear prefix is a sequence of CHAINS (tempcv.cpp:834-861 on frontalface_alt_tree: stages
// 0-4, then 5, 7, ..., 39, whose rejects — anywhere — start 6, 8, ..., 46): chain k covers positions [begin[k], end[k]) of the
// sweep order; passing a stage leads to the next position, passing the chain's last stage accepts; a reject inside chain k
// continues at the first stage of chain k + 1 when bit k of `chained` is set, else it is final.  n == 0: the tree does not
// have this shape (the per-lane target-stage walk is used).
struct CvChainDev {
    uint32_t n;
    uint32_t begin[4], end[4];
    uint32_t chained;
    uint32_t tail_max;           // see CV_TAIL_MAX
};
constexpr uint32_t CV_TAIL_MAX = 64;        // a population of at most CvChainDev::tail_max <= this many windows evaluates a stage stump-parallel (lane = stump)
constexpr uint32_t CV_TAIL_BLOCKS = 8;      // ... stages of up to 8 x 64 nodes
constexpr uint32_t CV_TQ_CHUNK = 256;       // windows per chunk of cv_tree_chain_pass at most (LDS: 24 bytes each; CvTreeArgs::chunk <= this)

constexpr int CV_WAVES_PER_BLOCK = 4;
constexpr int VJ_MAX_STAGES_DEV = 64;  // == VJ_MAX_STAGES
constexpr int CV_QCAP = 320;           // survivors of stage 0 a wave collects before it sweeps the later stages

// CV_HAAR_DO_CANNY_PRUNING's test of a window (tempcv.cpp:1147-1158): element offsets, from the window origin, of the corners of
// [cvRound(0.15 w), + cvRound(0.7 w)) x [cvRound(0.15 h), + cvRound(0.7 h)) in a (W + 1)-wide integral image
struct CvPruneDev { uint32_t p0, p1, p2, p3; };

struct CvArgs {
    const uint32_t* sum;
    const uint32_t* tilted;      // tilted integral images, same geometry as sum (null: no tilted features)
    const uint64_t* sqsum;
    const uint32_t* table;       // NodeRec[] (offsets in bytes, f32 weights per tempcv.cpp:700-768)
    const CvScaleDev* scales;
    const StageDev* stages;      // threshold = stage threshold - 0.0001f (tempcv.cpp:262, 419)
    const UnitDev* rows;         // one unit per (scale, window row): {scale slot, iy}; the exhaustive-grid kernels (scale-image levels): {level
                                 // slot, iy, element offset of the level's origin in the canvas's integral images}
    uint32_t n_rows;             // per frame
    uint32_t n_frames;
    uint32_t n_stages;
    uint32_t n_order;            // stage trees: stages reachable from stage 0, swept in StageDev::order
    uint32_t frame_elems;
    uint32_t stride;             // W + 1
    uint32_t sum_h;              // H + 1
    uint32_t total_waves;
    CvDet* det;
    uint32_t* det_count;
    uint32_t det_cap;
    unsigned long long* stage_entered;   // [VJ_MAX_STAGES] + [VJ_MAX_STAGES] = windows visited (border ones included)
    CvChainDev chains;           // stage trees made of chains (else n = 0)
    void* fail_scratch;          // ... CV_QCAP x 16 bytes per wave: where a chain's rejects wait for the next chain
    uint32_t tail_max;           // linear cascades: a wave's queue of at most this many windows evaluates a stage stump-parallel (<= CV_TAIL_MAX)
    uint32_t tree2;              // every tree is a root + its only node child, upright (frontalface_alt2): both nodes' gathers in flight
    // CV_HAAR_DO_CANNY_PRUNING (read by the prune variants of cv_profile_pass only)
    const uint32_t* edge_sum;    // integral images of the frames' edge maps, same geometry as sum
    const CvPruneDev* prune;     // per scale slot: the pruning rectangle's corners
};

// launch_cv_profile_pass(..., prune): the CV_HAAR_DO_CANNY_PRUNING variants (tempcv.cpp:1147-1158)
// exhaustive: CV_HAAR_SCALE_IMAGE's grid (tempcv.cpp:1079-1102) — every position is evaluated, a reject skips nothing, no border rule;
// a scale is a pyramid level in the canvas (ystep 1 or 2, positions and detections in the level's own coordinates)
// roc: cvHaarDetectObjectsForROC's outputRejectLevels (tempcv.cpp:1084-1095; exhaustive grid only) — CvArgs::det is
// an array of CvRocDet and det_cap counts those: a window is reported with the stage it reached and that stage's sum
int launch_cv_profile_pass(const CvArgs& a, bool trees, bool count, bool stage_tree, int n_blocks, void* stream, bool prune = false,
                           bool exhaustive = false, bool roc = false);

// One reported window of a ROC call: a linear cascade reports who passes (level = the stage count, weight = the last stage's sum) and
// who fails one of the last three stages (level = that stage, weight = its sum); a stage tree reports the accepted windows only.
struct CvRocDet {
    uint32_t x, y, slot, frame;   // as CvDet
    uint32_t level, pad;
    double weight;                // stage_sum of the last stage evaluated, the f64 the verdict compared
};
static_assert(sizeof(CvRocDet) == 32, "CvRocDet is 32 bytes");

// CV_HAAR_FIND_BIGGEST_OBJECT (VJ_FLAG_CV_FIND_BIGGEST; vj_cv_biggest.hip): the scales run from the largest window
// down, one round each, and every frame carries its own search state on the device — written by cv_biggest_update only, read by
// the waves of cv_biggest_pass (wave-uniform: through the scalar cache).  Zeroed per call and sub-batch.
struct CvBigState {
    uint32_t phase;          // 0: searching (the whole grid; scanROI is empty), 1: inside scanROI, 2: stopped on a limit (`flags`)
    uint32_t flags;          // CV_BIG_OVERFLOW: the frame's candidate segment was full when it had to be grouped; CV_BIG_LIMIT: more
                             // than GROUP_MAX candidates before the first grouped object
    int32_t  roi_x, roi_y, roi_w, roi_h;   // scanROI (tempcv.cpp:1442-1448)
    int32_t  min_w, min_h;   // minSize from the hit on (:1450-1452); phase 0: the call's
    int32_t  max_x, max_y, max_w, max_h;   // maxRect, as pushed onto the frame's candidates (:1440)
    uint32_t hit_slot;       // the scale slot after which it was found: maxRect follows that scale's candidates in the list
    uint32_t n_seen;         // candidates at the last grouping that found nothing (no new candidate: no new grouping)
    uint32_t pad[2];
};
static_assert(sizeof(CvBigState) == 64, "CvBigState is 64 bytes");
constexpr uint32_t CV_BIG_OVERFLOW = 1u, CV_BIG_LIMIT = 2u;
struct CvBigArgs {
    CvArgs cv;               // images, tables, stages, counters as for cv_profile_pass; rows / n_rows / chains / prune are not read;
                             // det: n_frames segments of det_cap candidates each (CvDet::slot = scale slot, in walk order)
    CvBigState* state;       // [n_frames]
    uint32_t* frame_count;   // [n_frames] candidates of each frame (may exceed det_cap: the call is repeated with more room)
    uint32_t slot;           // the round's scale (CvScaleDev slot; slots are in walk order: descending factor)
    int32_t  min_w, min_h;   // the call's minSize
    uint32_t width, height;  // of a frame
    int32_t  threshold;      // max(minNeighbors, 1)
    uint32_t rough;          // CV_HAAR_DO_ROUGH_SEARCH: minSize = 0.6 of the hit instead of 0.4
    double   eps;            // GROUP_EPS = 0.2
};
// one round: the scale `slot` on every frame that still searches or whose scanROI takes it, then the grouping step of the frames
// still searching (`update`); both on `stream`, in this order
int launch_cv_biggest_round(const CvBigArgs& a, bool trees, bool count, bool stage_tree, int n_blocks, bool update, void* stream);
int prepare_cv_biggest_kernels();   // per device: the dynamic-LDS cap of cv_biggest_update

// The profile's region pass (vj_detect_opencv_rois / vj_detect_opencv_chain; vj_cv_roi.hip): a cascade inside regions of
// the frames, on the frames' own integral images.  A region is the sub-image an OpenCV caller would hand over: factors, grid ends and
// the border rule come from its w x h.
// CvRoiDev, CvRoiUnit (and CvDet): vj_cv_roi_units.hpp
struct CvRoiArgs {
    CvArgs cv;               // images, stages, counters, detections as for cv_profile_pass (CvDet::frame = the region's index in `rois`); rows /
                             // n_rows / chains / prune are not read; scales: one record per FACTOR slot (win, equRect corners, ystep,
                             // table_first; its end_x / end_y are not read: the grid is the region's)
    const CvRoiDev* rois;
    const CvRoiUnit* units;  // ordered by (frame, region, factor, row)
    uint32_t n_units;
    const uint32_t* n_units_dev;   // not null: the unit count is read from here (the list was built on the device: vj_cv_chain.hip)
};
int launch_cv_roi_pass(const CvRoiArgs& a, bool trees, bool count, bool stage_tree, int n_blocks, void* stream);

// vj_detect_opencv_chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE; vj_cv_chain.hip): the first cascade's CvDet
// records become the regions (CvRoiDev) and units (CvRoiUnit) of the region pass without leaving the device.
struct CvChainArgs {
    const CvDet* det;            // the first cascade's detections: {x, y, scale slot, frame of the sub-batch}
    const uint32_t* det_count;   // ... their count (may exceed det_cap: the sub-batch is enqueued again with more room)
    uint32_t det_cap;
    const CvScaleDev* scales;    // the FIRST plan's scale records (win_w / win_h of a slot)
    uint32_t n_scales;
    uint32_t n_frames, width, height;
    uint32_t stride;             // W + 1
    uint32_t frame_elems;
    uint32_t grouped;            // 0: every record is a region; 1: grouped per frame (groupRectangles)
    int32_t  threshold;          // max(min_neighbors, 1)
    uint32_t group_max;          // a frame with more candidates raises CvChainState::overflow
    double   eps;                // GROUP_EPS = 0.2
    uint32_t* frame_count;       // [n_frames] } one zeroed block: frame_count | frame_cursor | grouped_count
    uint32_t* frame_cursor;      // [n_frames] }
    uint32_t* grouped_count;     // [n_frames] }
    uint32_t* frame_first;       // [n_frames + 1]
    uint64_t* keys;              // [det_cap] grouped: slot << 32 | y * stride + x, a frame's together
    CvRoiDev* staged;            // [det_cap] grouped: a frame's rectangles at frame_first[frame]
    CvRoiDev* rois;              // [det_cap] the regions, a frame's together, frames in order
    const CvChainFactor* factors;   // the SECOND cascade's factor slots (the region plan's)
    uint32_t n_factors;          // >= 1
    double   scale_factor;       // the second call's (the factor after the table's last: refused, as on the host)
    int32_t  win_w, win_h;       // the second cascade's window
    int32_t  min_w, min_h;       // its minimum object size
    uint32_t* roi_units;         // [det_cap] units of each region
    uint32_t* roi_first;         // [det_cap] where a region's units start
    CvRoiUnit* units;            // [unit_cap] ordered by (region, factor, row)
    uint32_t unit_cap;
    CvChainState* state;         // zeroed before the launches
};
// regions (count / offsets / scatter, or scatter / group / collect), then units (count / offsets / fill); all on `stream`, in order
int launch_cv_chain_handoff(const CvChainArgs& a, int n_cu, void* stream);
int prepare_cv_chain_kernels();   // per device: the dynamic-LDS cap of the grouping kernel

// The profile's LDS-tile kernel (vj_cv_tile.hip): small scales of stump cascades with linear stages and upright features.
constexpr int CVT_WAVES = 8;            // waves per workgroup
constexpr int CVT_WAVE_CAP = 256;       // windows (queue entries) per wave: four tile rows of <= 64 windows
constexpr int CVT_WS_MAX = 512;         // windows a tile may carry into the wave-split finish
constexpr int CVT_LDS_HEADER = CVT_WAVES * CVT_WAVE_CAP * 12 + 512;   // offset queue (u32) + norm-factor queue (f64) + counters + 32 reject words, bytes
struct CvTileArgs {
    const uint32_t* sum;
    const uint32_t* tilted;      // tilted integral images, same geometry (null: the cascade has no tilted features): staged behind the sum tile
    const uint64_t* sqsum;
    const uint32_t* table;       // CvNodeRec[] (the tile scales' records carry offsets in the tile's pitch)
    const CvScaleDev* scales;
    const StageDev* stages;      // as CvArgs::stages, plus sp_delta (order-independence bound of a stage's leaf sum)
    const UnitDev* tiles;        // tiles of ONE frame in this launch's LDS class: {scale slot, ix0 | iy0 << 16}; mode 3: {level slot, ix0 | iy0 << 16,
                                 // element offset of the level's origin in the canvas's integral images}
    uint32_t n_tiles;
    uint32_t* ticket;            // eight ticket counters of this launch (zeroed before it)
    uint32_t n_frames, n_stages, frame_elems;
    uint32_t stride;             // W + 1
    uint32_t sum_h;              // H + 1
    unsigned long long* bits;    // [n_frames][bits_frame_words]: stage-0 reject bits (pass 0), visited bits after skip_resolve
    uint32_t bits_frame_words;
    uint32_t lds_bytes;          // dynamic LDS of the launch
    unsigned long long repack_mask;   // bit s: pool the tile's survivors across its waves before stage s
    uint32_t ws_begin, ws_max;   // wave-split finish from this stage on, once at most ws_max (<= CVT_WS_MAX) windows are left
    CvDet* det;
    uint32_t* det_count;
    uint32_t det_cap;
    unsigned long long* stage_entered;   // as CvArgs
    // stage trees (mode 2): the survivors of the tree's linear prefix wait here for cv_tree_walk
    struct CvTreeEntry* tq;
    uint32_t* tq_count;          // one counter per tile scale (CvScaleDev::tq_slot; [0] alone for the flat queue); [64] is the
                                 // ticket of cv_tree_chain_pass (CvTreeArgs::ticket), not a count of this kernel
    uint32_t tq_cap;             // total entries of the queue buffer (all sub-queues)
    uint32_t tq_shift;
};
// A window that passed the linear prefix of a stage tree inside a tile and walks the rest of the tree with global gathers.
struct CvTreeEntry {
    uint32_t off;        // byte offset of the window origin in the batch sum image
    uint32_t word;       // its word in the reject / accept bitmaps (frame included)
    uint32_t bit_slot;   // bit | scale slot << 8
    uint32_t pad;
    double   vnf;        // variance norm factor
};
int launch_cv_tile_pass(const CvTileArgs& a, int mode /* 0: reject bits of stage 0, 1: the cascade on the visited windows, 2: stage trees:
                        the linear prefix on every grid window, 3: CV_HAAR_SCALE_IMAGE: the cascade on every grid window of a pyramid level */, bool count, bool tree2 /* every tree: a root and one node child */, int n_blocks, void* stream);
// Stage trees on tiles: the rest of the tree for the prefix's survivors (reject / accept bits), then — after skip_resolve — the
// accepted windows the walk visits become detections (vj_cv_profile.hip).
struct CvTreeArgs {
    const uint32_t* sum;
    const uint32_t* table;       // frame-stride CvNodeRec tables
    const CvScaleDev* scales;
    const StageDev* stages;
    uint32_t n_order, prefix;    // sweep positions [prefix, n_order) are walked
    uint32_t sum_bytes;          // n_frames * frame_elems * 4
    const CvTreeEntry* tq;
    const uint32_t* tq_count;
    uint32_t tq_cap;
    unsigned long long* reject;  // [n_frames][bits_frame_words]; visited bits after skip_resolve
    unsigned long long* accept;
    uint32_t bits_frame_words, n_frames;
    const UnitDev* segs;         // one per window row of a tile scale: {scale slot, first word, words per row}
    uint32_t n_segs;
    CvDet* det;
    uint32_t* det_count;
    uint32_t det_cap;
    // per-scale sub-queues + chains (cv_tree_chain_pass)
    uint32_t tq_shift;           // sub-queue capacities: cv_tq_cap(.., n_frames, tq_shift)
    uint32_t n_scales;
    uint32_t* ticket;            // chunk ticket counter (zeroed before the launch)
    CvChainDev chains;
    void* fail_scratch;          // CV_TQ_CHUNK x 24 bytes per wave
    uint32_t total_waves;
    uint32_t chunk;              // windows a wave draws at a time (64 .. CV_TQ_CHUNK)
};
int launch_cv_tree_walk(const CvTreeArgs& a, int n_blocks, void* stream);
int launch_cv_tree_chain_pass(const CvTreeArgs& a, int n_blocks, void* stream);
int launch_cv_tree_emit(const CvTreeArgs& a, int n_blocks, void* stream);
int prepare_cv_tile_kernels();   // per device: raise the dynamic-LDS cap
int launch_skip_resolve(const CascadeArgs& a, int n_blocks, void* stream);   // reject bits -> visited bits (vj_kernels.hip)

struct TiltedArgs {
    const uint8_t* gray;        // batch of frames
    uint64_t gray_frame_bytes;
    uint32_t gray_stride;
    uint32_t channels;
    uint32_t width, height;
    uint32_t n_frames;
    uint32_t frame_elems;
    uint32_t* tilted;           // [frames][frame_elems], rows of W + 1
};
// the tilted integral as three banded prefix sums; diag: n_frames x bands x 2 x (W + H) dwords, col: n_frames x bands x (W + 1)
int launch_tilted_bands(const TiltedArgs& a, uint32_t* diag, uint32_t* col, void* stream);
int launch_grayscale(const TiltedArgs& a, uint8_t* dst, uint32_t dst_stride, void* stream);

// The Canny edge map of CV_HAAR_DO_CANNY_PRUNING (vj_canny.hip): cvCanny(gray, edges, 0, 50, 3) for a batch of frames
struct CannyArgs {
    const uint8_t* gray;        // batch of frames (1 / 3 / 4 channels, as IntegralArgs)
    uint64_t gray_frame_bytes;
    uint32_t gray_stride;
    uint32_t channels;
    uint32_t width, height;
    uint32_t n_frames;
    uint8_t* cls;               // [frames][W * H] 0 not a candidate, 1 weak, 2 strong
    uint32_t* label;            // [frames][W * H] union-find parents (frame-local pixel indices)
    uint8_t* flag;              // [frames][W * H] 1: a root whose component holds a strong pixel
    uint8_t* edges;             // [frames] x edge_frame_bytes, rows of edge_pitch bytes: 0 / 255
    uint32_t edge_pitch;
    uint64_t edge_frame_bytes;
};
int launch_canny(const CannyArgs& a, void* stream);   // four kernels and a memset: a fixed count whatever the content

// CV_HAAR_DO_CANNY_PRUNING on the LDS-tile scales (vj_canny.hip): the pruning test of every grid window of the tile scales into a
// bitmap of the tiles' layout (one recurrence domain per window row, CvPlan::bit_segs), which feeds the unchanged tile kernels:
//   cv_prune_mark     prune_bits = the test; bits |= prune_bits (a pruned window is a "zero" of the walk); accept &= ~prune_bits
//   cv_prune_visited  (after skip_resolve) visited &= ~prune_bits, the pruned visited windows counted into *windows
struct CvPruneArgs {
    const uint32_t* sum;
    const uint32_t* edge_sum;
    const CvScaleDev* scales;
    const CvPruneDev* prune;
    const UnitDev* segs;         // {scale slot, first word, words per row, -}
    uint32_t n_segs, n_frames, frame_elems, stride, bits_frame_words;
    unsigned long long* bits;        // reject bits (mark) / visited bits (visited)
    unsigned long long* accept;      // stage trees: accept bits (null: linear cascade)
    unsigned long long* prune_bits;
    unsigned long long* windows;     // VJ_FLAG_COUNTERS: counts.windows (null: not counted)
};
int launch_cv_prune_mark(const CvPruneArgs& a, int n_blocks, void* stream);
int launch_cv_prune_visited(const CvPruneArgs& a, int n_blocks, void* stream);

// CV_HAAR_SCALE_IMAGE (VJ_FLAG_CV_SCALE_IMAGE; vj_pyramid.hip): every level of every frame's pyramid in ONE launch, written into
// one canvas per frame that holds all levels (shelf-packed; the integral kernels then run on the canvas as on a frame).
// cvResize(CV_INTER_LINEAR) of 8-bit gray, DESIGN.md §4.8: coefficient tables built on the host per plan.
// (PyrTap: vj_cv_roi_units.hpp, shared with the host planner of the regions' level canvases)
struct PyrLevelDev {
    uint32_t ox, oy;       // the level's origin in the canvas
    uint32_t w, h;         // its size
    uint32_t xtab, ytab;   // first PyrTap of its columns / rows in PyrArgs::taps
    uint32_t unit_first;   // first work unit (PYR_UNIT_PX pixels of one row) of this level within a frame
    uint32_t area;         // != 0: the source is exactly 2 w x 2 h: dst = (2 x 2 sum + 2) >> 2
};
constexpr uint32_t PYR_UNIT_PX = 256;   // pixels per workgroup: one thread each
struct PyrArgs {
    const uint8_t* gray;        // batch of frames (1 / 3 / 4 channels, as IntegralArgs)
    uint64_t gray_frame_bytes;
    uint32_t gray_stride;
    uint32_t channels;
    uint32_t width, height;     // of a frame
    uint32_t n_frames;
    const PyrLevelDev* levels;
    uint32_t n_levels;
    uint32_t n_units;           // per frame
    const PyrTap* taps;
    uint8_t* canvas;            // [frames] x canvas_frame_bytes, rows of canvas_pitch bytes
    uint32_t canvas_pitch;
    uint32_t canvas_w, canvas_h;
    uint64_t canvas_frame_bytes;
};
int launch_pyramid(const PyrArgs& a, void* stream);

// CV_HAAR_SCALE_IMAGE inside regions (vj_detect_opencv_rois, route 2; pyramid_regions in vj_pyramid.hip): every level
// image of every region of a canvas in ONE launch.  The levels name their source frame and crop (PyrRegionLevelDev); one canvas, not
// one per frame.
struct PyrRegionArgs {
    const uint8_t* gray;        // the sub-batch's frames (1 / 3 / 4 channels)
    uint64_t gray_frame_bytes;
    uint32_t gray_stride;
    uint32_t channels;
    uint32_t width, height;     // of a frame
    uint32_t n_frames;
    const PyrRegionLevelDev* levels;
    uint32_t n_levels;
    uint32_t n_units;
    const PyrTap* taps;
    uint8_t* canvas;            // rows of canvas_pitch bytes (a multiple of 4)
    uint32_t canvas_pitch;
    uint32_t canvas_w, canvas_h;
};
int launch_pyramid_regions(const PyrRegionArgs& a, void* stream);

}  // namespace vj
