// The settings of an environment (vj_env_configure) as a plain struct: no HIP type in it, so that the host-only planner
// (vj_clod_plan.cpp) and its sanitizer driver compile against it without the HIP runtime.
#pragma once
#include "vj_internal.hpp"
#include "vj_device.hpp"

#include <algorithm>
#include <vector>

namespace vj {

// What vj_env_configure sets, with the shipped values as initialisers: vj_env_create starts from Tunables{} and
// vj_env_configure(e, "defaults", "") returns to it.  Speed only — results never depend on them.
struct Tunables {
    int max_subbatch = 0;      // > 0: cap on frames per sub-batch (tests)
    uint32_t det_cap_init = 1u << 16;  // initial capacity of the detection buffer (grows on overflow)
    int concurrent = 1;   // 1: the tile chain and the global-gather chain overlap on two streams
    int gather_waves = -1;              // waves per workgroup of the global-gather kernels, 1 ... 8 (-1: calls of >= 8 frames 8 for stump cascades and
                                        // 4 for cascades of multi-node trees, else 3); above 4 the waves' queues are shorter (vj_gather_queue.hpp)
                                        // and the first-pass units with them.  5, 6 and 7 double the queue pass next to the tiles, and two-node
                                        // trees gain nothing from 8 (profiles/r15_notes.md)
    int gather_waves_for(int n_frames, bool general, bool trees) const {
        if (general) return vj::WAVES_PER_BLOCK;
        const int w = gather_waves > 0 ? gather_waves : (n_frames >= 8 ? (trees ? vj::GATHER_WAVES_FULL : vj::GATHER_WAVES_MAX) : vj::WAVES_PER_BLOCK);
        return std::min(std::max(w, 1), (int)vj::GATHER_WAVES_MAX);
    }
    // windows per first-pass unit of a plan built for a call of n_frames frames (stage trees keep the 512-entry layout)
    uint32_t unit_cap_for(int n_frames, bool general, bool trees) const {
        return general ? (uint32_t)vj::UNIT_WINDOWS : vj::gather_queue_cap((uint32_t)gather_waves_for(n_frames, false, trees));
    }
    int concurrent_blocks_per_cu = 1;   // workgroups per CU of the global-gather chain while it overlaps
    // scales' worth of tile work handed to the global-gather chain (largest tile scales first), by batch size: a single
    // frame is bound by the latency of the gather chain's thin queue pass (measured, 1080p / frontalface_alt: 1 frame
    // 1.20 / 1.46 / 1.46 ms at split 0 / 0.5 / 1.25; 4 frames 3.50 / 3.61 / 3.96; 16 frames 12.51 / 12.25 / 12.36;
    // 64 frames — / 48.0 / 54.0), so small batches keep everything they can on the tiles
    float tile_split = 2.5f;            // batches of >= 32 frames (round 16, the tile sweep's groups of three chunks and paired lone chunks: 64 x 1080p 33.35 / 33.08 / 33.41 / 34.45 / 35.95 ms for 2.25 / 2.5 / 2.75 / 3 / 3.25, 32: 16.77 / 16.67 / 16.91 / 17.40 / 18.06, repeats within 0.05 ms; round 15's kernels in the same job: 34.25 / 33.97 / 33.72 / 34.52 / 35.96 and 17.24 / 17.12 / 17.00 / 17.42 / 18.09 — 2.5 beats 2.75 by 0.33 ms at 64 and 0.24 ms at 32 on the new kernels and loses 0.25 / 0.12 ms on the old ones; profiles/r16_notes.md; round 15, eight gather waves with queues of 256 entries, q_group_units 2: 64 x 1080p 34.18 / 33.93 / 33.66 / 34.42 ms for 2.25 / 2.5 / 2.75 / 3, 32: 17.20 / 17.06 / 16.95 for 2.25 / 2.5 / 2.75, repeats within 0.1 ms; four waves at 1.25: 34.33 and 17.30; profiles/r15_notes.md; round 13, four gather waves, the grid pass hands its units out by ticket and is 2.9 ms shorter: 64 x 1080p 35.96 / 35.53 / 35.05 / 35.74 / 36.91 ms for 0.75 / 1 / 1.25 / 1.5 / 1.75, repeats within 0.04 ms but for 1.5; 32: 18.14 / 17.88 / 17.88 / 18.18 / 18.71 — 1.25 beats 1 by 0.48 ms at 64 and is level with it at 32; round 12, first sweep on the round-11 tile shapes, members of a group without their end barrier: 64 x 1080p 36.68 / 36.23 / 35.97 / 37.72 / 38.07 ms for 0.5 / 0.75 / 1 / 1.25 / 1.5, 32: 18.34 / 18.16 / 18.21 / 18.95 / 19.15 — 1 beats 1.25 by 1.7 ms at 64 and 0.7 ms at 32, repeats within 0.05 ms but for one value at 32; 0.75 is level with 1 at 32 and 0.25 ms behind at 64; round 10, after the tail's transposed records: 64 x 1080p 38.58 / 38.24 / 38.86 / 40.04 ms for 1 / 1.25 / 1.5 / 1.75, 32: 19.33 / 19.38 / 19.46 / 20.23 — 1.25 beats 1.5 at both sizes by more than the 0.03 ms between repeats, 1 wins only at 32; round 8, wave-independent tile tail: 64 x 1080p 38.94 / 40.14 / 41.00 / 42.35 / 43.60 ms for 1.5 / 1.75 / 2 / 2.25 / 2.5, 32: 19.50 / 20.19 / 20.68 / 21.14 / 21.84; round 4, band-major queue pass: 64 x 1080p 43.6 / 43.0 / 42.5 / 43.4 / 44.5 ms for 1.5 / 1.75 / 2 / 2.25 / 2.5; round 3: (four gather waves; 64 x 1080p: 46.70 / 46.24 / 45.57 / 45.16 / 45.55 / 46.72 ms for 0.75 / 1 / 1.25 / 1.5 / 1.75 / 2; 32: 23.39 / 23.16 / 22.80 / 22.62 / 22.78 / 23.38)
    float tile_split_mid = 2.75f;       // 8 .. 31 frames (round 15, eight gather waves: 16 x 1080p 8.86 / 8.70 / 8.70 / 9.25 ms for 1.75 / 2.25 / 2.75 / 3.25, 8: 4.57 / 4.48 / 4.48 / 4.75; four waves: 9.35 and 4.90 at 1.75, 8.93 and 4.72 at 1.25; round 4, band-major queue pass: 16 x 1080p 11.53 / 11.36 / 11.13 / 11.01 / 10.89 / 10.90 ms for 0.75 ... 2.0; round 3: (16 x 1080p: 11.81 / 11.67 / 11.47 / 11.52 / 11.86 for 0.75 ... 1.75; 8: 6.03 / 5.95 / 5.97 / 6.24); 5 .. 7 frames (three gather waves): at most 0.5
    float tile_split_small = 0.0f;      // <= 4 frames
    int one_pass_max_frames = 0;        // calls of at most this many frames (of 720p and more, stump cascades) run the gather chain in ONE pass; 0: never.
                                        // Content decides which is faster (profiles/r04_notes.md #15: noise -6 %, drawn faces +1-7 %), so it is off by default
    // linear_stumps: a linear cascade of stumps, whose batches run eight gather waves.  Cascades of multi-node trees and stage trees keep
    // their wave counts and with them round 13's balance (1.75 / 1.25), unless tile_split was set by hand
    float split_for(int n_frames, bool linear_stumps) const {
        const float mid = linear_stumps || tile_split_set ? tile_split_mid : 1.75f, large = linear_stumps || tile_split_set ? tile_split : 1.25f;
        return n_frames <= 4 ? tile_split_small : n_frames < 8 ? std::min(mid, 0.5f) : n_frames < 32 ? mid : large;
    }
    // (the defaults are fractions of the last tile scale of a WHOLE pyramid; a share of the scales (vj_shard_scales) may end with a
    // scale of half a million windows: it starts without a move and lets the feedback find one)
    float split_for(int n_frames, const vj_params& p, bool linear_stumps) const {
        return ((p.scale_mask[0] | p.scale_mask[1]) != 0 && !tile_split_set) ? 0.0f : split_for(n_frames, linear_stumps);
    }
    int tile_segments = 1;              // stage trees: tiles run the chains after the prefix themselves
    int seg_cut2 = 0;                   // stage trees: a second cut inside a long chain after this many of its stages (0: none)
    int general_prefix = 1;             // stage trees: run their linear prefix on the linear kernels (0: one general pass)
    int grid_block_w = 32;              // width of the 2-D window blocks of the global-gather first pass (0: row runs)
    int tile_lds_reserve_kb = 16;       // LDS per CU the tile classes leave to the other chain (its 3-wave workgroup: 12 KiB + granule
                                        // rounding; with 14 the CU's 160 KiB do not take two class-0 blocks next to it any more)
    int roi_tile_min_windows = 512;   // region pass: (region, scale) grids of at least this many windows run on LDS tiles (0: never)
    int balance_class(int n_frames) const {
        return n_frames < 8 ? n_frames : n_frames < 16 ? 8 : n_frames < 32 ? 16 : n_frames < 64 ? 32 : 64;
    }
    bool auto_balance = true, tile_split_set = false;
    int plan_cache_max = 48;      // plans kept per environment; the least recently used one is released beyond that
                                  // (a stream of ROI sizes — eyes inside faces of any size — would otherwise grow
                                  // device tables without bound)
    int integral_rows_mode = 2;      // band_rows: 0 one wave walks a band's chunks, 1 the chunks of a band side by side, 2 side by side except for batches
    int blocks_per_cu = 8;
    int tile_class_kb[vj::TILE_CLASSES] = {-2, -1, 0};  // image-tile LDS budget per class in KiB; -k = what lets k
                                                     // workgroups share a CU's 160 KiB; all 0 disables the tile path
    int tile_min_windows = 768;   // a class is acceptable for a scale when a tile holds at least this many windows
    int tile_max_dwords_per_window = 600;  // staging a tile must stay far cheaper than gathering its windows from L2
    bool tile_thresholds_set = false;   // the three thresholds were configured: no per-frame-size defaults (get_plan)
    int tile_accept_windows = 768;  // scales whose best tile holds fewer windows stay on the global-gather path
    int tile_end = 64;            // tile launches never enter a pass that begins at or beyond this stage
    int tile_min_lanes = 0;       // a tile leaves at a pass boundary when fewer windows than this survive in it
    unsigned long long tile_repack_mask = ~3ull;  // stages (2 and later) before which a tile re-packs its survivors
    int tile_sp_begin = 3;        // first stage at which a tile may switch to the wave-split finish (>= 64: never)
    int tile_ws_max = 512;        // windows a tile may carry into the wave-split finish
    int tile_ws_min = 48;         // ... below this many the wave-independent tail takes over
    int group_max = (int)vj::GROUP_MAX;   // vj_detect_chain groups up to this many raw candidates of one frame on the device (more: host path)
    bool tree_split_queues = true; // stage trees: the grid pass's survivors go down the tree while the tiles still run
    bool cv_tiles = true;         // OpenCV profile: small scales of stump cascades on LDS tiles (vj_cv_tile.hip)
    int cv_tile_ws_max = 512;     // ... windows a tile carries into its wave-split finish
    int cv_row_blocks = -1;       // ... workgroups per CU of cv_profile_pass while it runs next to the tiles (their LDS budget shrinks with it);
                                  // -1: 2 for stump cascades (round 4: the row kernel's pair / stump-parallel forms need fewer waves), 3 for multi-node trees
    int cv_row_blocks_tree = 2, cv_tile_min_windows_tree = 256;   // ... the same two for stage trees (swept: profiles/r03_cv_sweeps.log)
    int cv_tail_max = 64;             // ... a population of at most this many windows evaluates a stage stump-parallel (<= 64)
    int cv_tree_chunk = 64, cv_tree_chain_blocks = 2;   // ... windows per chunk and workgroups per CU of cv_tree_chain_pass
    bool cv_tiles_tilted = true;      // ... cascades with tilted features on LDS tiles too (the tilted integral's tile staged behind the sum's)
    bool cv_tree2 = true;             // ... cascades of two-node trees: the row kernel fetches both nodes of a tree at once
    int cv_row_band_px = 128;         // ... the row kernel's rows in band-major order, bands of this many pixels (0: scale after scale)
    bool cv_tree_chains = true;       // ... stage trees made of chains: compacting chain sweeps (0: the per-lane target-stage walk)
    int cv_tree_queue_cap = 0;        // ... stage trees: capacity of the prefix survivors' queue (0: a quarter of the tile windows)
    int cv_tile_min_windows0 = 2048;   // ... the same for the class with two tile workgroups per CU
    int cv_tile_min_windows = -1;     // ... a scale goes to tiles when a tile of at least this many windows fits the LDS (-1: 2048 for stump cascades, 1536 for trees)
    bool rois_on_device = true;   // vj_detect_rois: one region pass on the frames' integral images (0: one vj_detect per region size)
    int wide_tail = -1;           // queue passes: several windows in flight in the stump-parallel tail (-1: batches of <= 4 frames)
    int min_chunk = 32;           // queue passes: smallest chunk of windows a wave draws when there are fewer than 64 per wave
    int q_band_px = 128;          // first-pass units of a frame are ordered by image band of this height (then scale), and the queue pass of a
                                  // batch draws groups of units band-major (0: scale-major units, chunk-by-chunk queue pass)
    int q_group_units = 4;        // ... units of 512 windows per group; shorter units (more than four gather waves) form groups of as many windows:
                                  // 4 x 512 / 256 = 2 units at eight waves (round 15, units in a group at eight waves: 64 x 1080p 34.39 / 33.98 / 34.21 /
                                  // 34.45 ms for 1 / 2 / 3 / 4 at tile_split 2.5, 8 loses 0.9 ms.  Round 4, 512-entry queues: 2-4 equal, 5 / 6 / 8 / 16
                                  // lose 0.5 / 1 / 2-3 / 3-7 ms of 42.5)
    int q_band_min_frames = 8;    // ... batches of at least this many frames (a single frame keeps the thin-pass machinery)
    int q_slices = -1;            // queue passes: slices of a part handed out frame-major (-1: one per frame of the part's frame group)
    int sp_tail_max = 48;         // global-gather sweeps switch to the stump-parallel tail when a wave holds at most this many windows (0: never;
                                  // a launch clamps it to what its queues hold: gather_tail_max)
    int gather_pairs = -1;        // global-gather sweeps evaluate two stumps per step, all their gathers in flight together: 0 never, 1 for
                                  // waves that hold a single chunk, 2 always, -1 = by batch size: 2 up to 4 frames (a single frame is bound
                                  // by the LATENCY of thin waves walking 16 stages: queue pass 0.78 -> 0.64 ms), 0 beyond (a faster gather chain
                                  // only takes issue slots from the tile chain: 64 x 1080p 47.98 / 48.21 / 49.21 ms for 0 / 1 / 2)
    uint32_t pairs_for(int n_frames) const { return gather_pairs >= 0 ? (uint32_t)gather_pairs : n_frames <= 4 ? 2u : 0u; }
    std::vector<int> split_override;
    std::vector<int> pass_cut_nodes{35};    // default pass cuts, in cumulative nodes (profiles/r03_notes.md #6c: 35 beats 150 on four cascades)
};

}  // namespace vj
