// The planner of the clod profile: scale records, LDS tile shapes and groups, node tables, stage records, the chain-balance
// cut, gather units, pass bounds, tile lists and skip bitmaps of one (cascade, frame size, parameters, settings) — pure host
// index arithmetic that the kernels trust without bounds checks.  Nothing here touches a device: plan_clod fills a PlanHost
// and the PlanTables the driver uploads, one named step after the other, and the plan query (vj_plan_tiles) reads the same
// plan a call runs.  Compiled with -ffp-contract=off like vj_plan.cpp; re-entrant (no mutable statics).
#include "vj_clod_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <tuple>

namespace vj {

static constexpr uint32_t kSlackRows = 2;  // zero rows after row H (defined reads for the
                                           // one-column feature overshoot)

uint32_t frame_elems_for(int W, int H) {
    uint64_t e = (uint64_t)(W + 1) * (uint64_t)(H + 1 + kSlackRows);
    e = (e + 63u) & ~(uint64_t)63u;  // keep every frame 256-byte aligned
    return (uint32_t)e;
}

// What every entry point that takes a vj_params checks before it plans anything (vj_detect, vj_detect_rois,
// vj_detect_chain for both parameter sets, vj_stream_create, the plan query): the same VJ_ERR_ARG everywhere, so that no path
// can reach a kernel with a flag combination the plan does not describe (VJ_FLAG_GRID_F64 alone would give the region pass a
// position table its launcher never binds).
int check_params(const vj_params& p) {
    if (!(p.scale_factor > 1.0f)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    if ((p.flags & VJ_FLAG_SKIP_LIST) && (p.flags & VJ_FLAG_SKIP_ROW)) {
        set_error("VJ_FLAG_SKIP_LIST and VJ_FLAG_SKIP_ROW are two different loops of the reference: pick one");
        return VJ_ERR_ARG;
    }
    if ((p.flags & VJ_FLAG_GRID_F64) && !(p.flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW))) {
        set_error("VJ_FLAG_GRID_F64 names the block variant's two loops: combine it with VJ_FLAG_SKIP_ROW or VJ_FLAG_SKIP_LIST");
        return VJ_ERR_ARG;
    }
    return VJ_OK;
}

int tile_group_from_env() {
    const char* g = getenv("VJ_TILE_GROUP");
    return g ? std::max(1, std::min(atoi(g), (int)MAX_SCALES)) : TILE_GROUP_SHIPPED;
}

// One or two SMALL frames per call are bound by the latency of the gather chain (most of their scales are "large" for the
// batch thresholds: a 320 x 240 frame keeps two scales on tiles), and a tile with few windows is still far cheaper than
// the thin waves of the queue pass: 320 x 240 0.78 -> 0.46 ms with tiles of >= 64 windows, 640 x 480 0.80 -> 0.76 with
// >= 256 (tools/small_frames.py).  Batches keep the thresholds that make their tiles efficient (tools/many_small.py).
int small_frame_class(const Tunables& t, int W, int H, int n_frames) {
    if (t.tile_thresholds_set || n_frames > 2) return 0;
    const long long px = (long long)W * H;
    return px <= 115200 ? 2 : px <= 460800 ? 1 : 0;
}

TileThresholds thresholds_for(const Tunables& t, int small) {
    TileThresholds th{t.tile_min_windows, t.tile_accept_windows, t.tile_max_dwords_per_window};
    if (small == 2) th = TileThresholds{64, 64, 8000};
    else if (small == 1) th = TileThresholds{256, 256, 2000};
    else if (small == 3) th = TileThresholds{std::min(384, th.min_windows), std::min(384, th.accept_windows), th.max_dwords_per_window};
    return th;
}

static bool linear_stages(const StageProgram& prog, size_t s, size_t n_stages) {
    return prog.on_fail[s] == STAGE_REJECT && (prog.on_pass[s] == (int)s + 1 || (prog.on_pass[s] == STAGE_ACCEPT && s + 1 == n_stages));
}

// A linear cascade of stumps: the cascades whose batches run eight gather waves and the balance that goes with them
// (Tunables::gather_waves_for, split_for).
bool has_trees(const vj_cascade& c) {
    for (const auto& t : c.trees)
        if (t.n_nodes != 1) return true;
    return false;
}
bool linear_stumps(const vj_cascade& c) {
    if (has_trees(c)) return false;
    const StageProgram prog = build_stage_program(c);
    for (size_t s = 0; s < c.stages.size(); ++s)
        if (!linear_stages(prog, s, c.stages.size())) return false;
    return true;
}

// ---- cascade shape ----------------------------------------------------------------------------------------------------------

// What the cascade alone decides: the stage program, trees / tree2 / general, the sweep order (*order) and, where
// want_prefix asks for it, the linear prefix of a stage tree.  Refuses more than VJ_MAX_STAGES stages, tilted features
// without VJ_FLAG_TILTED_AS_UPRIGHT and stage links with a cycle.
static int cascade_shape(const vj_cascade& c, uint32_t flags, bool want_prefix, PlanHost* pl, std::vector<uint32_t>* order) {
    if ((int)c.stages.size() > VJ_MAX_STAGES) {
        set_error("cascade has %zu stages; at most %d are supported", c.stages.size(), VJ_MAX_STAGES);
        return VJ_ERR_LIMIT;
    }
    if (!(flags & VJ_FLAG_TILTED_AS_UPRIGHT))
        for (const auto& nd : c.nodes)
            if (nd.tilted) {
                set_error("the cascade has tilted features: the clod profile would evaluate them as upright rectangles like the reference "
                          "(clod.cpp:448-492 never reads the flag) — pass VJ_FLAG_TILTED_AS_UPRIGHT for that, or use vj_detect_opencv");
                return VJ_ERR_UNSUPPORTED;
            }
    pl->prog = build_stage_program(c);
    pl->trees = has_trees(c);
    if (pl->trees) {
        // two-node trees (frontalface_alt2): the tile kernel's wave-split finish knows this shape
        pl->tree2 = true;
        for (const auto& t : c.trees) {
            if (t.n_nodes != 2) { pl->tree2 = false; break; }
            const vj_node_desc& n0 = c.nodes[t.first_node];
            const vj_node_desc& n1 = c.nodes[t.first_node + 1];
            const int kids = (n0.left > 0) + (n0.right > 0);
            if (kids != 1 || (n0.left > 0 ? n0.left : n0.right) != 1 || n1.left > 0 || n1.right > 0) {
                pl->tree2 = false;
                break;
            }
        }
    }
    for (size_t s = 0; s < c.stages.size(); ++s) {
        if (!linear_stages(pl->prog, s, c.stages.size())) pl->general = true;
        pl->max_stage_nodes = std::max(pl->max_stage_nodes, pl->prog.n_nodes[s]);
    }
    // Topological order of the pass/fail graph rooted at stage 0: the general path sweeps the stages once in it.
    if (!stage_sweep_order(pl->prog, order)) {
        set_error("stage links form a cycle");
        return VJ_ERR_UNSUPPORTED;
    }
    pl->n_order = (uint32_t)order->size();
    if (pl->general && want_prefix) {
        // the linear head of a stage tree (frontalface_alt_tree: stages 0..4 before the two chains split)
        uint32_t P = 0;
        while (P + 1 < order->size() && (*order)[P] == P && pl->prog.on_fail[P] == STAGE_REJECT &&
               pl->prog.on_pass[P] == (int)(P + 1) && (*order)[P + 1] == P + 1)
            ++P;
        if (P >= 2) pl->general_prefix = P;
    }
    return VJ_OK;
}

// ---- one scale --------------------------------------------------------------------------------------------------------------

// How far the rectangles of a frame-stride record table read from a window origin: the furthest element, and the
// furthest column / row (the third rectangle only where the node has one).
struct Reach { uint32_t elems, x, y; };
static Reach table_reach(const NodeRec* recs, size_t n, uint32_t stride) {
    Reach r{0, 0, 0};
    for (size_t k = 0; k < n; ++k) {
        const NodeRec& nr = recs[k];
        const uint32_t dw[3] = {nr.dw01 & 0xffffu, nr.dw01 >> 16, nr.dw2_flags & 0xffffu};
        for (int q = 0; q < 3; ++q)
            if (q < 2 || nr.w[2] != 0.0f) {
                const uint32_t lt = nr.lt[q] / 4u;
                r.elems = std::max(r.elems, (nr.lt[q] + nr.dh[q] + dw[q]) / 4u);
                r.x = std::max(r.x, lt % stride + dw[q] / 4u);
                r.y = std::max(r.y, lt / stride + (nr.dh[q] / 4u) / stride);
            }
    }
    return r;
}

// The record of one accepted scale but for its tile fields, its frame-stride node table and, under VJ_FLAG_GRID_F64, its
// window positions.  *reach: the furthest element any gather of the scale can touch, relative to the frame's start, and how
// far right / down of a window origin its features and variance rectangle read.
static int scale_record(const vj_cascade& c, int W, const vj_scale_info& si, uint32_t pos_mode, bool sq32, PlanTables* tab, ScaleDev* out, Reach* reach) {
    const uint32_t stride = (uint32_t)W + 1u;
    const size_t n_nodes = c.nodes.size();
    ScaleDev& sd = *out;
    memset(&sd, 0, sizeof(sd));
    sd.step = si.step;
    sd.nx = (uint32_t)si.nx;
    sd.ny = (uint32_t)si.ny;
    sd.nwin = (uint32_t)si.nx * (uint32_t)si.ny;
    sd.e_lt = (uint32_t)si.equ_y * stride + (uint32_t)si.equ_x;
    sd.e_dw = (uint32_t)si.equ_w;
    sd.e_dh = (uint32_t)si.equ_h * stride;
    sd.area = (float)si.area;
    sd.table_first = (uint32_t)tab->table.size();
    sd.scale_idx = (uint32_t)si.scale_idx;
    sd.scale_f = si.scale;
    sd.win_w = (uint32_t)si.win_w;
    sd.win_h = (uint32_t)si.win_h;
    sd.sq32 = sq32 && (uint64_t)sd.win_w * sd.win_h <= SQ32_MAX_AREA ? 1u : 0u;
    // (the u32 layout of the squared integral: a larger window's variance rectangle in strips whose squared sums fit a dword)
    sd.sq_strip = sd.sq32 ? 0u : sq_strip_rows(sd.e_dw) * stride;
    tab->table.resize(tab->table.size() + n_nodes);
    int rc = build_node_table(c, W, si, tab->table.data() + sd.table_first);
    if (rc) return rc;
    // (positions are lrint(i * step); the other roundings of window_pos differ by at most one: one more covers them)
    const uint32_t x_max = (uint32_t)std::lrint((double)((float)(si.nx - 1) * si.step)) + (pos_mode != 0u ? 1u : 0u);
    const uint32_t y_max = (uint32_t)std::lrint((double)((float)(si.ny - 1) * si.step)) + (pos_mode != 0u ? 1u : 0u);
    const Reach features = table_reach(tab->table.data() + sd.table_first, n_nodes, stride);
    reach->elems = std::max(sd.e_lt + sd.e_dh + sd.e_dw, features.elems) + y_max * stride + x_max;
    reach->x = std::max((uint32_t)(si.equ_x + si.equ_w), features.x);
    reach->y = std::max((uint32_t)(si.equ_y + si.equ_h), features.y);
    if (pos_mode & 2u) {
        // the block variant's positions, index by index, with the reference's own expressions: lrint(index * step) in
        // its row loop (clod.cpp:941-942), round(index * step) in its per-stage lists (:1034), `step` a double (:862)
        if (tab->pos_tab.empty()) tab->pos_tab.push_back(0u);   // (base 0 means "no table")
        sd.pos_base = (uint32_t)tab->pos_tab.size();
        const double stepd = std::max(2.0, (double)si.scale);
        const int n_pos = std::max(si.nx, si.ny) + 1;
        for (int i = 0; i < n_pos; ++i)
            tab->pos_tab.push_back((pos_mode & 1u) ? (uint32_t)std::round((double)i * stepd) : (uint32_t)std::lrint((double)i * stepd));
    }
    return VJ_OK;
}

// ---- tile shape search ------------------------------------------------------------------------------------------------------

// LDS of a CU the tile classes may fill, and of that the image tile of one workgroup of class `cls` (header_bytes in front of
// it).  2 KiB of the CU's share stay free so that the nested class blocks (nest_class_lds) can be rounded up to whole
// allocation granules.
static uint32_t tile_lds_per_cu(const Tunables& t) { return (160u - (uint32_t)t.tile_lds_reserve_kb) * 1024u; }
static uint64_t class_budget(const Tunables& t, uint32_t cls, uint32_t header_bytes) {
    const int kb = t.tile_class_kb[cls];
    return kb < 0 ? ((tile_lds_per_cu(t) - 2048u) / (uint32_t)(-kb) - header_bytes) & ~63ull
                  : std::min<uint64_t>((uint64_t)kb * 1024u, 160u * 1024u - header_bytes);
}

struct TileShape { uint32_t cls, tw, th, pitch, rows; };
// LDS-tile path: the class and shape of a tw x th window tile for a scale of this step and reach.  Per class the shape with
// the most windows that fits wins (the kernel maps a tile-local index to (t / tw, t % tw): any width does); false when the best
// tile holds fewer than accept_windows windows — the scale stays on the global-gather path.
// The budget is what a launch allocates in front of the image tile, TILE_LDS_HEADER: the wave-independent tail needs no LDS
// beyond it (its survivor and verdict areas lie in the queue area).  former_shapes restates the search as it was before round 11
// for the plan dump (tools/plan_dump.py): the budget also lost the tables of the former stump-parallel finish (8 992 bytes for
// frontalface_alt: plans with the wave-independent tail, by the nodes of their widest stage) which no launch allocated any more,
// the candidate lists were coarser and the widest shape won a tie.
static bool search_tile_shape(const Tunables& t, const TileThresholds& thresholds, float step, uint32_t reach_x, uint32_t reach_y,
                              bool former_shapes, bool wave_tail, uint32_t max_stage_nodes, TileShape* out) {
    static const uint32_t kTw[] = {64, 56, 48, 40, 32, 24, 16, 12, 8}, kTh[] = {32, 28, 24, 20, 16, 12, 8, 6, 4};
    auto former = [&](uint32_t v) { return former_shapes && (v == 56u || v == 40u || v == 28u || v == 20u); };
    uint32_t header_bytes = TILE_LDS_HEADER;
    if (former_shapes && wave_tail) header_bytes += ((2u * 14u * (TILE_SP_BLOCK + 1u) + 2u * max_stage_nodes + 3u) & ~3u) * 4u;
    uint32_t best_n = 0;
    TileShape best{TILE_CLASSES, 0, 0, 0, 0};
    for (uint32_t cls = 0; cls < TILE_CLASSES && best_n < (uint32_t)thresholds.min_windows; ++cls) {
        const uint64_t budget = class_budget(t, cls, header_bytes);
        for (uint32_t tw : kTw)
            for (uint32_t th : kTh) {
                const uint32_t nwt = tw * th;
                if (nwt > TILE_WAVES * TILE_WAVE_CAP || nwt < 64 || nwt < best_n || (nwt == best_n && best.cls != cls)) continue;
                if (former(tw) || former(th)) continue;
                // rows staged 16 bytes per lane (not the de-interleaved step-2 tiles, whose sources are 8 bytes
                // apart): pitch a multiple of 4 dwords, not of 32 (rows would share banks); step 2: an odd pitch
                uint32_t pitch = (uint32_t)std::ceil((double)(tw - 1) * (double)step) + 3u + reach_x;
                if (step != 2.0f) {
                    pitch = (pitch + 3u) & ~3u;
                    if (pitch % 32u == 0u) pitch += 4u;
                } else {
                    pitch |= 1u;
                }
                const uint32_t rows = (uint32_t)std::ceil((double)(th - 1) * (double)step) + 3u + reach_y;
                if ((uint64_t)pitch * rows * 4u > budget) continue;
                // staging a tile must stay far cheaper than gathering its windows from L2
                if ((uint64_t)pitch * rows > (uint64_t)thresholds.max_dwords_per_window * nwt) continue;
                // as many windows as the best so far: the shape that stages fewer dwords (else the wider one stays)
                if (nwt == best_n && (former_shapes || pitch * rows >= best.pitch * best.rows)) continue;
                best_n = nwt;
                best = TileShape{cls, tw, th, pitch, rows};
            }
    }
    // (best_n == 0: no shape fits any class — with tile_accept_windows 0 that scale once became a tile scale of a 0 x 0 tile,
    // and tiles_x divided by zero)
    if (best_n == 0u || best_n < (uint32_t)thresholds.accept_windows) return false;
    *out = best;
    return true;
}

// A scale's records in the layout of the staged tile its group shares, `pitch` dwords per row (half != 0: de-interleaved,
// vj_plan.cpp), appended to the table, and its variance rectangle in that layout: the scale's grp_* fields.
static int add_group_table(const vj_cascade& c, const vj_scale_info& si, uint32_t pitch, uint32_t half, std::vector<NodeRec>* table, ScaleDev* sd) {
    sd->grp_table_first = (uint32_t)table->size();
    table->resize(table->size() + c.nodes.size());
    const int rc = build_node_table_stride(c, pitch, si, table->data() + sd->grp_table_first, half);
    if (rc) return rc;
    sd->grp_te_lt = (uint32_t)si.equ_y * pitch + deint_col((uint32_t)si.equ_x, half);
    sd->grp_te_dw = (int32_t)deint_col((uint32_t)(si.equ_x + si.equ_w), half) - (int32_t)deint_col((uint32_t)si.equ_x, half);
    sd->grp_te_dh = (uint32_t)si.equ_h * pitch;
    return VJ_OK;
}

// The tile fields of a scale that goes to tiles in `shape`, and its records in the tile's own layout: so far a group of one.
static int lay_out_tile(const vj_cascade& c, const vj_scale_info& si, const TileShape& shape, std::vector<NodeRec>* table, ScaleDev* sd) {
    sd->tile_rw = 1;
    sd->tile_tw = shape.tw;
    sd->tile_th = shape.th;
    sd->tile_pitch = shape.pitch;
    sd->tile_rows = shape.rows;
    sd->tile_class = shape.cls;
    // step exactly 2: every window origin is an even column -> de-interleave the tile rows
    sd->tile_half = si.step == 2.0f ? (sd->tile_pitch + 1u) / 2u : 0u;
    if (getenv("VJ_DEBUG_PLAN"))
        fprintf(stderr, "vj plan: scale %d s=%.3f step=%.2f nx=%u ny=%u class %u tile %ux%u = %u windows, pitch %u rows %u (%u B)%s\n",
                si.scale_idx, si.scale, si.step, sd->nx, sd->ny, sd->tile_class, sd->tile_tw, sd->tile_th, sd->tile_tw * sd->tile_th,
                sd->tile_pitch, sd->tile_rows, sd->tile_pitch * sd->tile_rows * 4u, sd->tile_half ? " deinterleaved" : " x4");
    const int rc = add_group_table(c, si, sd->tile_pitch, sd->tile_half, table, sd);
    if (rc) return rc;
    sd->tile_table_first = sd->grp_table_first;
    sd->te_lt = sd->grp_te_lt;
    sd->te_dw = sd->grp_te_dw;
    sd->te_dh = sd->grp_te_dh;
    sd->tiles_x = (sd->nx + sd->tile_tw - 1) / sd->tile_tw;
    sd->tile_row_end = sd->ny;
    return VJ_OK;
}

// ---- tile groups ------------------------------------------------------------------------------------------------------------

// Scale groups: up to tile_group consecutive step-2 de-interleaved tile scales share ONE staged tile.  Their window
// origins lie on the same lattice (x = 2 ix, y = 2 iy), so the tile the group's largest scale lays out for itself (shape
// search: its windows reach furthest) holds every member's windows at the same tile-local offsets; each member
// gets a NodeRec table and equ_rect offsets in that pitch / half.  The members' own tile fields stay for the ROI pass.
// Returns the lead of every scale (itself when not grouped) in *tile_lead.
static int group_tile_scales(const vj_cascade& c, int tile_group, const std::vector<vj_scale_info>& scales_info,
                             const std::vector<std::pair<uint32_t, uint32_t>>& tile_reach, std::vector<ScaleDev>* scales,
                             std::vector<NodeRec>* table, std::vector<uint32_t>* tile_lead) {
    const uint32_t n = (uint32_t)scales->size();
    tile_lead->resize(n);
    for (uint32_t slot = 0; slot < n; ++slot) (*tile_lead)[slot] = slot;
    auto groupable = [&](uint32_t k) {
        const ScaleDev& sd = (*scales)[k];
        return sd.tile_rw != 0u && sd.tile_half != 0u && sd.step == 2.0f;
    };
    for (uint32_t g0 = 0; tile_group > 1 && g0 < n;) {
        if (!groupable(g0)) { ++g0; continue; }
        // members in scale order, as long as the reach does not shrink (the last member's tile then covers them all)
        uint32_t g1 = g0 + 1;
        while (g1 < n && g1 - g0 < (uint32_t)tile_group && groupable(g1) &&
               tile_reach[g1].first >= tile_reach[g1 - 1].first && tile_reach[g1].second >= tile_reach[g1 - 1].second)
            ++g1;
        const uint32_t lead = g1 - 1;
        const ScaleDev& L = (*scales)[lead];
        for (uint32_t k = g0; k < lead; ++k) {
            const int rc = add_group_table(c, scales_info[k], L.tile_pitch, L.tile_half, table, &(*scales)[k]);
            if (rc) return rc;
            (*tile_lead)[k] = lead;
        }
        if (getenv("VJ_DEBUG_PLAN") && lead > g0)
            fprintf(stderr, "vj plan: scales %u..%u share the tile of scale %u\n", (*scales)[g0].scale_idx, L.scale_idx, L.scale_idx);
        g0 = g1;
    }
    return VJ_OK;
}

// ---- stage records ----------------------------------------------------------------------------------------------------------

// The stage records but for sp_first (tail_blocks), with the rounding bound of every stage's sum.
static std::vector<StageDev> stage_records(const vj_cascade& c, const StageProgram& prog, const std::vector<uint32_t>& order) {
    std::vector<StageDev> stages;
    for (size_t s = 0; s < c.stages.size(); ++s) {
        StageDev sd;
        memset(&sd, 0, sizeof(sd));
        sd.first_node = prog.first_node[s];
        sd.n_nodes = prog.n_nodes[s];
        sd.threshold = c.stages[s].threshold;
        sd.on_pass = prog.on_pass[s];
        sd.on_fail = prog.on_fail[s];
        sd.n_trees = (uint32_t)c.stages[s].n_trees;
        sd.order = s < order.size() ? order[s] : 0u;
        // rigorous bound on how far two summation orders of this stage's leaf values can differ:
        // every order satisfies |fl_sum - exact| <= gamma_{n-1} * sum|a_k| (Higham), gamma_k = k u / (1 - k u),
        // u = 2^-24, and |a_k| <= max(|left_k|, |right_k|); the factor 4 (instead of 2) also covers the
        // rounding of the comparison itself
        double amax = 0.0;
        const vj_stage_desc& st = c.stages[s];
        for (int t = 0; t < st.n_trees; ++t) {
            const vj_tree_desc& td = c.trees[st.first_tree + t];
            double m = 0.0;
            for (int k = 0; k <= td.n_nodes; ++k) m = std::max(m, (double)std::fabs(c.alpha[td.first_alpha + k]));
            amax += m;
        }
        const double n = (double)prog.n_nodes[s];
        sd.sp_delta = (float)(4.0 * n * std::ldexp(1.0, -24) * amax * 1.001 + 1e-30);
        stages.push_back(sd);
    }
    return stages;
}

// ---- tail blocks ------------------------------------------------------------------------------------------------------------

// Blocks of <= 64 consecutive nodes per stage, balanced, for the wave-independent tail of the tile kernel; every stage record
// gets the index of its first block.
static std::vector<SpBlock> tail_blocks(const StageProgram& prog, std::vector<StageDev>* stages) {
    std::vector<SpBlock> sp_blocks;
    for (size_t s = 0; s < stages->size(); ++s) {
        const uint32_t S = prog.n_nodes[s], nb = (S + TILE_SP_BLOCK - 1u) / TILE_SP_BLOCK;
        (*stages)[s].sp_first = (uint32_t)sp_blocks.size();
        uint32_t jb = 0;
        for (uint32_t b = 0; b < nb && nb <= (uint32_t)TILE_SP_MAX_BLOCKS && s < 256; ++b) {
            const uint32_t jn = S / nb + (b < S % nb ? 1u : 0u);
            sp_blocks.push_back(SpBlock{prog.first_node[s] + jb, jn | (jb << 8) | (b << 16) | (nb << 20) | ((uint32_t)s << 24)});
            jb += jn;
        }
    }
    return sp_blocks;
}

// The tail's own copy of the tile tables (TILE_TAIL_BLOCK_RECS): per table and block, the 14 dwords of the block's records
// transposed into four lane-contiguous pieces.  The fields are the table's; only their place differs.  (The gather chain's
// stump-parallel tail reads frame-stride tables in blocks of its own: it keeps the record form.)
static void transpose_tail_tables(const std::vector<SpBlock>& sp_blocks, std::vector<ScaleDev>* scales, std::vector<NodeRec>* table) {
    auto emit_tail = [&](uint32_t table_first) {
        const uint32_t tail_first = (uint32_t)table->size();
        table->resize(table->size() + sp_blocks.size() * (size_t)TILE_TAIL_BLOCK_RECS);   // (zeroed: the padding records)
        for (size_t x = 0; x < sp_blocks.size(); ++x) {
            uint32_t* blk = reinterpret_cast<uint32_t*>(table->data() + tail_first + x * (size_t)TILE_TAIL_BLOCK_RECS);
            const uint32_t jn = sp_blocks[x].desc & 0xffu;
            for (uint32_t j = 0; j < jn; ++j) {
                const uint32_t* rec = reinterpret_cast<const uint32_t*>(&(*table)[table_first + sp_blocks[x].first_node + j]);
                for (uint32_t d = 0; d < 12u; ++d) blk[(d / 4u) * 4u * TILE_SP_BLOCK + j * 4u + d % 4u] = rec[d];
                for (uint32_t d = 12u; d < 14u; ++d) blk[12u * TILE_SP_BLOCK + j * 2u + (d - 12u)] = rec[d];
            }
        }
        return tail_first;
    };
    for (ScaleDev& sd : *scales) {
        if (!sd.tile_rw) continue;
        sd.tile_tail_first = emit_tail(sd.tile_table_first);
        sd.grp_tail_first = sd.grp_table_first == sd.tile_table_first ? sd.tile_tail_first : emit_tail(sd.grp_table_first);
    }
}

// ---- chain-balance cut ------------------------------------------------------------------------------------------------------

// Balance between the two chains: tile_split scales' worth of tile work (counted from the largest tile
// scale down, fractions by window rows) moves to the global-gather chain, which overlaps the tile chain.
static void cut_tile_rows(float tile_split, const std::vector<uint32_t>& tile_lead, std::vector<ScaleDev>* scales) {
    double remaining = std::max(0.0, (double)tile_split);
    for (size_t k = scales->size(); k-- > 0 && remaining > 0.0;) {
        ScaleDev& sd = (*scales)[k];
        if (!sd.tile_rw) continue;
        const double move = std::min(1.0, remaining);
        remaining -= move;
        const uint32_t keep_rows = (uint32_t)((double)sd.ny * (1.0 - move));
        const uint32_t th = (*scales)[tile_lead[k]].tile_th;   // (the group's tile rows)
        sd.tile_row_end = keep_rows / th * th;
    }
}

// ---- gather units -----------------------------------------------------------------------------------------------------------

// First-pass units of the global-gather path: whole scales, and the rows of split scales the tiles leave, in 2-D blocks of
// <= unit_cap windows (what a wave's queue holds at the plan's wave count): a compact footprint in the sum image per wave (a
// row run of 512 windows drags a full-width band of 20 s rows through the L2).
static int gather_units(const Tunables& t, const std::vector<ScaleDev>& scales, uint32_t unit_cap, std::vector<UnitDev>* units) {
    for (uint32_t slot = 0; slot < scales.size(); ++slot) {
        const ScaleDev& sd = scales[slot];
        const uint32_t row0 = sd.tile_row_end;
        if (row0 >= sd.ny) continue;
        gather_cut_units(sd.nx, sd.ny, row0, (uint32_t)std::max(0, t.grid_block_w), unit_cap,
                         [&](uint32_t first, uint32_t count, uint32_t bw) { units->push_back(UnitDev{slot, first, count, bw}); });
    }
    for (const UnitDev& u : *units)
        if (u.count > unit_cap) {
            set_error("internal error: a first-pass unit of %u windows for queues of %u", u.count, unit_cap);
            return VJ_ERR_LIMIT;
        }
    return VJ_OK;
}

// Band-major order: the units of a frame sorted by the image band their top row lies in, then by scale — the waves of an
// XCD (which take a contiguous run of the (frame, unit) list) then gather from ONE band of the sum image across all scales
// instead of sweeping the frame once per scale — and, for the queue pass, groups of consecutive units of one (band, scale).
static void order_units_by_band(const Tunables& t, const std::vector<ScaleDev>& scales, uint32_t unit_cap, std::vector<UnitDev>* units,
                                std::vector<UnitDev>* unit_groups) {
    auto band_of = [&](const UnitDev& u) {
        const ScaleDev& sd = scales[u.scale];
        const uint32_t iy0 = u.bw != 0u ? (u.first >> 16) : u.first / std::max(1u, sd.nx);
        return (uint32_t)std::lrint((double)((float)iy0 * sd.step)) / (uint32_t)t.q_band_px;
    };
    std::vector<std::pair<uint32_t, UnitDev>> keyed;
    keyed.reserve(units->size());
    for (const UnitDev& u : *units) keyed.push_back({band_of(u), u});
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a, const auto& b) {
        return std::make_tuple(a.first, a.second.scale) < std::make_tuple(b.first, b.second.scale);   // (stable: blocks stay row-major inside)
    });
    // (q_group_units counts units of UNIT_WINDOWS windows: a plan with shorter units groups as many windows)
    const uint32_t G = std::max<uint32_t>(1u, (uint32_t)std::max(1, t.q_group_units) * unit_cap / (uint32_t)UNIT_WINDOWS);
    for (size_t i = 0; i < keyed.size(); ++i) {
        (*units)[i] = keyed[i].second;
        if (unit_groups->empty() || unit_groups->back().bw != keyed[i].first || unit_groups->back().scale != keyed[i].second.scale ||
            unit_groups->back().count >= G)
            unit_groups->push_back(UnitDev{keyed[i].second.scale, (uint32_t)i, 0u, keyed[i].first});
        ++unit_groups->back().count;
    }
}

// ---- pass bounds ------------------------------------------------------------------------------------------------------------

// Default pass split: stage boundaries after which the survivor population is small
// enough that re-packing it across the whole device pays for the extra launch.
static std::vector<uint32_t> default_pass_bounds(const vj_cascade& c, const StageProgram& prog,
                                                 const std::vector<int>& override_, const std::vector<int>& cut_nodes) {
    const uint32_t n = (uint32_t)c.stages.size();
    std::vector<uint32_t> b{0};
    if (!override_.empty()) {
        for (int v : override_)
            if (v > (int)b.back() && v < (int)n) b.push_back((uint32_t)v);
    } else {
        // cuts after given numbers of cumulative nodes (default: one, after 35 — frontalface_alt: before stage 3 —
        // measured best on batches of four cascades: [0,3) global first pass, one queue pass for the rest whose chunks hold
        // the survivors of the whole batch re-packed, both on the global-gather chain while the tile chain runs the whole
        // cascade next to it; round 1 cut after ~150 nodes, which the frame-major chunk order of round 3 made too late)
        uint32_t acc = 0;
        size_t ci = 0;
        for (uint32_t s = 0; s < n && ci < cut_nodes.size(); ++s) {
            acc += prog.n_nodes[s];
            if (acc >= (uint32_t)cut_nodes[ci] && s + 1 < n) {
                b.push_back(s + 1);
                while (ci < cut_nodes.size() && acc >= (uint32_t)cut_nodes[ci]) ++ci;
            }
        }
    }
    b.push_back(n);
    while (b.size() > (size_t)VJ_MAX_PASSES + 1) b.erase(b.end() - 2);  // at most VJ_MAX_PASSES launches
    return b;
}

// Can the part of a stage tree after its linear prefix be cut into linear segments?  A segment is a run of positions of
// the sweep order whose pass edges follow the order, whose rejects all go to the first position of a LATER segment (or are
// final), and whose end accepts.  Then the passes are the prefix and every segment in two or three parts (pass_bounds,
// seg_last, seg_fail), and where every segment's rejects feed the next one the tile kernel runs the chains itself (tile_seg_*);
// else the plan keeps its one general pass after the prefix.
static void segment_stage_tree(const StageProgram& prog, const std::vector<uint32_t>& order, int seg_cut2, PlanHost* pl) {
    struct Seg { uint32_t b, e; int fail_pos; };
    std::vector<Seg> segs;
    std::vector<int> pos_of(prog.on_pass.size(), -1);
    for (uint32_t i = 0; i < pl->n_order; ++i) pos_of[order[i]] = (int)i;
    bool ok = true;
    uint32_t b = pl->general_prefix;
    while (b < pl->n_order && ok) {
        const int f = prog.on_fail[order[b]];
        uint32_t e2 = b;
        while (true) {
            const uint32_t sid = order[e2];
            if (prog.on_fail[sid] != f) { ok = false; break; }
            const int np = prog.on_pass[sid];
            ++e2;
            if (np == STAGE_ACCEPT) break;
            if (e2 >= pl->n_order || np != (int)order[e2]) { ok = false; break; }
        }
        if (!ok) break;
        segs.push_back(Seg{b, e2, f == STAGE_REJECT ? -1 : pos_of[f]});
        b = e2;
    }
    for (const Seg& sg : segs)   // a reject target must be the start of a later segment
        if (sg.fail_pos >= 0) {
            bool found = false;
            for (const Seg& t : segs) found |= t.b == (uint32_t)sg.fail_pos && t.b >= sg.e;
            ok &= found;
        }
    // passes: the prefix, then every segment in two parts (its first stages see most of its windows)
    std::vector<uint32_t> bounds{0u, pl->general_prefix};
    std::vector<uint8_t> last{0}, failq{0};   // index = pass; entry 0 = the prefix pass
    std::vector<int> seg_first_pass;
    for (const Seg& sg : segs) {
        seg_first_pass.push_back((int)bounds.size() - 1);
        // cuts inside a chain: after its third stage (most of its windows are gone by then) and, when the chain is
        // long and launches are left, once more after its seg_cut2-th — the survivors are re-packed device-wide at
        // every cut instead of riding on in thin waves
        const uint32_t cut = sg.e - sg.b > 4 ? sg.b + 3 : sg.e;
        if (cut < sg.e) { bounds.push_back(cut); last.push_back(0); failq.push_back(0); }
        const uint32_t cut2 = seg_cut2 > 3 && sg.e - sg.b > (uint32_t)seg_cut2 + 4u && bounds.size() + 2 * (segs.size() - seg_first_pass.size()) + 1 < (size_t)VJ_MAX_PASSES
                                  ? sg.b + (uint32_t)seg_cut2 : sg.e;
        if (cut2 < sg.e) { bounds.push_back(cut2); last.push_back(0); failq.push_back(0); }
        bounds.push_back(sg.e); last.push_back(1); failq.push_back(0);
    }
    if (!ok || segs.empty() || bounds.size() - 1 > (size_t)VJ_MAX_PASSES) return;
    for (size_t k = 0; k < segs.size(); ++k) {
        if (segs[k].fail_pos < 0) continue;
        int target_pass = -1;
        for (size_t t = 0; t < segs.size(); ++t)
            if (segs[t].b == (uint32_t)segs[k].fail_pos) target_pass = seg_first_pass[t];
        const int p_end = k + 1 < segs.size() ? seg_first_pass[k + 1] : (int)bounds.size() - 1;
        for (int ps = seg_first_pass[k]; ps < p_end; ++ps) failq[(size_t)ps] = (uint8_t)target_pass;
    }
    pl->pass_bounds = bounds;
    pl->seg_last = last;
    pl->seg_fail = failq;
    bool chain_ok = segs.size() <= 4;
    for (size_t k = 0; k < segs.size() && chain_ok; ++k)
        if (segs[k].fail_pos >= 0 && (k + 1 >= segs.size() || segs[k + 1].b != (uint32_t)segs[k].fail_pos)) chain_ok = false;
    if (chain_ok) {
        pl->tile_n_seg = (uint32_t)segs.size();
        for (size_t k = 0; k < segs.size(); ++k) {
            pl->tile_seg_end[k] = segs[k].e;
            if (segs[k].fail_pos >= 0) pl->tile_seg_chain |= 1u << k;
        }
    }
}

// The passes of the gather chain (linear cascades: stage indices; stage trees: positions in StageDev::order,
// [linear prefix | the rest]) and the stage at which the tile launches stop.
static void plan_passes(const Tunables& t, const vj_cascade& c, const std::vector<uint32_t>& order, bool one_pass, PlanHost* pl) {
    pl->pass_bounds = default_pass_bounds(c, pl->prog, t.split_override, t.pass_cut_nodes);
    // A call of a few frames may run the gather chain in ONE pass (one_pass_max_frames; the first pass runs every stage, thin waves finishing
    // stump-parallel): one dependent launch fewer — a noise frame at 1080p 1.23 -> 1.15 ms, a 4096 x 4096 one 7.81 -> 7.02 — but frames with
    // many deep survivors (blocks, drawn faces) lose as much without the queue pass's re-packing (profiles/r04_notes.md #15): off by default
    // (stump cascades: a tree cascade's thin waves have no stump-parallel form and lose — frontalface_alt2, one 1080p frame, 1.30 -> 1.41 ms)
    if (one_pass && !pl->general && !pl->trees && t.split_override.empty()) pl->pass_bounds = {0u, (uint32_t)c.stages.size()};
    if (pl->general) {
        if (pl->general_prefix) pl->pass_bounds = {0u, pl->general_prefix, pl->n_order};
        else pl->pass_bounds = {0u, pl->n_order};
        if (pl->general_prefix) segment_stage_tree(pl->prog, order, t.seg_cut2, pl);
    }
    // tile launches run deeper than the global-gather first pass (LDS gathers are ~10x cheaper)
    pl->tile_end = std::min<uint32_t>((uint32_t)c.stages.size(), std::max<uint32_t>((uint32_t)t.tile_end, pl->pass_bounds[1]));
    if (pl->pass_bounds.size() == 2) pl->tile_end = pl->pass_bounds[1];
}

// ---- tile lists -------------------------------------------------------------------------------------------------------------

// The tiles of one frame class by class (a group's tiles once, under its first member) and the dynamic LDS of every class launch.
static void tile_lists(PlanHost* pl) {
    for (uint32_t cls = 0; cls < TILE_CLASSES; ++cls) {
        pl->class_first[cls] = (uint32_t)pl->tile_units.size();
        for (uint32_t slot = 0; slot < pl->scales.size(); ++slot) {
            const uint32_t lead = pl->tile_lead[slot];
            const ScaleDev& L = pl->scales[lead];
            if (!pl->scales[slot].tile_rw || L.tile_class != cls || (slot > 0 && pl->tile_lead[slot - 1] == lead)) continue;
            // a group's tiles cover the union of its members' tile rows; a member skips the tiles past its own
            // tile_row_end (rows the balance gave to the gather chain) and past its own grid edge
            uint32_t row_end = 0, nx = 0;
            for (uint32_t k = slot; k <= lead; ++k) {
                row_end = std::max(row_end, pl->scales[k].tile_row_end);
                nx = std::max(nx, pl->scales[k].nx);
            }
            for (uint32_t iy0 = 0; iy0 < row_end; iy0 += L.tile_th)
                for (uint32_t ix0 = 0; ix0 < nx; ix0 += L.tile_tw)
                    pl->tile_units.push_back(UnitDev{slot, ix0 | (iy0 << 16), lead > slot ? lead - slot + 1u : 0u, 0});
            pl->class_lds[cls] = std::max(pl->class_lds[cls], L.tile_pitch * L.tile_rows * 4u);
        }
        // the region pass lays a scale's tile out in the scale's OWN shape and launches with this class's block: a group
        // member's own shape may be larger than the shape of the lead it follows on the frame's tile list
        for (const ScaleDev& sd : pl->scales)
            if (sd.tile_rw && sd.tile_class == cls && pl->class_lds[cls])
                pl->class_lds[cls] = std::max(pl->class_lds[cls], sd.tile_pitch * sd.tile_rows * 4u);
        if (pl->class_lds[cls]) pl->class_lds[cls] += TILE_LDS_HEADER;
    }
    pl->class_first[TILE_CLASSES] = (uint32_t)pl->tile_units.size();
}

// Nest the LDS blocks of consecutive classes: the tile launches follow each other on CUs where the gather
// chain's workgroup holds a block somewhere in the middle of the LDS, so the k workgroups of one class have to
// fit exactly into the hole the workgroup(s) of the other class leave behind (measured: a class-0 pair 2 KB
// larger than the class-1 block it follows leaves one tile workgroup per CU idle, + 17 % on that launch).
static void nest_class_lds(const Tunables& t, uint32_t class_lds[TILE_CLASSES]) {
    for (uint32_t cls = 0; cls + 1 < TILE_CLASSES; ++cls) {
        const int ka = t.tile_class_kb[cls], kb = t.tile_class_kb[cls + 1];
        if (ka >= 0 || kb >= 0 || !class_lds[cls] || !class_lds[cls + 1]) continue;
        const uint32_t na = (uint32_t)(-ka), nb = (uint32_t)(-kb);   // workgroups per CU: na > nb
        if (na <= nb || na % nb != 0u) continue;
        const uint32_t ratio = na / nb;
        uint32_t big = std::max(class_lds[cls + 1], ratio * class_lds[cls]);
        // whole allocation granules (the hardware hands LDS out in 512-byte granules; 1 KiB is safe)
        big = (big + ratio * 1024u - 1u) / (ratio * 1024u) * (ratio * 1024u);
        if ((uint64_t)big * nb > tile_lds_per_cu(t)) continue;
        class_lds[cls + 1] = big;
        class_lds[cls] = big / ratio;
    }
}

// ---- skip bitmaps -----------------------------------------------------------------------------------------------------------

// P2 skip modes: one bitmap word per 64 consecutive windows of a recurrence domain — a window row
// (VJ_FLAG_SKIP_ROW, clod.cpp:1430) or a scale's whole row-major list (VJ_FLAG_SKIP_LIST, clod.cpp:729-732).
// Returns the words of one frame's bitmap.
static uint32_t skip_bitmaps(uint32_t skip_mode, std::vector<ScaleDev>* scales, std::vector<UnitDev>* skip_units, std::vector<UnitDev>* skip_segs) {
    uint32_t word = 0;
    for (uint32_t slot = 0; slot < scales->size(); ++slot) {
        ScaleDev& sd = (*scales)[slot];
        sd.skip_base = word;
        if (skip_mode == VJ_FLAG_SKIP_ROW) {
            sd.skip_wpr = (sd.nx + 63u) / 64u;
            for (uint32_t iy = 0; iy < sd.ny; ++iy) {
                skip_segs->push_back(UnitDev{slot, word, sd.skip_wpr, 0});
                for (uint32_t ix0 = 0; ix0 < sd.nx; ix0 += 64u)
                    skip_units->push_back(UnitDev{slot, ix0 | (iy << 16), std::min<uint32_t>(64u, sd.nx - ix0), word++});
            }
        } else {
            sd.skip_wpr = 0;
            const uint32_t n_words = (sd.nwin + 63u) / 64u;
            skip_segs->push_back(UnitDev{slot, word, n_words, 0});
            for (uint32_t i0 = 0; i0 < sd.nwin; i0 += 64u)
                skip_units->push_back(UnitDev{slot, i0, std::min<uint32_t>(64u, sd.nwin - i0), word++});
        }
    }
    return word;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------

// Is scale k of the enumeration part of this plan?  (scale_mask: a subset of the scales, multi-GPU sharding of one frame)
static bool scale_selected(const vj_scale_info& si, const vj_params& p) {
    if (!si.accepted || si.nx <= 0 || si.ny <= 0) return false;
    if ((p.scale_mask[0] | p.scale_mask[1]) == 0) return true;
    const int k = si.scale_idx;
    return k < 127 && ((p.scale_mask[k >> 6] >> (k & 63)) & 1ull);   // bit 127 = VJ_SCALE_MASK_NONE
}

int plan_clod(const Tunables& t, int tile_group, bool sq32, const vj_cascade& c, int W, int H, const vj_params& p, float tile_split,
              const TileThresholds& thresholds, int n_frames, bool one_pass, bool former_shapes, PlanHost* pl, PlanTables* tab) {
    pl->tile_split = tile_split;
    std::vector<uint32_t> order;
    int rc = cascade_shape(c, p.flags, t.general_prefix != 0, pl, &order);
    if (rc) return rc;
    pl->skip_mode = p.flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW);
    // how a grid index becomes a pixel position (window_pos): bit 0 = round half away from zero, bit 1 = f64 product.
    // precomputeWindows / the OpenCL path: lrint of the f32 product (clod.cpp:514); plain CPU loop: round() of it (:1416);
    // block variant: lrint of the f64 product in its row loop (:941-942), round() of it in its per-stage lists (:1034)
    pl->pos_mode = (p.flags & VJ_FLAG_GRID_F64) ? (pl->skip_mode == VJ_FLAG_SKIP_LIST ? 3u : 2u)
                                                : (pl->skip_mode == VJ_FLAG_SKIP_ROW ? 1u : 0u);
    // wave-independent tail of a tile (tile_wave_tail): stages of more than TILE_SP_MAX_BLOCKS * 64 nodes rule it out
    pl->wave_tail = !pl->trees && !pl->general && t.tile_sp_begin < (int)c.stages.size() &&
                    pl->max_stage_nodes <= (uint32_t)TILE_SP_MAX_BLOCKS * TILE_SP_BLOCK;
    pl->scales_all = plan_scales(c, W, H, p);
    pl->frame_elems = frame_elems_for(W, H);
    for (const vj_scale_info& si : pl->scales_all) {
        if (!scale_selected(si, p)) continue;
        if (pl->scales.size() >= (size_t)MAX_SCALES) {
            set_error("more than %d scales", MAX_SCALES);
            return VJ_ERR_LIMIT;
        }
        ScaleDev sd;
        Reach reach;
        if ((rc = scale_record(c, W, si, pl->pos_mode, sq32, tab, &sd, &reach))) return rc;
        pl->max_reach_elems = std::max(pl->max_reach_elems, reach.elems);
        pl->windows_per_frame += sd.nwin;
        TileShape shape;
        const bool may_tile = (!pl->general || pl->general_prefix) && si.ny < 65536 && si.nx < 65536;
        if (may_tile && search_tile_shape(t, thresholds, si.step, reach.x, reach.y, former_shapes, pl->wave_tail, pl->max_stage_nodes, &shape))
            if ((rc = lay_out_tile(c, si, shape, &tab->table, &sd))) return rc;
        pl->scales.push_back(sd);
        pl->scales_info.push_back(si);
        pl->tile_reach.push_back({reach.x, reach.y});
    }
    if (pl->max_reach_elems >= pl->frame_elems) {
        set_error("feature reach %u exceeds the frame allocation %u", pl->max_reach_elems, pl->frame_elems);
        return VJ_ERR_LIMIT;
    }
    if ((rc = group_tile_scales(c, tile_group, pl->scales_info, pl->tile_reach, &pl->scales, &tab->table, &pl->tile_lead))) return rc;
    pl->stages = stage_records(c, pl->prog, order);
    tab->sp_blocks = tail_blocks(pl->prog, &pl->stages);
    pl->n_sp_blocks = (uint32_t)tab->sp_blocks.size();
    if (pl->wave_tail && !tab->sp_blocks.empty()) transpose_tail_tables(tab->sp_blocks, &pl->scales, &tab->table);
    cut_tile_rows(tile_split, pl->tile_lead, &pl->scales);
    pl->unit_cap = t.unit_cap_for(n_frames, pl->general, pl->trees);
    if ((rc = gather_units(t, pl->scales, pl->unit_cap, &pl->units))) return rc;
    if (t.q_band_px > 0 && !pl->units.empty()) order_units_by_band(t, pl->scales, pl->unit_cap, &pl->units, &pl->unit_groups);
    plan_passes(t, c, order, one_pass, pl);
    tile_lists(pl);
    nest_class_lds(t, pl->class_lds);
    if (pl->skip_mode) {
        if (pl->general) {
            set_error("the skip modes restate the reference's CPU loops, which run linear cascades only");
            return VJ_ERR_UNSUPPORTED;
        }
        pl->skip_frame_words = skip_bitmaps(pl->skip_mode, &pl->scales, &tab->skip_units, &tab->skip_segs);
        pl->n_skip_units = (uint32_t)tab->skip_units.size();
        pl->n_skip_segs = (uint32_t)tab->skip_segs.size();
    }
    return VJ_OK;
}

}  // namespace vj

using namespace vj;

// The tile side of the plan a fresh environment builds for a call of n_frames frames, on the host alone: the default
// settings (Tunables{}) and diagnostics, through the planner every call runs.
// tile_split < 0: the default chain balance of that batch size (Tunables::split_for), else the given one — what a call runs
// after vj_env_configure("tile_split", ...) or where the balance feedback has walked to.
static int plan_tiles_query(const vj_cascade* c, int width, int height, const vj_params* p, int n_frames, uint32_t flags, float tile_split,
                            vj_tile_plan_info* info, vj_tile_cut_info* cut, vj_tile_info* out, uint64_t* gather_windows, int cap, int* n) {
    if (!c || !p || !n || width <= 0 || height <= 0 || n_frames <= 0 || (cap > 0 && !out) || tile_split != tile_split ||
        (flags & ~(uint32_t)(VJ_PLAN_TILES_FORMER_SHAPES | VJ_PLAN_TILES_NO_GROUPS)))
        return VJ_ERR_ARG;
    int rc = check_params(*p);
    if (rc) return rc;
    const Tunables t;
    const int tile_group = (flags & VJ_PLAN_TILES_NO_GROUPS) ? 1 : tile_group_from_env();
    PlanHost pl;
    PlanTables tab;
    rc = plan_clod(t, tile_group, true, *c, width, height, *p, tile_split < 0.0f ? t.split_for(n_frames, *p, linear_stumps(*c)) : tile_split,
                   thresholds_for(t, small_frame_class(t, width, height, n_frames)), n_frames, one_pass_for(t, width, height, n_frames),
                   (flags & VJ_PLAN_TILES_FORMER_SHAPES) != 0u, &pl, &tab);
    if (rc) return rc;
    // the windows every first-pass unit of the gather chain covers, clipped to its scale's grid as the grid pass clips them
    std::vector<uint64_t> unit_windows(pl.scales.size(), 0);
    for (const UnitDev& u : pl.units) {
        const ScaleDev& sd = pl.scales[u.scale];
        if (u.bw != 0u) {
            const uint32_t ix0 = u.first & 0xffffu, iy0 = u.first >> 16, bh = u.count / u.bw;
            if (ix0 < sd.nx && iy0 < sd.ny)
                unit_windows[u.scale] += (uint64_t)std::min(u.bw, sd.nx - ix0) * std::min(bh, sd.ny - iy0);
        } else if (u.first < sd.nwin) {
            unit_windows[u.scale] += std::min(u.count, sd.nwin - u.first);
        }
    }
    if (cut) {
        memset(cut, 0, sizeof(*cut));
        cut->tile_split = pl.tile_split;
        cut->gather_units = (uint32_t)pl.units.size();
        for (uint64_t w : unit_windows) cut->gather_windows += w;
        cut->plan_windows = pl.windows_per_frame;
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->header_bytes = TILE_LDS_HEADER;
        info->gather_reserve_bytes = (uint32_t)t.tile_lds_reserve_kb * 1024u;
        info->max_tile_windows = TILE_WAVES * TILE_WAVE_CAP;
        info->n_classes = TILE_CLASSES;
        for (uint32_t cls = 0; cls < TILE_CLASSES; ++cls) {
            info->class_lds[cls] = pl.class_lds[cls];
            info->class_per_cu[cls] = t.tile_class_kb[cls] < 0 ? -t.tile_class_kb[cls] : 0;
            info->class_tiles[cls] = pl.class_first[cls + 1] - pl.class_first[cls];
        }
    }
    *n = (int)pl.scales.size();
    for (int k = 0; k < *n && k < cap; ++k) {
        const ScaleDev& sd = pl.scales[(size_t)k];
        vj_tile_info& ti = out[k];
        memset(&ti, 0, sizeof(ti));
        ti.scale_idx = (int32_t)sd.scale_idx;
        ti.scale = sd.scale_f;
        ti.step = sd.step;
        ti.nx = (int32_t)sd.nx;
        ti.ny = (int32_t)sd.ny;
        ti.reach_x = (int32_t)pl.tile_reach[(size_t)k].first;
        ti.reach_y = (int32_t)pl.tile_reach[(size_t)k].second;
        if (gather_windows) gather_windows[k] = unit_windows[(size_t)k];
        ti.lds_class = -1;
        ti.lead_scale_idx = ti.scale_idx;
        if (!sd.tile_rw) continue;
        ti.lds_class = (int32_t)sd.tile_class;
        ti.tile_w = (int32_t)sd.tile_tw;
        ti.tile_h = (int32_t)sd.tile_th;
        ti.pitch = (int32_t)sd.tile_pitch;
        ti.rows = (int32_t)sd.tile_rows;
        ti.lead_scale_idx = (int32_t)pl.scales[pl.tile_lead[(size_t)k]].scale_idx;
        ti.tile_row_end = (int32_t)sd.tile_row_end;
    }
    return VJ_OK;
}

extern "C" {

int vj_plan_tiles(const vj_cascade* c, int width, int height, const vj_params* p, int n_frames, uint32_t flags,
                  vj_tile_plan_info* info, vj_tile_info* out, int cap, int* n) {
    return plan_tiles_query(c, width, height, p, n_frames, flags, -1.0f, info, nullptr, out, nullptr, cap, n);
}

int vj_plan_tiles_split(const vj_cascade* c, int width, int height, const vj_params* p, int n_frames, uint32_t flags, float tile_split,
                        vj_tile_plan_info* info, vj_tile_cut_info* cut, vj_tile_info* out, uint64_t* gather_windows, int cap, int* n) {
    return plan_tiles_query(c, width, height, p, n_frames, flags, tile_split, info, cut, out, gather_windows, cap, n);
}

}  // extern "C"
