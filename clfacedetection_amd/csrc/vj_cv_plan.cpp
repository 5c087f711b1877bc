// The planner of the OpenCV profile: the three scale enumerations of cvHaarDetectObjects as the reference keeps it in tempcv.cpp,
// the pyramid's canvas, a stage tree's prefix and chains, node tables, LDS tile shapes, tile / row / bitmap lists, pruning
// rectangles and the pyramid's taps of one (cascade, frame size, parameters, batch-size class, settings) — pure host index
// arithmetic that the kernels trust without bounds checks.  Nothing here touches a device: plan_cv fills a CvPlanHost and the
// CvPlanTables the driver uploads, one named step after the other.  Compiled with -ffp-contract=off; re-entrant (no mutable statics).
#include "vj_cv_plan.hpp"
#include "vj_clod_plan.hpp"   // frame_elems_for
#include "vj_cv_roi_levels_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vj {

// ---- the cascade --------------------------------------------------------------------------------------------------------------

CvShape cv_shape_of(const vj_cascade* c) {
    CvShape sh;
    for (const auto& st : c->stages) sh.is_tree |= st.next != -1;
    for (const auto& t : c->trees)
        if (t.n_nodes != 1) sh.trees = true;
    for (const auto& nd : c->nodes) sh.has_tilted |= nd.tilted != 0;
    // two-node trees (frontalface_alt2): root + one node child — the shape the tile kernel's tree path knows
    sh.tree2 = sh.trees;
    for (const auto& t : c->trees) {
        if (!sh.tree2) break;
        if (t.n_nodes != 2) { sh.tree2 = false; break; }
        const vj_node_desc& n0 = c->nodes[t.first_node];
        const vj_node_desc& n1 = c->nodes[t.first_node + 1];
        const int kids = (n0.left > 0) + (n0.right > 0);
        if (kids != 1 || (n0.left > 0 ? n0.left : n0.right) != 1 || n1.left > 0 || n1.right > 0) sh.tree2 = false;
    }
    sh.two_rects.assign(c->stages.size(), 1);
    for (size_t s2 = 0; s2 < c->stages.size(); ++s2)
        for (int t = 0; t < c->stages[s2].n_trees; ++t) {
            const vj_tree_desc& td = c->trees[c->stages[s2].first_tree + t];
            for (int l = 0; l < td.n_nodes; ++l) {
                const vj_rect_desc& r2 = c->nodes[td.first_node + l].rect[2];
                // :452-457: the third rectangle counts unless |weight| < DBL_EPSILON or it is empty
                if (!(std::fabs((double)r2.weight) < 2.220446049250313e-16 || r2.w == 0 || r2.h == 0)) sh.two_rects[s2] = 0;
            }
        }
    return sh;
}

int build_cv_node_recs(const vj_cascade* c, double scale, uint32_t stride, double weight_scale, CvNodeRec* recs, uint64_t* max_reach) {
    for (size_t t = 0; t < c->trees.size(); ++t) {
        const vj_tree_desc& td = c->trees[t];
        for (int j = 0; j < td.n_nodes; ++j) {
            const vj_node_desc& nd = c->nodes[td.first_node + j];
            CvNodeRec& r = recs[td.first_node + j];
            memset(&r, 0, sizeof(r));
            if (nd.rect[0].weight == 0.0f || nd.rect[1].weight == 0.0f) {
                set_error("node %d: rect 0 and rect 1 must both be weighted", td.first_node + j);
                return VJ_ERR_UNSUPPORTED;
            }
            double sum0 = 0, area0 = 0;
            const double correction_ratio = weight_scale * (!nd.tilted ? 1 : 0.5);   // :731
            for (int q = 0; q < 3; ++q) {
                // hidfeature->rect[k].p0 == 0 ends the list (tempcv.cpp:663): only a third rectangle can be absent (:452-455)
                if (q == 2 && (std::fabs((double)nd.rect[2].weight) < 2.220446049250313e-16 || nd.rect[2].w == 0 || nd.rect[2].h == 0))
                    break;
                const int tx = cv_round(nd.rect[q].x * scale), ty = cv_round(nd.rect[q].y * scale);
                const int tw = cv_round(nd.rect[q].w * scale), th = cv_round(nd.rect[q].h * scale);
                // corners p0, p1 = p0 + da, p2 = p0 + db, p3 = p0 + da + db (element offsets)
                const int64_t p0 = (int64_t)ty * stride + tx;
                int64_t da, db;
                if (!nd.tilted) {         // :735-741
                    da = tw;
                    db = (int64_t)th * stride;
                } else {                  // :743-750: p1 = (y + h, x - h), p2 = (y + w, x + w), p3 = (y + w + h, x + w - h)
                    da = (int64_t)th * stride - th;
                    db = (int64_t)tw * stride + tw;
                }
                if (p0 < 0 || da < 0 || db < 0 || (p0 + da + db) * 4 > 0x7fffffffll) {
                    set_error("feature offsets exceed the device record range");
                    return VJ_ERR_LIMIT;
                }
                r.lt[q] = (uint32_t)(p0 * 4);
                r.da[q] = (uint32_t)(da * 4);
                r.db[q] = (uint32_t)(db * 4);
                r.w[q] = (float)(nd.rect[q].weight * correction_ratio);
                if (q == 0)
                    area0 = tw * th;
                else
                    sum0 += r.w[q] * tw * th;                          // float * int * int, added to a double (:756)
                *max_reach = std::max<uint64_t>(*max_reach, (uint64_t)(p0 + da + db));
                *max_reach = std::max<uint64_t>(*max_reach, (uint64_t)(p0 + db));
            }
            r.w[0] = (float)(-sum0 / area0);
            r.thr = nd.threshold;
            uint32_t flags = nd.tilted ? CV_NODE_TILTED : 0u;
            auto leaf_or_node = [&](int v, uint32_t flag, uint32_t* dst) {
                if (v > 0) {
                    flags |= flag;
                    *dst = (uint32_t)v;
                } else {
                    const float a = c->alpha[td.first_alpha - v];
                    memcpy(dst, &a, 4);
                }
            };
            leaf_or_node(nd.left, NODE_LEFT_IS_NODE, &r.left);
            leaf_or_node(nd.right, NODE_RIGHT_IS_NODE, &r.right);
            if (j == td.n_nodes - 1) flags |= NODE_TREE_LAST;
            r.flags = flags;
        }
    }
    return VJ_OK;
}

std::vector<StageDev> build_cv_stage_recs(const vj_cascade* c, const StageProgram& prog, const std::vector<uint32_t>& order,
                                          const std::vector<uint8_t>& two_rects, bool trees, bool is_tree) {
    std::vector<StageDev> stages(c->stages.size());
    for (size_t s = 0; s < c->stages.size(); ++s) {
        memset(&stages[s], 0, sizeof(StageDev));
        stages[s].first_node = prog.first_node[s];
        stages[s].n_nodes = prog.n_nodes[s];
        stages[s].threshold = c->stages[s].threshold - 0.0001f;   // icv_stage_threshold_bias, in f32
        stages[s].n_trees = (uint32_t)c->stages[s].n_trees;
        stages[s].on_pass = prog.on_pass[s];
        stages[s].on_fail = prog.on_fail[s];
        stages[s].order = s < order.size() ? order[s] : 0u;
        // an f64 product per rectangle only on cvRunHaarClassifierCascadeSum's stump path (:863-888)
        stages[s].cv_f64 = (two_rects[s] && !trees && !is_tree) ? 1u : 0u;
        // wave-split finish of the tile kernel: bound on the difference between any two summation orders of the stage's
        // leaf values (the f32 form of the clod profile's bound, stage_records in vj_clod_plan.cpp; the kernel scales it to f64's unit roundoff)
        double amax = 0.0;
        for (int t = 0; t < c->stages[s].n_trees; ++t) {
            const vj_tree_desc& td = c->trees[c->stages[s].first_tree + t];
            double m = 0.0;
            for (int k = 0; k <= td.n_nodes; ++k) m = std::max(m, (double)std::fabs(c->alpha[td.first_alpha + k]));
            amax += m;
        }
        stages[s].sp_delta = (float)(4.0 * (double)prog.n_nodes[s] * std::ldexp(1.0, -24) * amax * 1.001 + 1e-30);
    }
    return stages;
}

int cv_cascade_host(const vj_cascade* c, CvCascadeHost* out) {
    if ((int)c->stages.size() > VJ_MAX_STAGES || c->stages.empty()) {
        set_error("cascade has %zu stages; 1..%d are supported", c->stages.size(), VJ_MAX_STAGES);
        return VJ_ERR_LIMIT;
    }
    out->prog = build_stage_program(*c);
    if (!stage_sweep_order(out->prog, &out->order)) {
        set_error("stage links form a cycle");
        return VJ_ERR_UNSUPPORTED;
    }
    out->shape = cv_shape_of(c);
    out->stages = build_cv_stage_recs(c, out->prog, out->order, out->shape.two_rects, out->shape.trees, out->shape.is_tree);
    return VJ_OK;
}

int cv_max_level_end(const vj_cascade* c, int W, int H, double scale_factor, int max_w, int max_h) {
    double factor = 1;
    for (int k = 0; k <= 65536; ++k, factor *= scale_factor) {
        if (cv_round(W / factor) - c->win_w + 1 <= 0 || cv_round(H / factor) - c->win_h + 1 <= 0) return -1;
        if (cv_round(c->win_w * factor) > max_w || cv_round(c->win_h * factor) > max_h) return k;
    }
    return -1;
}

namespace {

// ---- the scales ---------------------------------------------------------------------------------------------------------------

struct CvScaleHost {
    double factor;
    int idx;
    int win_w, win_h, end_x, end_y;
    // CV_HAAR_SCALE_IMAGE: a level of the pyramid — its size, its place in the canvas and its grid step
    int lw = 0, lh = 0, ox = 0, oy = 0, step = 0;
};

// The factors of the scale loop (tempcv.cpp:1344-1377), counted upwards; *factor: the first one that is too large
int count_factors(const vj_cascade* c, int W, int H, double scale_factor, double* factor) {
    int n_factors = 0;
    *factor = 1;
    for (; *factor * c->win_w < W - 10 && *factor * c->win_h < H - 10; n_factors++, *factor *= scale_factor) {}
    return n_factors;
}

// One scale of that loop: its window and its grid
CvScaleHost scale_at(const vj_cascade* c, int W, int H, double factor, int idx) {
    const double ystep = std::max(2., factor);
    CvScaleHost s;
    s.factor = factor;
    s.idx = idx;
    s.win_w = cv_round(c->win_w * factor);
    s.win_h = cv_round(c->win_h * factor);
    s.end_x = cv_round((W - s.win_w) / ystep);
    s.end_y = cv_round((H - s.win_h) / ystep);
    return s;
}

// The plain scale loop: ascending factors; scales below minSize or without a position are skipped and keep their number
std::vector<CvScaleHost> ascending_scales(const vj_cascade* c, int W, int H, const vj_cv_params& p) {
    std::vector<CvScaleHost> hs;
    double factor;
    const int n_factors = count_factors(c, W, H, p.scale_factor, &factor);
    factor = 1;
    for (int k = 0; k < n_factors; ++k, factor *= p.scale_factor) {
        const CvScaleHost s = scale_at(c, W, H, factor, k);
        if (s.win_w < p.min_w || s.win_h < p.min_h) continue;
        if (s.end_x <= 0 || s.end_y <= 0) continue;
        hs.push_back(s);
    }
    return hs;
}

// find-biggest (tempcv.cpp:1344-1380): the factors are counted upwards, then walked DOWN from the last one by repeated
// multiplication with the reciprocal — other doubles than the ascending ones in general.  The loop BREAKS at the first window
// below minSize, but minSize is the frame's own from its first grouped object on (:1450-1452, possibly smaller than the
// call's): every scale is planned, and the waves of cv_biggest_pass apply the break per frame (windows only shrink, so a
// frame that broke stays out).  Slot k is the k-th scale of the walk; scale_idx = n_factors - 1 - k.
std::vector<CvScaleHost> descending_scales(const vj_cascade* c, int W, int H, const vj_cv_params& p) {
    std::vector<CvScaleHost> hs;
    double factor;
    const int n_factors = count_factors(c, W, H, p.scale_factor, &factor);
    const double down = 1. / p.scale_factor;
    factor *= down;
    for (int k = 0; k < n_factors; ++k, factor *= down) {
        const CvScaleHost s = scale_at(c, W, H, factor, n_factors - 1 - k);
        if (s.end_x <= 0 || s.end_y <= 0) continue;   // (no position: nothing to walk, and no new candidate to group)
        hs.push_back(s);
    }
    return hs;
}

// CV_HAAR_SCALE_IMAGE: the level loop (tempcv.cpp:1268-1288; maxSize is the image unless a ROC call brings one)
// (the loop itself, build_taps and resize_is_area: vj_cv_roi_levels_host.cpp — the regions' level canvases share them)
int level_scales(const vj_cascade* c, int W, int H, const vj_cv_params& p, const CvMaxSize* roc, std::vector<CvScaleHost>* hs) {
    const int max_w = roc ? roc->max_w : W, max_h = roc ? roc->max_h : H;
    std::vector<CvLevelHost> lv;
    const int lrc = cv_scale_image_levels(c->win_w, c->win_h, W, H, p.scale_factor, p.min_w, p.min_h, max_w, max_h, &lv);
    if (lrc) return lrc;
    for (const CvLevelHost& l : lv) {
        CvScaleHost s;
        s.factor = l.factor;
        s.idx = l.idx;
        s.win_w = l.win_w;
        s.win_h = l.win_h;
        s.lw = l.lw;
        s.lh = l.lh;
        s.step = l.step;
        s.end_x = l.end_x;
        s.end_y = l.end_y;
        hs->push_back(s);
    }
    return VJ_OK;
}

// One canvas per frame holds every level (levels come in decreasing size): shelves of the canvas's width, a level goes to the
// first shelf that has room beside what it holds, else it opens a new one below.  A rectangle sum does not depend on where the
// integral image starts (u32 wrap-around cancels, the u64 square sums are exact), and the four corners of a tilted rectangle
// give the sum of the pixels INSIDE it whatever lies beside it: neighbours need no gap.  *IW x *IH: the canvas.
int pack_canvas(std::vector<CvScaleHost>* hs, int* IW, int* IH) {
    struct Shelf { int y, h, used; };
    std::vector<Shelf> shelves;
    *IW = hs->empty() ? 1 : (*hs)[0].lw;
    *IH = 0;
    for (CvScaleHost& s : *hs) {
        Shelf* fit = nullptr;
        for (Shelf& sh : shelves)
            if (sh.used + s.lw <= *IW && s.lh <= sh.h) { fit = &sh; break; }
        if (!fit) {
            shelves.push_back(Shelf{*IH, s.lh, 0});
            *IH += s.lh;
            fit = &shelves.back();
        }
        s.ox = fit->used;
        s.oy = fit->y;
        fit->used += s.lw;
    }
    *IH = std::max(*IH, 1);
    if (*IH >= 65535 || (uint64_t)(*IW + 1) * (uint64_t)(*IH + 3) >= (1ull << 30)) {
        set_error("the image pyramid (%d x %d for %zu levels) does not fit 32-bit offsets", *IW, *IH, hs->size());
        return VJ_ERR_LIMIT;
    }
    return VJ_OK;
}

// ---- a stage tree -------------------------------------------------------------------------------------------------------------

// stage trees: the tiles run the tree's linear prefix — leading stages of the sweep order that reject outright and pass
// on to the next one (cv_profile_pass finds the same prefix) — when the prefix is stages 0, 1, 2, ... themselves
uint32_t tree_prefix_of(const StageProgram& prog, const std::vector<uint32_t>& order) {
    uint32_t tree_prefix = 0;
    while (tree_prefix + 1u < order.size() && order[tree_prefix] == tree_prefix && prog.on_fail[tree_prefix] == STAGE_REJECT &&
           prog.on_pass[tree_prefix] == (int)order[tree_prefix + 1u])
        ++tree_prefix;
    return tree_prefix;
}

// Is the rest of the tree a sequence of chains (CvChainDev)?  A chain is a run of sweep positions whose pass edges follow
// the order and end in an accept, whose rejects all go to ONE place: nowhere (final) or the first stage of the NEXT chain.
// n = 0 when it is not.
CvChainDev tree_chains(const StageProgram& prog, const std::vector<uint32_t>& order, uint32_t tree_prefix, int tail_max) {
    CvChainDev ch;
    memset(&ch, 0, sizeof(ch));
    bool ok = true;
    uint32_t b = tree_prefix;
    while (b < order.size() && ok) {
        if (ch.n == 4u) { ok = false; break; }
        const int f = prog.on_fail[order[b]];
        uint32_t e2 = b;
        while (true) {
            const uint32_t sid = order[e2];
            if (prog.on_fail[sid] != f) { ok = false; break; }
            const int np = prog.on_pass[sid];
            ++e2;
            if (np == STAGE_ACCEPT) break;
            if (e2 >= order.size() || np != (int)order[e2]) { ok = false; break; }
        }
        if (!ok) break;
        ch.begin[ch.n] = b;
        ch.end[ch.n] = e2;
        if (f != STAGE_REJECT) {
            if (e2 < order.size() && f == (int)order[e2]) ch.chained |= 1u << ch.n;   // rejects start the next chain
            else ok = false;
        }
        ++ch.n;
        b = e2;
    }
    ch.tail_max = (uint32_t)std::max(0, std::min(tail_max, (int)CV_TAIL_MAX));
    if (ok && ch.n != 0u && !((ch.chained >> (ch.n - 1u)) & 1u)) return ch;
    return CvChainDev{};
}

// ---- tiles --------------------------------------------------------------------------------------------------------------------

// Which scales may go to LDS tiles (vj_cv_tile.hip), and next to how many workgroups of the row kernel.
struct TileRules {
    bool on;                   // the plan has a tile path at all
    bool share_tables;         // scale image: one tile-pitch table per tile shape
    int min_windows0, min_windows;   // a scale goes to class 0 / class 1 when a tile of at least this many windows fits
    uint32_t class_bytes[2];   // image bytes of a tile per LDS class
    uint32_t images;           // LDS images per tile: the sum's, and the tilted integral's behind it
};

// (a stage tree's row kernel evaluates the whole tree at every grid position and is far slower per window than the tiles'
// prefix: trees send every scale they can to tiles and leave the row kernel two workgroups per CU)
// (linear cascades, profiles/r04_notes.md #5b: stumps 2 workgroups x tiles of >= 2048 windows — 64 x 1080p frontalface_alt 66.6 ms against 80.5
// at 3 x 1536, frontalface_default 51.4 / 57.1, 256 x 720p 112.7 / 136.9 —, multi-node trees the other way round: frontalface_alt2 99.3 / 77.5;
// two-node trees with both nodes fetched at once (CvArgs::tree2, #5d): 2 x 1536 69.9 ms against 80.9 at 3 x 1536)
// *row_blocks: workgroups per CU of cv_profile_pass next to the tiles.
TileRules tile_rules(const Tunables& t, const CvShape& sh, const CvPlanHost& pl, bool small_batch, int* row_blocks) {
    const bool rows_tree2 = sh.tree2 && !sh.is_tree && !sh.has_tilted && t.cv_tree2;
    // (cascades with tilted features, #12: a tile holds two images, so the shapes that fit are smaller — and the row kernel they relieve is 2-3x
    // the tiles' cost per window: two workgroups x tiles of >= 512 windows, `fullbody` 16 x 1080p 28-29 ms against 40.8 with every tile of
    // >= 2048 windows refused, `upperbody` 50.7 / 96.6, `mcs_righteye`'s kernels 30.9 / 72.4)
    const bool tilt_tiles = sh.has_tilted && t.cv_tiles_tilted && !sh.is_tree;
    const int lin_blocks = t.cv_row_blocks > 0 ? t.cv_row_blocks : tilt_tiles ? 2 : sh.trees && !rows_tree2 ? 3 : 2;
    const int lin_min_windows = t.cv_tile_min_windows > 0 ? t.cv_tile_min_windows : tilt_tiles ? 512 : sh.trees ? 1536 : 2048;
    *row_blocks = sh.is_tree ? t.cv_row_blocks_tree : lin_blocks;
    TileRules r;
    r.min_windows = sh.is_tree ? t.cv_tile_min_windows_tree : lin_min_windows;
    r.min_windows0 = tilt_tiles ? std::min(t.cv_tile_min_windows0, 512) : t.cv_tile_min_windows0;
    // a call of <= 4 frames is bound by latency, not by the balance of two saturated chains: one row-kernel workgroup per CU
    // and every scale that has a tile of 512 windows on tiles (one 1080p frame: 2.4 -> 2.0 ms)
    if (small_batch && !sh.is_tree) {
        *row_blocks = 1;
        r.min_windows = std::min(r.min_windows, 512);
        r.min_windows0 = std::min(r.min_windows0, 1024);
    }
    // ---- LDS-tile path (vj_cv_tile.hip): stump cascades with linear stages and upright features.  A tile is tw x th
    // windows (tw divides 64, so a tile row never straddles a word of the reject / visited bitmap); its footprint is
    // the span of its window origins plus the furthest corner any feature or the equRect reaches.  Two LDS classes
    // like the clod profile's tiles: two workgroups per CU or one, next to one workgroup of cv_profile_pass.
    // Tilted features (round 4): the tile's footprint of the TILTED integral is staged right behind the sum's (same origin, pitch and
    // rows: a tilted rectangle's corners (y, x), (y + h, x - h), (y + w, x + w), (y + w + h, x + w - h) lie inside the window's box), a
    // tilted node's record carries that distance in its corner offsets, and the kernel's node code does not change.
    // CV_HAAR_SCALE_IMAGE: the levels of linear cascades whose grid fills a tile run cv_tile_pass<3> (the exhaustive grid; step 1 or 2);
    // stage trees stay on the exhaustive-grid row kernel (their tile path is built around the tree queue and the accept bitmap)
    // (a ROC call keeps every level on the rows: the tile kernel has no form that reports reject levels)
    r.on = !pl.find_biggest && !(pl.scale_image && sh.is_tree) && !pl.roc && t.cv_tiles && (!sh.trees || (sh.tree2 && !sh.is_tree)) &&
           (!sh.is_tree || pl.tree_prefix != 0u) && (!sh.has_tilted || tilt_tiles);
    r.share_tables = pl.scale_image;
    r.images = sh.has_tilted ? 2u : 1u;
    // LDS budget of a CU: the row kernel's workgroups (20 KiB each) stay resident next to two tile workgroups
    // of class 0 or one of class 1; a tile workgroup also owns CVT_LDS_HEADER bytes of queues
    const uint32_t avail = 160u * 1024u - (uint32_t)*row_blocks * 20u * 1024u - 1024u;
    r.class_bytes[0] = avail / 2u - (uint32_t)CVT_LDS_HEADER;
    r.class_bytes[1] = avail - (uint32_t)CVT_LDS_HEADER;
    return r;
}

// How far right / down of a window origin the equRect and the features of a frame-stride table reach (the third rectangle only
// where the node has one)
struct TileReach { uint32_t x, y; };
TileReach tile_reach(const CvNodeRec* recs, size_t n_nodes, uint32_t stride, const CvEquRect& q) {
    TileReach reach{(uint32_t)(q.ex + q.ew), (uint32_t)(q.ex + q.eh)};
    for (size_t n = 0; n < n_nodes; ++n) {
        const CvNodeRec& r = recs[n];
        for (int k = 0; k < 3; ++k)
            if (k < 2 || r.w[2] != 0.0f) {
                const uint32_t p0 = r.lt[k] / 4u;
                if (r.flags & CV_NODE_TILTED) {   // da = h * (stride - 1), db = w * (stride + 1): rightmost corner x + w, lowest y + w + h
                    const uint32_t hh = (r.da[k] / 4u) / (stride - 1u), ww = (r.db[k] / 4u) / (stride + 1u);
                    reach.x = std::max(reach.x, p0 % stride + ww);
                    reach.y = std::max(reach.y, p0 / stride + ww + hh);
                } else {
                    reach.x = std::max(reach.x, p0 % stride + r.da[k] / 4u);
                    reach.y = std::max(reach.y, p0 / stride + (r.db[k] / 4u) / stride);
                }
            }
    }
    return reach;
}

// The tile shape of a scale: the shape of the most windows that fits class 0 when it is worth two workgroups per CU, else that
// of class 1; false when neither holds enough windows (the scale stays on the row kernel).
struct TileShape { uint32_t tw, th, pitch, rows; int cls; };
bool search_tile_shape(const TileRules& rules, const CvScaleDev& sd, const TileReach& reach, TileShape* out) {
    static const uint32_t kTw[] = {64, 32, 16}, kTh[] = {32, 24, 16, 12, 8, 4};
    uint32_t best_n = 0;
    *out = TileShape{0, 0, 0, 0, -1};
    for (int cls = 0; cls < 2; ++cls) {
        for (uint32_t tw : kTw)
            for (uint32_t th : kTh) {
                const uint32_t pitch = (((uint32_t)std::ceil((double)(tw - 1) * sd.ystep) + 3u + reach.x) + 3u) & ~3u;
                const uint32_t trows = (uint32_t)std::ceil((double)(th - 1) * sd.ystep) + 3u + reach.y;
                if ((uint64_t)pitch * trows * 4u * rules.images > rules.class_bytes[cls]) continue;
                const uint32_t nwin = std::min(tw, sd.end_x) * std::min(th, sd.end_y);
                if (nwin > best_n) { best_n = nwin; *out = TileShape{tw, th, pitch, trows, cls}; }
            }
        // a class-0 tile must be worth two workgroups per CU; else try the larger class
        if (best_n >= (uint32_t)(cls == 0 ? rules.min_windows0 : rules.min_windows)) {
            out->cls = cls;
            return true;
        }
        best_n = 0;
    }
    return false;
}

// The records [first, first + n_nodes) of `table` once more at its end, with corner steps in the tile's pitch; a tilted node's in
// the tilted image behind the sum image.  Returns where the copy starts.
uint32_t append_tile_pitch_table(std::vector<CvNodeRec>* table, size_t first, size_t n_nodes, uint32_t stride, uint32_t pitch, uint32_t rows) {
    const uint32_t tile_first = (uint32_t)table->size();
    table->resize(table->size() + n_nodes);   // (within the reserved capacity)
    const CvNodeRec* recs = table->data() + first;
    CvNodeRec* trec = table->data() + tile_first;
    for (size_t n = 0; n < n_nodes; ++n) {
        trec[n] = recs[n];
        for (int q = 0; q < 3; ++q)
            if (q < 2 || recs[n].w[2] != 0.0f) {
                const uint32_t p0 = recs[n].lt[q] / 4u;
                if (recs[n].flags & CV_NODE_TILTED) {
                    const uint32_t hh = (recs[n].da[q] / 4u) / (stride - 1u), ww = (recs[n].db[q] / 4u) / (stride + 1u);
                    trec[n].lt[q] = (pitch * rows + (p0 / stride) * pitch + p0 % stride) * 4u;
                    trec[n].da[q] = (hh * pitch - hh) * 4u;
                    trec[n].db[q] = (ww * pitch + ww) * 4u;
                } else {
                    const uint32_t hh = (recs[n].db[q] / 4u) / stride;
                    trec[n].lt[q] = ((p0 / stride) * pitch + p0 % stride) * 4u;
                    trec[n].db[q] = hh * pitch * 4u;
                }
            }
    }
    return tile_first;
}

// Scale slot k on tiles when a shape fits: its tile fields and its table in the tile's pitch.  Returns its LDS class, -1 when it
// stays on the row kernel.
int tile_scale(const TileRules& rules, size_t k, const CvEquRect& q, uint32_t stride, size_t n_nodes, std::vector<CvScaleDev>* scales,
               std::vector<CvNodeRec>* table) {
    CvScaleDev& sd = (*scales)[k];
    TileShape ts;
    if (sd.end_x >= 65536u || sd.end_y >= 65536u || !search_tile_shape(rules, sd, tile_reach(table->data() + sd.table_first, n_nodes, stride, q), &ts))
        return -1;
    sd.tile_tw = ts.tw;
    sd.tile_th = ts.th;
    sd.tile_pitch = ts.pitch;
    sd.tile_rows = ts.rows;
    // scale image: levels whose tiles have one shape share one table in that pitch (every level is the cascade at factor 1)
    for (size_t j = 0; j < k && rules.share_tables; ++j)
        if ((*scales)[j].tile_th != 0u && (*scales)[j].tile_pitch == ts.pitch && (*scales)[j].tile_rows == ts.rows) {
            sd.tile_table_first = (*scales)[j].tile_table_first;
            return ts.cls;
        }
    sd.tile_table_first = append_tile_pitch_table(table, sd.table_first, n_nodes, stride, ts.pitch, ts.rows);
    return ts.cls;
}

// ---- one scale ----------------------------------------------------------------------------------------------------------------

// The record of scale slot k but for its tile fields; returns its equRect.
CvEquRect scale_record(const vj_cascade* c, const CvScaleHost& s, size_t k, bool si, uint32_t stride, CvScaleDev* sd) {
    const double scale = si ? 1. : s.factor;   // cvSetImagesForHaarClassifierCascade(.., 1.) for every level (:1321)
    memset(sd, 0, sizeof(*sd));
    sd->ystep = si ? (double)s.step : std::max(2., scale);
    const CvEquRect q = cv_equ_rect(c->win_w, c->win_h, scale);
    cv_set_equ_rect(sd, q, stride);
    sd->win_w = (uint32_t)s.win_w;
    sd->win_h = (uint32_t)s.win_h;
    sd->end_x = (uint32_t)s.end_x;
    sd->end_y = (uint32_t)s.end_y;
    sd->table_first = si ? 0u : (uint32_t)(k * c->nodes.size());   // (the levels share the table of factor 1)
    sd->scale_idx = (uint32_t)s.idx;
    return q;
}

// CV_HAAR_DO_CANNY_PRUNING (tempcv.cpp:1147-1158): the rectangle [x + ex, + ew) x [y + ey, + eh) of the scaled window, tested at
// every visited position BEFORE the border rule — so its furthest corner, from the last grid position, must stay in the frame's
// allocation (rows past H read the zeroed slack rows, as OpenCV's pointers read whatever follows): false when it does not.
bool prune_rect(const CvScaleHost& s, const CvScaleDev& sd, uint32_t stride, uint32_t frame_elems, CvPruneDev* pr) {
    const int px = cv_round(s.win_w * 0.15), py = cv_round(s.win_h * 0.15);
    const int pw = cv_round(s.win_w * 0.7), ph = cv_round(s.win_h * 0.7);
    pr->p0 = (uint32_t)py * stride + (uint32_t)px;
    pr->p1 = pr->p0 + (uint32_t)pw;
    pr->p2 = (uint32_t)(py + ph) * stride + (uint32_t)px;
    pr->p3 = pr->p2 + (uint32_t)pw;
    const uint64_t last = (uint64_t)cv_round((double)(sd.end_y - 1u) * sd.ystep) * stride + (uint64_t)cv_round((double)(sd.end_x - 1u) * sd.ystep);
    return last + pr->p3 < (uint64_t)frame_elems;
}

// ---- the lists of a frame -----------------------------------------------------------------------------------------------------

// Tiles of one frame by LDS class; rows of every scale and of the scales that stay on cv_profile_pass; one recurrence domain per
// window row of a tile scale in the per-frame bitmap.  Completes the tile scales' records (queue slot, bitmap base).
void frame_lists(const std::vector<CvScaleHost>& hs, const std::vector<int>& tile_class, uint32_t stride, uint32_t images, int row_band_px,
                 CvPlanHost* pl, CvPlanTables* tab) {
    std::vector<CvScaleDev>& scales = pl->scales;
    const bool si = pl->scale_image;
    auto canvas_origin = [&](size_t k) { return si ? (uint32_t)hs[k].oy * stride + (uint32_t)hs[k].ox : 0u; };
    for (size_t k = 0; k < hs.size() && !pl->find_biggest; ++k)   // (find-biggest: cv_biggest_pass lays out a scale's rows itself)
        for (uint32_t iy = 0; iy < scales[k].end_y; ++iy) tab->rows.push_back(UnitDev{(uint32_t)k, iy, canvas_origin(k), 0});
    uint32_t word = 0;
    for (size_t k = 0; k < hs.size(); ++k) {
        CvScaleDev& sd = scales[k];
        if (sd.tile_th == 0u) continue;
        sd.tq_slot = pl->n_tile_scales;
        sd.tq_win_first = (uint32_t)std::min<uint64_t>(pl->tile_windows, 0xffffffffull);
        ++pl->n_tile_scales;
        pl->tile_windows += (uint64_t)sd.end_x * sd.end_y;
        sd.bits_base = word;
        const uint32_t wpr = (sd.end_x + 63u) / 64u;
        for (uint32_t iy = 0; iy < sd.end_y; ++iy) tab->bit_segs.push_back(UnitDev{(uint32_t)k, word + iy * wpr, wpr, 0});
        word += wpr * sd.end_y;
    }
    pl->bits_frame_words = word;
    for (int cls = 0; cls < 2; ++cls) {
        pl->class_first[cls] = (uint32_t)tab->tiles.size();
        uint32_t lds = 0;
        for (size_t k = 0; k < hs.size(); ++k) {
            const CvScaleDev& sd = scales[k];
            if (sd.tile_th == 0u || tile_class[k] != cls) continue;
            lds = std::max(lds, (uint32_t)CVT_LDS_HEADER + sd.tile_pitch * sd.tile_rows * 4u * images);
            for (uint32_t iy0 = 0; iy0 < sd.end_y; iy0 += sd.tile_th)
                for (uint32_t ix0 = 0; ix0 < sd.end_x; ix0 += sd.tile_tw)
                    tab->tiles.push_back(UnitDev{(uint32_t)k, ix0 | (iy0 << 16), canvas_origin(k), 0});
        }
        pl->class_lds[cls] = lds;
    }
    pl->class_first[2] = (uint32_t)tab->tiles.size();
    // Band-major row order (cv_row_band_px != 0): the rows of ALL scales whose top lies in one band of the image, band after
    // band.  The waves of an XCD walk one contiguous piece of the (frame, row) list together (cv_profile_pass), so what they
    // gather from at one time is a band of one frame's integral image — within the XCD's 4 MB of L2 — instead of a whole
    // scale's rows, i.e. the whole 8.3 MB image (rows are independent: the skip rule runs along a row).
    if (row_band_px > 0) {
        const double band = (double)row_band_px;
        std::stable_sort(tab->rows.begin(), tab->rows.end(), [&](const UnitDev& x, const UnitDev& y) {
            // (levels: bands of the canvas)
            const uint32_t bx = (uint32_t)(((double)x.first * scales[x.scale].ystep + hs[x.scale].oy) / band),
                           by = (uint32_t)(((double)y.first * scales[y.scale].ystep + hs[y.scale].oy) / band);
            return bx != by ? bx < by : x.scale != y.scale ? x.scale < y.scale : x.first < y.first;
        });
    }
    for (const UnitDev& r : tab->rows)
        if (scales[r.scale].tile_th == 0u) tab->rows_rest.push_back(r);
    pl->n_rows = (uint32_t)tab->rows.size();
    pl->n_rows_rest = (uint32_t)tab->rows_rest.size();
    pl->n_bit_segs = (uint32_t)tab->bit_segs.size();
}

// The pyramid launch's level table and taps (vj_pyramid.hip): per level its columns' taps, then its rows'
int pyramid_tables(const std::vector<CvScaleHost>& hs, int W, int H, CvPlanHost* pl, CvPlanTables* tab) {
    tab->pyr_levels.resize(hs.size());
    size_t n_taps = 0;
    for (const CvScaleHost& s : hs) n_taps += (size_t)s.lw + (size_t)s.lh;
    tab->pyr_taps.resize(n_taps);
    uint32_t tap = 0, unit = 0;
    for (size_t k = 0; k < hs.size(); ++k) {
        const CvScaleHost& s = hs[k];
        const bool area = resize_is_area(W, H, s.lw, s.lh);
        tab->pyr_levels[k] = PyrLevelDev{(uint32_t)s.ox, (uint32_t)s.oy, (uint32_t)s.lw, (uint32_t)s.lh, tap, tap + (uint32_t)s.lw, unit, area ? 1u : 0u};
        build_taps(W, s.lw, false, area, tab->pyr_taps.data() + tap);
        build_taps(H, s.lh, true, area, tab->pyr_taps.data() + tap + s.lw);
        tap += (uint32_t)(s.lw + s.lh);
        const uint64_t units = (uint64_t)((s.lw + PYR_UNIT_PX - 1) / PYR_UNIT_PX) * (uint64_t)s.lh;
        if (unit + units > 0x7fffffffull) {
            set_error("the image pyramid has too many work units");
            return VJ_ERR_LIMIT;
        }
        unit += (uint32_t)units;
    }
    pl->n_pyr_levels = (uint32_t)hs.size();
    pl->n_pyr_units = unit;
    return VJ_OK;
}

}  // namespace

// ---- the plan -----------------------------------------------------------------------------------------------------------------

int plan_cv(const Tunables& t, const vj_cascade* c, int W, int H, const vj_cv_params& p, bool small_batch, const CvMaxSize* roc,
            CvPlanHost* pl, CvPlanTables* tab) {
    CvCascadeHost ch;
    int rc = cv_cascade_host(c, &ch);
    if (rc) return rc;
    const CvShape& shape = ch.shape;
    pl->prog = ch.prog;
    // CV_HAAR_SCALE_IMAGE never reads doCannyPruning (tempcv.cpp:1257-1329)
    // CV_HAAR_FIND_BIGGEST_OBJECT clears both (tempcv.cpp:1227, :1254)
    const bool fb = (p.flags & VJ_FLAG_CV_FIND_BIGGEST) != 0u;
    const bool si = !fb && (p.flags & VJ_FLAG_CV_SCALE_IMAGE) != 0u;
    pl->find_biggest = fb;
    pl->scale_image = si;
    pl->roc = roc != nullptr;
    pl->prune = !fb && !si && (p.flags & VJ_FLAG_CV_CANNY_PRUNING) != 0u;
    pl->trees = shape.trees;
    pl->is_tree = shape.is_tree;
    pl->has_tilted = shape.has_tilted;
    pl->tree2 = shape.tree2;
    pl->n_order = (uint32_t)ch.order.size();
    pl->n_stages = (uint32_t)c->stages.size();
    std::vector<CvScaleHost> hs;
    int IW = W, IH = H;   // what the integral images are computed of: the frame, or the canvas of the pyramid's levels
    if (si) {
        if ((rc = level_scales(c, W, H, p, roc, &hs))) return rc;
        if ((rc = pack_canvas(&hs, &IW, &IH))) return rc;
        pl->canvas_w = (uint32_t)IW;
        pl->canvas_h = (uint32_t)IH;
        pl->canvas_pitch = ((uint32_t)IW + 3u) & ~3u;
    } else {
        hs = fb ? descending_scales(c, W, H, p) : ascending_scales(c, W, H, p);
    }
    const uint32_t stride = (uint32_t)IW + 1u;
    if (shape.is_tree) pl->tree_prefix = tree_prefix_of(ch.prog, ch.order);
    if (!fb && shape.is_tree && pl->tree_prefix != 0u && ch.prog.on_pass[ch.order[pl->tree_prefix - 1u]] == (int)ch.order[pl->tree_prefix])   // (find-biggest: no chain sweep)
        pl->chains = tree_chains(ch.prog, ch.order, pl->tree_prefix, t.cv_tail_max);
    const TileRules rules = tile_rules(t, shape, *pl, small_batch, &pl->row_blocks);
    const size_t n_nodes = c->nodes.size();
    pl->scales.assign(hs.size(), CvScaleDev{});
    tab->table.assign((si ? std::min<size_t>(hs.size(), 1) : hs.size()) * n_nodes, CvNodeRec{});   // (the levels share the table of factor 1)
    tab->table.reserve(2 * hs.size() * n_nodes);   // tile copies of the small scales' records are appended: no reallocation
    tab->prune.assign(pl->prune ? hs.size() : 0, CvPruneDev{});
    std::vector<int> tile_class(hs.size(), -1);
    bool reach_ok = true;
    const uint32_t frame_elems = frame_elems_for(IW, IH);
    uint64_t max_reach = 0;   // furthest element a feature of this scale touches, from the window origin
    for (size_t k = 0; k < hs.size(); ++k) {
        pl->level_factor.push_back(hs[k].factor);
        CvScaleDev& sd = pl->scales[k];
        const CvEquRect q = scale_record(c, hs[k], k, si, stride, &sd);
        if (!si || k == 0) {
            max_reach = 0;
            if ((rc = build_cv_node_recs(c, si ? 1. : hs[k].factor, stride, q.inv_area, tab->table.data() + sd.table_first, &max_reach))) return rc;
        }
        // evaluated windows satisfy x + win_w <= W and y + win_h <= H (border rule); a feature may overshoot its
        // window by one column / row (separate rounding): the frame allocation has two zeroed slack rows for that
        // (a level: its windows lie inside it, and it inside the canvas)
        const uint64_t origin_max = si ? (uint64_t)(hs[k].oy + hs[k].lh - c->win_h) * stride + (uint64_t)(hs[k].ox + hs[k].lw - c->win_w)
                                       : (uint64_t)(H - hs[k].win_h) * stride + (uint64_t)(W - hs[k].win_w);
        if (origin_max + max_reach >= (uint64_t)frame_elems) reach_ok = false;
        if (pl->prune && !prune_rect(hs[k], sd, stride, frame_elems, &tab->prune[k])) reach_ok = false;
        if (rules.on) tile_class[k] = tile_scale(rules, k, q, stride, n_nodes, &pl->scales, &tab->table);
    }
    frame_lists(hs, tile_class, stride, rules.images, t.cv_row_band_px, pl, tab);
    tab->stages = std::move(ch.stages);
    if (!reach_ok) {
        set_error("feature reach exceeds the frame allocation");
        return VJ_ERR_LIMIT;
    }
    return si && !hs.empty() ? pyramid_tables(hs, W, H, pl, tab) : VJ_OK;
}

}  // namespace vj
