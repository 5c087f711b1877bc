// vj_run_windows: the clod profile's cascade on a caller's list of windows — what the shared driver
// (vj_points_driver.hpp) needs of the profile.  What needs no device is vj_points_host.cpp; the node tables are build_node_table's
// (vj_plan.cpp), as every other clod path builds them.
#include "vj_points_driver.hpp"

using namespace vj;

namespace {

struct ClodPoints {
    static constexpr const char* name = "vj_run_windows";
    typedef ClodPointScale Geom;
    typedef ClodPointScaleDev ScaleDev;
    typedef ClodPointResult Result;
    typedef ClodPointArgs Args;
    static constexpr int waves = CLOD_POINT_WAVES;
    static constexpr auto check = clod_points_check;
    static constexpr auto scatter = clod_points_scatter;
    static auto& cascades(vj_env* e) { return e->clod_point_cascades; }
    static auto& plans(vj_env* e) { return e->clod_point_plans; }
    static vj_env::ClodPointPlanKey plan_key(const vj_cascade* c, int W, float scale, uint32_t flags) {
        uint32_t bits;
        memcpy(&bits, &scale, 4);
        return vj_env::ClodPointPlanKey(c->uid, W, bits, (flags & VJ_FLAG_TILTED_AS_UPRIGHT) ? 1 : 0);
    }
    // the stage records the clod plans hold
    static void build_stages(const vj_cascade* c, const StageProgram& prog, const std::vector<uint32_t>& order, PointCascade* pc,
                             std::vector<StageDev>* stages) {
        const size_t n = c->stages.size();
        for (const auto& t : c->trees)
            if (t.n_nodes != 1) pc->trees = true;
        stages->resize(n);
        for (size_t s = 0; s < n; ++s) {
            const bool linear = prog.on_fail[s] == STAGE_REJECT && (prog.on_pass[s] == (int)s + 1 || (prog.on_pass[s] == STAGE_ACCEPT && s + 1 == n));
            if (!linear) pc->is_tree = true;
            StageDev& sd = (*stages)[s];
            memset(&sd, 0, sizeof(sd));
            sd.first_node = prog.first_node[s];
            sd.n_nodes = prog.n_nodes[s];
            sd.threshold = c->stages[s].threshold;
            sd.on_pass = prog.on_pass[s];
            sd.on_fail = prog.on_fail[s];
            sd.n_trees = (uint32_t)c->stages[s].n_trees;
            sd.order = s < order.size() ? order[s] : 0u;
        }
    }
    static int geometry(const vj_cascade* c, float scale, int W, int H, ClodPointScale* g) {
        return clod_point_scale(c->win_w, c->win_h, scale, W, H, g);
    }
    // precomputeKernelCascade (clod.cpp:529-578) reads the image only through its width
    static int build_scale(const vj_cascade* c, float scale, int W, const ClodPointScale& sc, ClodPointScaleDev* rec, NodeRec* table,
                           uint64_t* max_reach) {
        const uint32_t stride = (uint32_t)W + 1u;
        rec->area = (float)sc.area;
        rec->e_lt = (uint32_t)sc.ex * stride + (uint32_t)sc.ex;
        rec->e_dw = (uint32_t)sc.ew;
        rec->e_dh = (uint32_t)sc.eh * stride;
        vj_scale_info si;
        memset(&si, 0, sizeof(si));
        si.scale = scale;
        si.area = sc.area;
        si.accepted = 1;
        const int rc = build_node_table(*c, W, si, table);
        // furthest element a gather of this scale touches, from the window origin: the variance rectangle and every feature corner
        uint64_t reach = (uint64_t)rec->e_lt + rec->e_dh + rec->e_dw;
        for (size_t n = 0; n < c->nodes.size(); ++n) {
            const NodeRec& r = table[n];
            const uint32_t dw[3] = {r.dw01 & 0xffffu, r.dw01 >> 16, r.dw2_flags & 0xffffu};
            for (int q = 0; q < 3; ++q)
                if (q < 2 || r.w[2] != 0.0f) reach = std::max<uint64_t>(reach, ((uint64_t)r.lt[q] + r.dh[q] + dw[q]) / 4u);
        }
        *max_reach = reach;
        return rc;
    }
    static int extra_images(vj_env*, const PointCascade&, const uint8_t*, size_t, int, int, int, int, int) { return VJ_OK; }
    static void fill_args(const vj_env*, const PointCascade&, uint32_t flags, ClodPointArgs* a) {
        a->signed_mean = (flags & VJ_FLAG_SIGNED_MEAN) ? 1u : 0u;
    }
    static int launch(const ClodPointArgs& a, const PointCascade& pc, int n_blocks, void* stream) {
        return launch_clod_points_pass(a, pc.trees, pc.is_tree, n_blocks, stream);
    }
};

}  // namespace

extern "C" {

// runCascade + computeVariance on a caller's windows (clod.cpp:736-787, :418-446)
int vj_run_windows(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const float* scales, int n_scales,
                   const vj_window* windows, uint32_t n_windows, int start_stage, uint32_t flags, vj_clod_window_result* out) {
    if (refuse_equalize(flags, "vj_run_windows")) return VJ_ERR_UNSUPPORTED;
    return run_points<ClodPoints>(e, c, frames, n_frames, scales, n_scales, windows, n_windows, start_stage, flags, out);
}

}  // extern "C"
