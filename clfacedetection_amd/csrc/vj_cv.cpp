// Host driver of the OpenCV arithmetic profile: cvHaarDetectObjects' scale-cascade path as the reference
// keeps it in tempcv.cpp (its private copy of OpenCV 2.4.2 haar.cpp; call site main.cpp:145), on the GPU.
//   scale loop, window grid            tempcv.cpp:1344-1417
//   cvSetImagesForHaarClassifierCascade  tempcv.cpp:549-768 (equRect, cvRound-ed rectangles, f32 weights,
//                                        CV_ADJUST_WEIGHTS = 0; the "align blocks" flags can never be set:
//                                        kx = r0.width / base_w >= 1)
//   stage threshold bias               tempcv.cpp:262, 419
//   hidden-cascade flags               tempcv.cpp:410-470 (isStumpBased, is_tree, per-stage two_rects) — they select
//                                        the arithmetic of a node sum (vj_cv_profile.hip: cv_node_sum)
//   CV_HAAR_SCALE_IMAGE branch         tempcv.cpp:1257-1329, invoker :989-1113 (VJ_FLAG_CV_SCALE_IMAGE: the image pyramid in one canvas per
//                                        frame, vj_pyramid.hip; ONE node table at factor 1; exhaustive-grid tile and row kernels)
//   CV_HAAR_FIND_BIGGEST_OBJECT        tempcv.cpp:1353-1490 (VJ_FLAG_CV_FIND_BIGGEST, with VJ_FLAG_CV_ROUGH_SEARCH: the descending scale list, one round per
//                                        scale, per-frame search state on the device; detect_biggest below, vj_cv_biggest.hip)
// Stumps or multi-node trees, linear cascades or stage trees, upright or tilted features (tilted integral).
// Second arithmetic profile.  OpenCV itself is not available here or on the GPU box, so
// parity is against the oracle's restatement of the same lines (oc_detect_opencvlike): unpinned.
#include "vj_points_driver.hpp"
#include "vj_cv_roi_host.hpp"
#include "vj_cv_roi_levels_host.hpp"
#include "vj_cv_tq_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>

using namespace vj;

namespace {

// (the planner — scales, canvas, node tables, tile shapes, work lists, the pyramid's taps — needs no device: vj_cv_plan.cpp)

// What vj_detect_opencv_roc adds to a scale-image call: maxSize, and where the levels and weights of the reported
// windows go, parallel to the call's rectangles.
struct CvRocCall : CvMaxSize {
    std::vector<int32_t>* levels;
    std::vector<double>* weights;
};

// The device copies of a plan: every table at the size its kernels index, at least one element where a launch binds the pointer
// of an empty list.
static int upload_cv_plan(CvPlan* pl, const CvPlanTables& tab) {
    struct Row { DevBuf* buf; const void* src; size_t bytes, min_bytes; };
    const Row rows[] = {
        {&pl->d_table, tab.table.data(), tab.table.size() * sizeof(CvNodeRec), sizeof(CvNodeRec)},
        {&pl->d_scales, pl->scales.data(), pl->scales.size() * sizeof(CvScaleDev), sizeof(CvScaleDev)},
        {&pl->d_stages, tab.stages.data(), tab.stages.size() * sizeof(StageDev), 0},
        {&pl->d_rows, tab.rows.data(), tab.rows.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_tiles, tab.tiles.data(), tab.tiles.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_rows_rest, tab.rows_rest.data(), tab.rows_rest.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_bit_segs, tab.bit_segs.data(), tab.bit_segs.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_prune, tab.prune.data(), tab.prune.size() * sizeof(CvPruneDev), 0},
        {&pl->d_pyr_levels, tab.pyr_levels.data(), tab.pyr_levels.size() * sizeof(PyrLevelDev), 0},
        {&pl->d_pyr_taps, tab.pyr_taps.data(), tab.pyr_taps.size() * sizeof(PyrTap), 0},
    };
    for (const Row& r : rows) {
        const size_t want = std::max(r.bytes, r.min_bytes);
        if (!want) continue;   // (an empty list nothing binds)
        if (const int rc = r.buf->ensure(want)) return rc;
        if (r.bytes) HIP_TRY(hipMemcpy(r.buf->p, r.src, r.bytes, hipMemcpyHostToDevice));
    }
    return VJ_OK;
}

static int get_cv_plan(vj_env* e, const vj_cascade* c, int W, int H, const vj_cv_params* p, int n_frames, CvPlan** out,
                       const CvRocCall* roc = nullptr) {
    uint64_t sf_bits;
    memcpy(&sf_bits, &p->scale_factor, 8);
    const bool small_batch = n_frames <= 4;
    const bool fb = (p->flags & VJ_FLAG_CV_FIND_BIGGEST) != 0u;   // (rough search changes no table: it is read per call)
    const bool si = !fb && (p->flags & VJ_FLAG_CV_SCALE_IMAGE) != 0u;
    const bool prune = !fb && !si && (p->flags & VJ_FLAG_CV_CANNY_PRUNING) != 0u;
    // (a find-biggest plan depends on neither minSize — the break is the waves' — nor the batch-size class: one plan for all)
    const vj_env::CvPlanKey key(c->uid, W, H, fb ? 0 : p->min_w, fb ? 0 : p->min_h, sf_bits,
                                fb ? 8 : (small_batch ? 1 : 0) | (prune ? 2 : 0) | (si ? 4 : 0) | (roc ? 16 : 0),
                                roc ? cv_max_level_end(c, W, H, p->scale_factor, roc->max_w, roc->max_h) : -1);
    auto it = e->cv_plans.find(key);
    if (it != e->cv_plans.end()) {
        it->second->last_used = ++e->plan_tick;
        *out = it->second.get();
        return VJ_OK;
    }
    if ((int)e->cv_plans.size() >= std::max(1, e->plan_cache_max)) {   // bounded: the least recently used plans go first
        HIP_TRY(hipStreamSynchronize(e->stream));
        cache_make_room(e, e->cv_plans);
    }
    auto pl = std::make_unique<CvPlan>();
    CvPlanTables tab;
    int rc = plan_cv(*e, c, W, H, *p, small_batch, roc, pl.get(), &tab);
    if (!rc) rc = upload_cv_plan(pl.get(), tab);
    if (rc) {
        pl->release_device();
        return rc;
    }
    pl->last_used = ++e->plan_tick;
    *out = pl.get();
    e->cv_plans[key] = std::move(pl);
    return VJ_OK;
}

// The edge maps of `nf` frames already on the device (cvCanny(gray, edges, 0, 50, 3), vj_canny.hip) into e->d_edges: 0 / 255 bytes,
// rows of *pitch bytes, frames pitch * H bytes apart.
static int enqueue_canny(vj_env* e, const uint8_t* d_gray, size_t gray_frame_bytes, int gray_stride, int W, int H, int nf, int CH,
                         uint32_t* pitch) {
    const size_t px = (size_t)W * (size_t)H * (size_t)nf;
    const uint32_t ep = ((uint32_t)W + 3u) & ~3u;
    int rc;
    if ((rc = e->d_canny_cls.ensure(px))) return rc;
    if ((rc = e->d_canny_label.ensure(px * 4u))) return rc;
    if ((rc = e->d_canny_flag.ensure(px))) return rc;
    if ((rc = e->d_edges.ensure((size_t)ep * (size_t)H * (size_t)nf))) return rc;
    CannyArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.gray = d_gray;
    ca.gray_frame_bytes = gray_frame_bytes;
    ca.gray_stride = (uint32_t)gray_stride;
    ca.channels = (uint32_t)CH;
    ca.width = (uint32_t)W;
    ca.height = (uint32_t)H;
    ca.n_frames = (uint32_t)nf;
    ca.cls = (uint8_t*)e->d_canny_cls.p;
    ca.label = (uint32_t*)e->d_canny_label.p;
    ca.flag = (uint8_t*)e->d_canny_flag.p;
    ca.edges = (uint8_t*)e->d_edges.p;
    ca.edge_pitch = ep;
    ca.edge_frame_bytes = (uint64_t)ep * (uint64_t)H;
    const int hrc = launch_canny(ca, e->stream);
    if (hrc) {
        set_error("canny launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    *pitch = ep;
    return VJ_OK;
}

// The u32 integral of the edge maps into e->d_edge_sum (d_sum's geometry, zeroed slack rows): the banded integral kernels' sum-only
// instances (launch_integral_sum); the band arrays are scratch shared with enqueue_integral on the same stream.
static int enqueue_edge_integral(vj_env* e, uint32_t pitch, int W, int H, int nf) {
    const uint32_t fe = frame_elems_for(W, H);
    int rc;
    if ((rc = e->d_edge_sum.ensure((size_t)fe * 4u * (size_t)nf))) return rc;
    const size_t used = (size_t)(W + 1) * (size_t)(H + 1);
    const bool zeroed = e->edge_slack_w == W && e->edge_slack_h == H && e->edge_slack_frames >= nf && e->edge_slack_sum == e->d_edge_sum.p;
    for (int f = 0; f < nf && !zeroed; ++f)
        HIP_TRY(hipMemsetAsync((uint32_t*)e->d_edge_sum.p + (size_t)f * fe + used, 0, (fe - used) * 4, e->stream));
    if (!zeroed) {
        e->edge_slack_w = W;
        e->edge_slack_h = H;
        e->edge_slack_frames = nf;
        e->edge_slack_sum = e->d_edge_sum.p;
    }
    IntegralArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.channels = 1;
    ia.gray = (const uint8_t*)e->d_edges.p;
    ia.gray_frame_bytes = (uint64_t)pitch * (uint64_t)H;
    ia.gray_stride = pitch;
    ia.width = (uint32_t)W;
    ia.height = (uint32_t)H;
    ia.n_frames = (uint32_t)nf;
    ia.n_bands = ((uint32_t)H + BAND_ROWS - 1) / BAND_ROWS;
    ia.band_pitch = ((uint32_t)W + 3u) & ~3u;
    ia.band_sum = (uint32_t*)e->d_band_sum.p;
    ia.sum = (uint32_t*)e->d_edge_sum.p;
    ia.frame_elems = fe;
    const int hrc = launch_integral_sum(ia, e->stream);
    if (hrc) {
        set_error("edge integral launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

// What stage_frames needs of ensure_image_buffers: the lane's staging buffer for `frames` frames at the device's pitch
int ensure_gray_staging(vj_env* e, int W, int H, int frames, int channels) {
    const size_t gstride = ((size_t)W * (size_t)channels + 3) & ~(size_t)3;
    return e->lane0.d_gray.ensure(gstride * (size_t)H * (size_t)frames);
}

// The pyramid launch (vj_pyramid.hip): the levels `d_levels` / `d_taps` describe, of `nf` frames already on the device, into
// e->d_pyr: canvases of pitch * ch bytes.  What no level covers is left as it is: the integral kernels read it, but no rectangle sum
// inside a level depends on it.
int enqueue_pyramid(vj_env* e, const uint8_t* d_gray, size_t gray_frame_bytes, int gray_stride, int W, int H, int nf, int CH,
                    const void* d_levels, const void* d_taps, uint32_t n_levels, uint32_t n_units, uint32_t cw, uint32_t ch, uint32_t pitch) {
    const size_t bytes = (size_t)pitch * (size_t)ch * (size_t)nf;
    int rc;
    if ((rc = e->d_pyr.ensure(bytes))) return rc;
    PyrArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.gray = d_gray;
    pa.gray_frame_bytes = gray_frame_bytes;
    pa.gray_stride = (uint32_t)gray_stride;
    pa.channels = (uint32_t)CH;
    pa.width = (uint32_t)W;
    pa.height = (uint32_t)H;
    pa.n_frames = (uint32_t)nf;
    pa.levels = (const PyrLevelDev*)d_levels;
    pa.n_levels = n_levels;
    pa.n_units = n_units;
    pa.taps = (const PyrTap*)d_taps;
    pa.canvas = (uint8_t*)e->d_pyr.p;
    pa.canvas_pitch = pitch;
    pa.canvas_w = cw;
    pa.canvas_h = ch;
    pa.canvas_frame_bytes = (uint64_t)pitch * (uint64_t)ch;
    const int hrc = launch_pyramid(pa, e->stream);
    if (hrc) {
        set_error("pyramid launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

// The prune-bitmap kernels' arguments for the tile scales of this sub-batch (e->d_cv_prune_bits: the skip bitmap's size)
static CvPruneArgs prune_args(vj_env* e, const CvPlan* pl, const CvArgs& a, int nf, unsigned long long* windows) {
    CvPruneArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.sum = a.sum;
    pa.edge_sum = a.edge_sum;
    pa.scales = a.scales;
    pa.prune = a.prune;
    pa.segs = (const UnitDev*)pl->d_bit_segs.p;
    pa.n_segs = pl->n_bit_segs;
    pa.n_frames = (uint32_t)nf;
    pa.frame_elems = a.frame_elems;
    pa.stride = a.stride;
    pa.bits_frame_words = pl->bits_frame_words;
    pa.bits = (unsigned long long*)e->d_skip_bits.p;
    pa.prune_bits = (unsigned long long*)e->d_cv_prune_bits.p;
    pa.windows = windows;
    return pa;
}

// ------------------------------------------------------------------------ what the passes of this file share
// A cascade's shape as the argument rules below read it: of a CvPlan, a CvRoiPlan, a PointCascade or a CvShape
struct CvFacts { bool has_tilted, is_tree, tree2; };
template <class P> static CvFacts facts_of(const P& p) { return CvFacts{p.has_tilted, p.is_tree, p.tree2}; }

// The three fields every pass of the profile derives from the shape and the tunables (CvArgs and CvPointArgs)
template <class A> static void fill_shape_args(const vj_env* e, const CvFacts& f, A* a) {
    a->tilted = f.has_tilted ? (const uint32_t*)e->d_tilted.p : nullptr;
    a->tail_max = (uint32_t)std::max(0, std::min(e->cv_tail_max, (int)CV_TAIL_MAX));
    a->tree2 = f.tree2 && !f.is_tree && !f.has_tilted && e->cv_tree2 ? 1u : 0u;
}

struct CvTables { const void *table, *scales, *stages; uint32_t n_order, n_stages; };
struct CvGeom { uint32_t frame_elems, stride, sum_h, n_frames; };

// The CvArgs every pass starts from: the environment's integral images, a plan's tables, the geometry, and where detections and
// counters go (counts: stage_entered [VJ_MAX_STAGES] | visited ... | the detection count).  rows / total_waves and whatever one
// path adds are the caller's.
static CvArgs cv_base_args(const vj_env* e, const CvFacts& f, const CvTables& t, const CvGeom& g, void* det, uint32_t det_cap, void* counts) {
    CvArgs a;
    memset(&a, 0, sizeof(a));
    a.sum = (const uint32_t*)e->d_sum.p;
    a.sqsum = (const uint64_t*)e->d_sqsum.p;
    a.n_order = t.n_order;
    a.table = (const uint32_t*)t.table;
    a.scales = (const CvScaleDev*)t.scales;
    a.stages = (const StageDev*)t.stages;
    a.n_frames = g.n_frames;
    a.n_stages = t.n_stages;
    a.frame_elems = g.frame_elems;
    a.stride = g.stride;
    a.sum_h = g.sum_h;
    a.det = (CvDet*)det;
    a.det_count = (uint32_t*)((unsigned long long*)counts + 2 * VJ_MAX_STAGES);
    a.det_cap = det_cap;
    a.stage_entered = (unsigned long long*)counts;
    fill_shape_args(e, f, &a);
    return a;
}
template <class Plan> static CvTables tables_of(const Plan* pl) {
    return CvTables{pl->d_table.p, pl->d_scales.p, pl->d_stages.p, pl->n_order, pl->n_stages};
}

static int cascade_launched(int hrc) {
    if (!hrc) return VJ_OK;
    set_error("cascade launch failed: %s", hipGetErrorString((hipError_t)hrc));
    return VJ_ERR_HIP;
}

// Frames per sub-batch: 32-bit byte offsets into the batch's sum images, and the configured "max_subbatch"
static int cv_max_frames(const vj_env* e, int n_frames, uint32_t frame_elems) {
    const int m = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_frames, 0xfffffff0ull / ((uint64_t)frame_elems * 4u)));
    return e->max_subbatch > 0 ? std::min(m, e->max_subbatch) : m;
}

// A sub-batch's way onto the device, between lane0.ev[0] and ev[1]: the frames staged, VJ_FLAG_EQUALIZE_HIST, then — with a plan
// that has them — the pyramid of CV_HAAR_SCALE_IMAGE (from there on the "frames" are the gray canvases, and the integral images
// are theirs) or the edge maps and their integral, then the integrals.
static int enqueue_cv_ingest(vj_env* e, const vj_image* frames, int nf, int W, int H, int CH, bool equalize, const CvPlan* pl, bool tilted) {
    const bool si = pl && pl->scale_image;
    const int IW = si ? (int)pl->canvas_w : W, IH = si ? (int)pl->canvas_h : H;
    int rc;
    if (si) {   // the frames' gray staging alone; the integral buffers are the canvases'
        if ((rc = ensure_gray_staging(e, W, H, nf, CH))) return rc;
        if ((rc = ensure_image_buffers(e, IW, IH, nf, false))) return rc;
    } else if ((rc = ensure_image_buffers(e, W, H, nf, true, CH))) {
        return rc;
    }
    const uint8_t* d_gray;
    size_t gray_frame_bytes;
    int gray_stride;
    int gray_ch = CH;
    if ((rc = stage_frames(e, frames, nf, W, H, &d_gray, &gray_frame_bytes, &gray_stride))) return rc;
    HIP_TRY(hipEventRecord(e->lane0.ev[0], e->stream));
    // VJ_FLAG_EQUALIZE_HIST: from here on the frames are the lane's equalized gray batch
    if (equalize && (rc = enqueue_equalize(e, nullptr, &d_gray, &gray_frame_bytes, &gray_stride, &gray_ch, W, H, nf))) return rc;
    if (si) {   // every level of every frame
        if ((rc = enqueue_pyramid(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, gray_ch, pl->d_pyr_levels.p, pl->d_pyr_taps.p,
                                  pl->n_pyr_levels, pl->n_pyr_units, pl->canvas_w, pl->canvas_h, pl->canvas_pitch)))
            return rc;
        d_gray = (const uint8_t*)e->d_pyr.p;
        gray_frame_bytes = (size_t)pl->canvas_pitch * (size_t)IH;
        gray_stride = (int)pl->canvas_pitch;
        gray_ch = 1;
    }
    if (pl && pl->prune) {   // the edge maps and their integral
        uint32_t pitch = 0;
        if ((rc = enqueue_canny(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, gray_ch, &pitch))) return rc;
        if ((rc = enqueue_edge_integral(e, pitch, W, H, nf))) return rc;
    }
    if ((rc = enqueue_integral(e, d_gray, gray_frame_bytes, gray_stride, IW, IH, nf, gray_ch))) return rc;
    if (tilted && (rc = enqueue_tilted(e, d_gray, gray_frame_bytes, gray_stride, IW, IH, nf, gray_ch))) return rc;
    HIP_TRY(hipEventRecord(e->lane0.ev[1], e->stream));
    return VJ_OK;
}

// After a pass's launches: its counters on the host (e->d_cv_counts, `counts_bytes` of them) once the stream has drained, and the
// number of detections it reported — which may be more than the buffer held.
static int read_cv_counts(vj_env* e, size_t counts_bytes, std::vector<unsigned long long>* h, uint32_t* n_det) {
    h->resize((counts_bytes + 7) / 8);
    HIP_TRY(hipMemcpyAsync(h->data(), e->d_cv_counts.p, counts_bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *n_det = (uint32_t)((*h)[2 * VJ_MAX_STAGES] & 0xffffffffull);
    return VJ_OK;
}

// One pass until its detections fit.  Per attempt: e->d_cv_det for *det_cap records, the counters zeroed, enqueue(*det_cap) — the
// launches — between lane0.ev[2] and ev[3], the counters read back; more detections than *det_cap: the capacity grown, once more.
// `twice`: the error of the case that cannot happen (the count of a repeated pass is the count that sized its buffer).
template <class Enqueue>
static int run_cv_pass_until_fit(vj_env* e, size_t counts_bytes, uint32_t* det_cap, const char* twice, Enqueue&& enqueue,
                                 std::vector<unsigned long long>* h, uint32_t* n_det) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        int rc;
        if ((rc = e->d_cv_det.ensure((size_t)*det_cap * sizeof(CvDet)))) return rc;
        HIP_TRY(hipMemsetAsync(e->d_cv_counts.p, 0, counts_bytes, e->stream));
        HIP_TRY(hipEventRecord(e->lane0.ev[2], e->stream));
        if ((rc = enqueue(*det_cap))) return rc;
        HIP_TRY(hipEventRecord(e->lane0.ev[3], e->stream));
        if ((rc = read_cv_counts(e, counts_bytes, h, n_det))) return rc;
        if (*n_det <= *det_cap) return VJ_OK;
        *det_cap = grown_cap(*det_cap, *n_det);   // overflow: grow and run the pass again
    }
    set_error("%s", twice);
    return VJ_ERR_LIMIT;
}

static void add_cv_counters(const std::vector<unsigned long long>& h, size_t n_stages, vj_counters* k) {
    for (size_t s = 0; s < n_stages; ++s) k->stage_entered[s] += h[s];
    k->windows += h[VJ_MAX_STAGES];
}

template <class Det> static int read_cv_dets(vj_env* e, uint32_t n_det, std::vector<Det>* raw) {
    raw->resize(n_det);
    if (n_det) HIP_TRY(hipMemcpy(raw->data(), e->d_cv_det.p, (size_t)n_det * sizeof(Det), hipMemcpyDeviceToHost));
    return VJ_OK;
}


// CV_HAAR_FIND_BIGGEST_OBJECT (VJ_FLAG_CV_FIND_BIGGEST; tempcv.cpp:1353-1490).  Per sub-batch: the integrals, then
// one round per scale of the descending list — cv_biggest_pass and the grouping step cv_biggest_update — all enqueued up front;
// the frames' search states live on the device and steer the kernels, the host reads nothing until the last round is done.  Then
// step 5 on the host: a frame's candidates in the walk's order, maxRect behind the scale that found it, groupRectangles, the
// first group of strictly greatest area.
static int detect_biggest(vj_env* e, const vj_cascade* c, CvPlan* pl, const vj_image* frames, int n_frames, int W, int H, int CH,
                          const vj_cv_params* p, bool equalize, vj_result* out) {
    const std::vector<CvScaleDev>& scales = pl->scales;
    const uint32_t stride = (uint32_t)W + 1u;
    const uint32_t frame_elems = frame_elems_for(W, H);
    const bool count = (p->flags & VJ_FLAG_COUNTERS) != 0;
    const int threshold = (int)std::max<uint32_t>(p->min_neighbors, 1u);
    DevBuf& d_det = e->d_cv_det;
    DevBuf& d_counts = e->d_cv_counts;
    const size_t counts_bytes = 2 * VJ_MAX_STAGES * sizeof(uint64_t);   // stage_entered | visited
    int rc;
    if ((rc = d_counts.ensure(counts_bytes))) return rc;
    const int max_frames = cv_max_frames(e, n_frames, frame_elems);
    // a frame's segment of the detection buffer: what a search may hold before its first grouped object (GROUP_MAX) and as much
    // again for the scanROI's candidates, or the configured start ("det_cap"); a fuller frame repeats the sub-batch with more room
    uint32_t frame_cap = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(e->det_cap_init, 2u * GROUP_MAX));
    std::vector<vj_rect> all;
    std::vector<unsigned long long> h(counts_bytes / 8);
    std::vector<CvBigState> st;
    std::vector<uint32_t> fc;
    std::vector<CvDet> raw;
    out->timing.n_cascade_launches = 0;
    for (int f0 = 0, nf = 0; f0 < n_frames && !scales.empty(); f0 += nf) {
        nf = std::min(max_frames, n_frames - f0);
        if ((rc = enqueue_cv_ingest(e, frames + f0, nf, W, H, CH, equalize, pl, pl->has_tilted))) return rc;   // (a find-biggest plan: neither pyramid nor edge maps)
        const size_t state_bytes = (size_t)nf * sizeof(CvBigState), big_bytes = state_bytes + (size_t)nf * sizeof(uint32_t);
        if ((rc = e->d_cv_big.ensure(big_bytes))) return rc;
        st.resize((size_t)nf);
        fc.resize((size_t)nf);
        for (;;) {
            if ((uint64_t)frame_cap * (uint64_t)nf * sizeof(CvDet) > (1ull << 40)) {
                set_error("vj_detect_opencv: the candidate buffer of the find-biggest search would exceed 1 TiB");
                return VJ_ERR_LIMIT;
            }
            if ((rc = d_det.ensure((size_t)frame_cap * (size_t)nf * sizeof(CvDet)))) return rc;
            HIP_TRY(hipMemsetAsync(d_counts.p, 0, counts_bytes, e->stream));
            HIP_TRY(hipMemsetAsync(e->d_cv_big.p, 0, big_bytes, e->stream));
            CvBigArgs b;
            memset(&b, 0, sizeof(b));
            CvArgs& a = b.cv;
            a = cv_base_args(e, facts_of(*pl), tables_of(pl), CvGeom{frame_elems, stride, (uint32_t)H + 1u, (uint32_t)nf}, d_det.p, frame_cap, d_counts.p);
            a.det_count = nullptr;   // (every frame's segment has a counter of its own: b.frame_count; the counters end with `visited`)
            b.state = (CvBigState*)e->d_cv_big.p;
            b.frame_count = (uint32_t*)((char*)e->d_cv_big.p + state_bytes);
            b.min_w = p->min_w;
            b.min_h = p->min_h;
            b.width = (uint32_t)W;
            b.height = (uint32_t)H;
            b.threshold = threshold;
            b.rough = (p->flags & VJ_FLAG_CV_ROUGH_SEARCH) != 0u ? 1u : 0u;
            b.eps = 0.2;
            HIP_TRY(hipEventRecord(e->lane0.ev[2], e->stream));
            int launches = 0;
            for (size_t k = 0; k < scales.size(); ++k) {
                b.slot = (uint32_t)k;
                // one wave per (frame, window row) of the scale, at most four workgroups per CU (the rest by stride)
                const uint64_t waves = (uint64_t)scales[k].end_y * (uint64_t)nf;
                const int n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((waves + CV_WAVES_PER_BLOCK - 1) / CV_WAVES_PER_BLOCK, (uint64_t)std::max(1, e->n_cu * 4)));
                a.total_waves = (uint32_t)n_blocks * CV_WAVES_PER_BLOCK;
                // (the grouping step follows EVERY scale, the last one too, :1422-1454: a frame that first groups there still gets its
                // maxRect pushed before step 5, which counts it among the neighbors)
                if ((rc = cascade_launched(launch_cv_biggest_round(b, pl->trees, count, pl->is_tree, n_blocks, true, e->stream)))) return rc;
                launches += 2;
            }
            HIP_TRY(hipEventRecord(e->lane0.ev[3], e->stream));
            HIP_TRY(hipMemcpyAsync(h.data(), d_counts.p, counts_bytes, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync(st.data(), b.state, state_bytes, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync(fc.data(), b.frame_count, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            uint32_t most = 0;
            for (int f = 0; f < nf; ++f) {
                most = std::max(most, fc[(size_t)f]);
                if (st[(size_t)f].flags & CV_BIG_LIMIT) {
                    set_error("vj_detect_opencv: frame %d holds %u candidates before its first grouped object; the find-biggest search groups at most %u on the device",
                              f0 + f, fc[(size_t)f], GROUP_MAX);
                    return VJ_ERR_LIMIT;
                }
            }
            if (most > frame_cap) {   // some frame's segment overflowed: the sub-batch's rounds again with room for it
                frame_cap = grown_cap(frame_cap, most);
                continue;
            }
            float ms_i = 0, ms_c = 0, ms_t = 0;
            HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms_c, e->lane0.ev[2], e->lane0.ev[3]));
            HIP_TRY(hipEventElapsedTime(&ms_t, e->lane0.ev[0], e->lane0.ev[3]));
            out->timing.integral_ms += ms_i;
            out->timing.cascade_ms += ms_c;
            out->timing.total_ms += ms_t;
            out->timing.n_cascade_launches += launches;
            if (count) add_cv_counters(h, pl->n_stages, &out->counters);
            break;
        }
        // ---- step 5 (tempcv.cpp:1458-1490), frame by frame
        // (one strided copy of the head of every segment, as long as the fullest frame's list — not the whole segments; none at all
        // when no frame has a candidate)
        uint32_t most = 0;
        for (int f = 0; f < nf; ++f) most = std::max(most, fc[(size_t)f]);   // (<= frame_cap here)
        raw.resize((size_t)most * (size_t)nf);
        if (most != 0u)
            HIP_TRY(hipMemcpy2D(raw.data(), (size_t)most * sizeof(CvDet), d_det.p, (size_t)frame_cap * sizeof(CvDet), (size_t)most * sizeof(CvDet),
                                (size_t)nf, hipMemcpyDeviceToHost));
        for (int f = 0; f < nf; ++f) {
            const uint32_t n = fc[(size_t)f];
            if (n == 0u) continue;
            CvDet* d0 = raw.data() + (size_t)f * most;
            std::sort(d0, d0 + n, [](const CvDet& x, const CvDet& y) { return std::tie(x.slot, x.y, x.x) < std::tie(y.slot, y.y, y.x); });
            const CvBigState& s = st[(size_t)f];
            std::vector<vj_rect> cand;
            cand.reserve(n + 1u);
            bool pushed = s.phase != 1u;
            for (uint32_t i = 0; i <= n; ++i) {
                if (!pushed && (i == n || d0[i].slot > s.hit_slot)) {   // maxRect follows the candidates of the scale that found it
                    cand.push_back(vj_rect{s.max_x, s.max_y, s.max_w, s.max_h, 0.0f, f0 + f, -1});
                    pushed = true;
                }
                if (i < n)
                    cand.push_back(vj_rect{(int32_t)d0[i].x, (int32_t)d0[i].y, (int32_t)scales[d0[i].slot].win_w, (int32_t)scales[d0[i].slot].win_h, 0.0f,
                                           f0 + f, -1});
            }
            uint32_t m = (uint32_t)cand.size();
            if ((rc = vj_group_rectangles(cand.data(), &m, threshold, 0.2))) return rc;
            const vj_rect* best = nullptr;
            for (uint32_t i = 0; i < m; ++i)
                if ((int64_t)cand[i].w * cand[i].h > (best ? (int64_t)best->w * best->h : 0)) best = &cand[i];
            if (best) all.push_back(*best);
        }
    }
    return cv_result_epilogue(all, count ? &pl->prog : nullptr, out);
}

}  // namespace

extern "C" {

int vj_canny(vj_env* e, const vj_image* image, uint8_t* edges, int edges_stride) {
    if (!e || !image || !image->data || !edges || edges_stride < image->width) return VJ_ERR_ARG;
    int ch, rc;
    if ((rc = check_single_image(image, &ch))) return rc;
    const int w = image->width, h = image->height;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_image_buffers(e, w, h, 1, true, ch))) return rc;
    const uint8_t* d_src;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_src, &fb, &gs))) return rc;
    uint32_t pitch = 0;
    if ((rc = enqueue_canny(e, d_src, fb, gs, w, h, 1, ch, &pitch))) return rc;
    HIP_TRY(hipMemcpy2DAsync(edges, (size_t)edges_stride, e->d_edges.p, pitch, (size_t)w, (size_t)h, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return VJ_OK;
}

int vj_resize_linear(vj_env* e, const vj_image* image, int dst_w, int dst_h, uint8_t* dst, int dst_stride) {
    if (!e || !image || !image->data || !dst || dst_w <= 0 || dst_h <= 0 || dst_stride < dst_w) return VJ_ERR_ARG;
    int ch, rc;
    if ((rc = check_single_image(image, &ch))) return rc;
    const int w = image->width, h = image->height;
    if (w > 65535 || h > 65535 || dst_w > 65535 || dst_h > 65535 || (uint64_t)(dst_w + 3) * (uint64_t)dst_h >= (1ull << 31)) {
        set_error("vj_resize_linear: sizes up to 65535 x 65535 and 2^31 bytes");
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_gray_staging(e, w, h, 1, ch))) return rc;
    const uint8_t* d_src;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_src, &fb, &gs))) return rc;
    // one level at the canvas's origin: level record, then the columns' and the rows' taps
    const bool area = resize_is_area(w, h, dst_w, dst_h);
    static_assert(sizeof(PyrLevelDev) % sizeof(PyrTap) == 0, "the taps follow the level record");
    const size_t lv_taps = sizeof(PyrLevelDev) / sizeof(PyrTap);
    std::vector<PyrTap> tab(lv_taps + (size_t)dst_w + (size_t)dst_h);
    const PyrLevelDev lv{0u, 0u, (uint32_t)dst_w, (uint32_t)dst_h, 0u, (uint32_t)dst_w, 0u, area ? 1u : 0u};
    memcpy(tab.data(), &lv, sizeof(lv));
    build_taps(w, dst_w, false, area, tab.data() + lv_taps);
    build_taps(h, dst_h, true, area, tab.data() + lv_taps + dst_w);
    if ((rc = e->d_pyr_tab.ensure(tab.size() * sizeof(PyrTap)))) return rc;
    HIP_TRY(hipMemcpyAsync(e->d_pyr_tab.p, tab.data(), tab.size() * sizeof(PyrTap), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));   // (`tab` is pageable and leaves scope)
    const uint32_t pitch = ((uint32_t)dst_w + 3u) & ~3u;
    const uint32_t units = (uint32_t)((dst_w + PYR_UNIT_PX - 1) / PYR_UNIT_PX) * (uint32_t)dst_h;
    if ((rc = enqueue_pyramid(e, d_src, fb, gs, w, h, 1, ch, e->d_pyr_tab.p, (const PyrTap*)e->d_pyr_tab.p + lv_taps, 1u, units,
                              (uint32_t)dst_w, (uint32_t)dst_h, pitch)))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)dst_stride, e->d_pyr.p, pitch, (size_t)dst_w, (size_t)dst_h, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return VJ_OK;
}

void vj_cv_params_default(vj_cv_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->scale_factor = 1.1;
}

int vj_cv_plan_info_get(vj_env* e, const vj_cascade* c, int width, int height, int n_frames, const vj_cv_params* p,
                        vj_cv_plan_info* out) {
    if (!e || !c || !p || !out || n_frames <= 0 || width <= 0 || height <= 0 || width >= 65535 || height >= 65535) return VJ_ERR_ARG;
    if (!(p->scale_factor > 1.0)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    HIP_TRY(hipSetDevice(e->device));
    CvPlan* pl;
    const int rc = get_cv_plan(e, c, width, height, p, n_frames, &pl);
    if (rc) return rc;
    out->tile_windows = pl->tile_windows;
    out->n_tile_scales = pl->n_tile_scales;
    out->tree_prefix = pl->tree_prefix;
    if (pl->is_tree && pl->n_tile_scales != 0 && pl->class_first[2] != 0)   // as vj_detect_opencv chooses (uncounted calls)
        out->tree_queue = pl->chains.n != 0u && pl->n_tile_scales <= 64u && e->cv_tree_queue_cap <= 0 && e->cv_tree_chains ? 1 : 2;
    out->tq_shift = pl->tq_shift;
    out->tq_split_frames = pl->tq_split_frames;
    return VJ_OK;
}

}  // extern "C"

namespace {

// vj_detect_opencv_chain's hook into vj_detect_opencv: called after every sub-batch of frames [f0, f0 + nf) while its integral images
// (sum, sqsum and, with need_tilted, the tilted integral) are still on the device, with the sub-batch's raw candidates (unsorted;
// rect.frame counts from the call's first frame).
typedef std::function<int(int f0, int nf, const vj_rect* raw, size_t n_raw)> CvSubBatchHook;

// vj_detect_opencv_chain with VJ_FLAG_CV_CHAIN_DEVICE: what vj_detect_opencv's sub-batch loop calls so that the
// second cascade is enqueued behind the first before the host waits.  Per attempt at a sub-batch: enqueue() behind the first
// cascade's launches (hand-off kernels, vj_cv_chain.hip, then the region pass; the state block and the second cascade's counters
// are copied back on the stream), check() after the synchronisation (a short buffer: grown, *again; a frame the device does not
// group: the sub-batch goes through the host hook), finish() once the first cascade's result of the sub-batch stands.
struct CvChainDevice {
    vj_env* e = nullptr;
    const vj_cascade* second = nullptr;
    const vj_cv_params* p_second = nullptr;   // (flags: VJ_FLAG_COUNTERS at most)
    bool grouped = false;                     // p_first->min_neighbors != 0
    int32_t threshold = 1;                    // max(min_neighbors, 1)
    int W = 0, H = 0;
    CvRoiPlan* rp = nullptr;                  // the second cascade's tables; its factor table is on the device (begin())
    const CvSubBatchHook* host_hook = nullptr;
    vj_result* out_second = nullptr;
    std::vector<vj_rect>* all2 = nullptr;     // the second cascade's candidates (rect.frame = index in out_first)
    std::vector<vj_rect>* regions = nullptr;  // grouped: the regions of every sub-batch so far — out_first's rectangles
    uint32_t unit_cap = 0, det2_cap = 0;
    bool fallback = false;                    // this sub-batch is redone through the host hook
    CvChainState h_state = {};
    std::vector<unsigned long long> h_counts2;
    int begin();
    int enqueue(int nf, const CvPlan* pl, const CvArgs& a, uint32_t det_cap);
    int check(bool* again);
    int finish(int f0, int nf, const vj_rect* raw, size_t n_raw, size_t base);
};

// ------------------------------------------------------------------------ vj_detect_opencv
// What the functions of one call share
struct CvCall {
    vj_env* e;
    const vj_image* frames;
    const vj_cv_params* p;            // (without VJ_FLAG_EQUALIZE_HIST)
    vj_result* out;
    bool equalize, need_tilted, count;
    const CvSubBatchHook* hook;
    const CvRocCall* roc;
    CvChainDevice* dev;
    CvPlan* pl;
    int W, H, CH;
    int IH;                           // rows the integral images cover (CV_HAAR_SCALE_IMAGE: the canvas that holds the pyramid's levels)
    uint32_t stride, frame_elems;
    int max_frames;                   // frames per sub-batch (the tree queue may lower it: CvTqSizing::RESPLIT)
    uint32_t det_cap;
    std::vector<vj_rect> all;
    std::vector<int32_t> all_levels;  // (ROC) parallel to `all`
    std::vector<double> all_weights;
};
// counters: stage_entered[VJ_MAX_STAGES] | visited | ... | detection count | pad | 4 x 8 tile ticket counters
// ... | 64 tree-queue counters (one per tile scale) | chain-pass ticket
constexpr size_t CV_COUNTS_BYTES = 2 * VJ_MAX_STAGES * sizeof(uint64_t) + 16 + 4 * 8 * sizeof(uint32_t) + 64 * sizeof(uint32_t) + 16;

// One attempt at a sub-batch as it was enqueued, or why it was not
struct CvAttempt {
    enum { LAUNCHED, ROWS_ONLY /* the same attempt again on the rows */, RESPLIT /* the same frames again, cc.max_frames at a time */ } outcome = LAUNCHED;
    CvArgs a;
    uint32_t tq_cap = 0;        // != 0: stage-tree tiles, with a survivor queue of this many entries ...
    bool chain_pass = false;    // ... as one sub-queue per scale (cv_tree_chain_pass), else one flat queue (cv_tree_walk)
};

static int check_cv_call(const vj_image* frames, int n_frames, const vj_cv_params* p, int* W_out, int* H_out, int* CH_out) {
    if (!(p->scale_factor > 1.0)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    const int W = frames[0].width, H = frames[0].height;
    if (W <= 0 || H <= 0 || W >= 65535 || H >= 65535) return VJ_ERR_ARG;
    if ((uint64_t)(W + 1) * (uint64_t)(H + 3) >= (1ull << 30)) {   // the limit of vj_detect (check_frames): 32-bit byte offsets
        set_error("image too large");                              // into one frame's sum image
        return VJ_ERR_LIMIT;
    }
    const int CH = image_channels(frames[0]);
    for (int i = 0; i < n_frames; ++i)
        if (!frames[i].data || frames[i].width != W || frames[i].height != H || image_channels(frames[i]) != CH ||
            (CH != 1 && CH != 3 && CH != 4) || frames[i].stride < W * CH) {
            set_error("frame %d: all frames of a batch must be non-null and of equal size and channel count", i);
            return VJ_ERR_ARG;
        }
    *W_out = W;
    *H_out = H;
    *CH_out = CH;
    return VJ_OK;
}

// ---- the launch paths of one attempt.  Each ends on e->stream.
// Every scale on cv_profile_pass.  Four workgroups (16 waves) per CU: every wave walks its own window row, and the rows in flight on
// an XCD should stay inside its 4 MiB L2 (64 x 1080p: 376 / 235 / 179 / 153 / 173 / 194 / 193 ms for 1 / 2 / 3 / 4 / 5 / 6 / 8)
static int launch_cv_rows(const CvCall& cc, CvArgs& a) {
    const vj_env* e = cc.e;
    const CvPlan* pl = cc.pl;
    const int n_blocks = std::max(1, e->n_cu * 4);
    a.total_waves = (uint32_t)n_blocks * CV_WAVES_PER_BLOCK;
    return cascade_launched(launch_cv_profile_pass(a, pl->trees, cc.count, pl->is_tree, n_blocks, e->stream, pl->prune, pl->scale_image, cc.roc != nullptr));
}

// What the three tile paths share.  The small scales run on LDS tiles (vj_cv_tile.hip), the rest on cv_profile_pass, concurrently
// on two streams: the row kernel is bound by the texture-address unit, the tile kernel by LDS and VALU.  The row kernel is launched
// first, with one workgroup per CU, so that the tile workgroups find their LDS share next to it.
// begin: stream2 forked off e->stream (behind whatever the path has enqueued there: its bitmaps' memsets) and the rest rows on it
static int begin_cv_tiles(const CvCall& cc, const CvArgs& a, bool count, bool stage_tree, bool prune, bool exhaustive, bool* two) {
    vj_env* e = cc.e;
    const CvPlan* pl = cc.pl;
    *two = e->concurrent && pl->n_rows_rest != 0;
    if (*two) {
        HIP_TRY(hipEventRecord(e->fork_ev, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->stream2, e->fork_ev, 0));
    }
    if (pl->n_rows_rest == 0) return VJ_OK;
    CvArgs b = a;
    b.rows = (const UnitDev*)pl->d_rows_rest.p;
    b.n_rows = pl->n_rows_rest;
    const int nb = std::max(1, e->n_cu * (*two ? pl->row_blocks : 4));
    b.total_waves = (uint32_t)nb * CV_WAVES_PER_BLOCK;
    return cascade_launched(launch_cv_profile_pass(b, pl->trees, count, stage_tree, nb, *two ? e->stream2 : e->stream, prune, exhaustive));
}
// end: e->stream waits for the rest rows (also after a launch that failed)
static int end_cv_tiles(const CvCall& cc, bool two, int rc) {
    if (two) {
        HIP_TRY(hipEventRecord(cc.e->join_ev, cc.e->stream2));
        HIP_TRY(hipStreamWaitEvent(cc.e->stream, cc.e->join_ev, 0));
    }
    return rc;
}

// the tile kernel's arguments but for what differs between the paths: n_stages, the bitmap, the finish thresholds (ws_begin, ws_max),
// stage_entered, the tree queue
static CvTileArgs cv_tile_base_args(const CvArgs& a) {
    CvTileArgs t;
    memset(&t, 0, sizeof(t));
    t.sum = a.sum;
    t.tilted = a.tilted;
    t.sqsum = a.sqsum;
    t.table = a.table;
    t.scales = a.scales;
    t.stages = a.stages;
    t.n_frames = a.n_frames;
    t.frame_elems = a.frame_elems;
    t.stride = a.stride;
    t.sum_h = a.sum_h;
    t.repack_mask = ~3ull;        // before every stage from 2 on (as the clod profile's tiles)
    t.det = a.det;
    t.det_count = a.det_count;
    t.det_cap = a.det_cap;
    return t;
}

// cv_tile_pass<mode>: one launch per LDS class that has tiles; the classes' ticket counters from `first_slot` on (8 dwords each)
static int launch_cv_tile_classes(const CvCall& cc, const CvArgs& a, const CvTileArgs& t, int mode, bool count, bool tree2, int first_slot) {
    const vj_env* e = cc.e;
    const CvPlan* pl = cc.pl;
    uint32_t* tickets = a.det_count + 4;
    for (int cls = 0; cls < 2; ++cls) {
        const uint32_t n_cls = pl->class_first[cls + 1] - pl->class_first[cls];
        if (!n_cls) continue;
        CvTileArgs ta = t;
        ta.tiles = (const UnitDev*)pl->d_tiles.p + pl->class_first[cls];
        ta.n_tiles = n_cls;
        ta.lds_bytes = pl->class_lds[cls];
        ta.ticket = tickets + 8 * (first_slot + cls);
        const int per_cu = std::max(1, std::min(2, (int)((160u * 1024u - (uint32_t)pl->row_blocks * 20u * 1024u) / ta.lds_bytes)));
        const int tb = (int)std::min<uint64_t>((uint64_t)n_cls * (uint64_t)a.n_frames, (uint64_t)e->n_cu * (uint64_t)per_cu);
        if (const int rc = cascade_launched(launch_cv_tile_pass(ta, mode, count, tree2, std::max(1, tb), e->stream))) return rc;
    }
    return VJ_OK;
}

// reject bits -> visited bits, one recurrence domain per window row (skip_resolve)
static int launch_cv_skip_resolve(const CvCall& cc, uint32_t nf) {
    CascadeArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.skip_bits = (unsigned long long*)cc.e->d_skip_bits.p;
    ra.skip_frame_words = cc.pl->bits_frame_words;
    ra.skip_segs = (const UnitDev*)cc.pl->d_bit_segs.p;
    ra.n_skip_segs = cc.pl->n_bit_segs;
    ra.n_frames = nf;
    return cascade_launched(launch_skip_resolve(ra, std::max(1, cc.e->n_cu * 2), cc.e->stream));
}

// Linear cascades: cv_tile_pass<0> (reject bits of stage 0), skip_resolve, cv_tile_pass<1> (the cascade on the visited windows)
static int launch_cv_plain_tiles(const CvCall& cc, const CvArgs& a) {
    vj_env* e = cc.e;
    const CvPlan* pl = cc.pl;
    const int nf = (int)a.n_frames;
    const bool count = cc.count;
    int rc;
    if ((rc = e->d_skip_bits.ensure((size_t)pl->bits_frame_words * 8u * (size_t)nf))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_skip_bits.p, 0, (size_t)pl->bits_frame_words * 8u * (size_t)nf, e->stream));
    bool two;
    rc = begin_cv_tiles(cc, a, count, pl->is_tree, pl->prune, false, &two);
    CvTileArgs t = cv_tile_base_args(a);
    t.n_stages = pl->n_stages;
    t.bits = (unsigned long long*)e->d_skip_bits.p;
    t.bits_frame_words = pl->bits_frame_words;
    t.ws_begin = 3;
    t.ws_max = (uint32_t)e->cv_tile_ws_max;
    t.stage_entered = a.stage_entered;
    if (!rc) rc = launch_cv_tile_classes(cc, a, t, 0, count, pl->tree2, 0);
    if (!rc && pl->prune) {   // pruned windows are "zeros" of the walk (prune bitmap: cv_prune_mark)
        // one wave per window row of a tile scale: the rows' words are latency-bound gathers, thousands of waves hide them
        const CvPruneArgs pa = prune_args(e, pl, a, nf, nullptr);
        rc = cascade_launched(launch_cv_prune_mark(pa, (int)std::max<uint32_t>(1u, (pa.n_segs * pa.n_frames + 3u) / 4u), e->stream));
    }
    if (!rc) rc = launch_cv_skip_resolve(cc, a.n_frames);
    if (!rc && pl->prune) {   // ... visited but not evaluated: out of the visited bits, into counts.windows
        const CvPruneArgs pa = prune_args(e, pl, a, nf, count ? a.stage_entered + VJ_MAX_STAGES : nullptr);
        rc = cascade_launched(launch_cv_prune_visited(pa, std::max(1, e->n_cu * 2), e->stream));
    }
    if (!rc) rc = launch_cv_tile_classes(cc, a, t, 1, count, pl->tree2, 2);
    return end_cv_tiles(cc, two, rc);
}

// CV_HAAR_SCALE_IMAGE: the levels whose grid fills a tile on cv_tile_pass<3> — every grid window, no bitmap passes —, the small
// levels on the exhaustive-grid row kernel
static int launch_cv_scale_image_tiles(const CvCall& cc, const CvArgs& a) {
    const CvPlan* pl = cc.pl;
    bool two;
    int rc = begin_cv_tiles(cc, a, cc.count, false, false, true, &two);
    CvTileArgs t = cv_tile_base_args(a);
    t.n_stages = pl->n_stages;
    t.ws_begin = 3;
    t.ws_max = (uint32_t)cc.e->cv_tile_ws_max;
    t.stage_entered = a.stage_entered;
    if (!rc) rc = launch_cv_tile_classes(cc, a, t, 3, cc.count, pl->tree2, 0);
    return end_cv_tiles(cc, two, rc);
}

// Stage tree (uncounted calls): the tiles run the linear prefix on every grid window (cv_tile_pass<2>), cv_tree_walk or
// cv_tree_chain_pass the rest of the tree for the survivors, skip_resolve + cv_tree_emit the sequential walk.  cv_profile_pass keeps
// the large scales.  The survivors' queue has room for 1 / 2^shift of the tile windows; an overflow takes two off the shift and runs
// the attempt again, a forced capacity (tests) falls back to the rows instead (run_cv_subbatch).
// (the shift belongs to the PLAN: one survivor-heavy workload does not make every later call allocate more)
static int launch_cv_tree_tiles(CvCall& cc, CvAttempt* at) {
    vj_env* e = cc.e;
    CvPlan* pl = cc.pl;
    const CvArgs& a = at->a;
    const int nf = (int)a.n_frames;
    int rc;
    const size_t bits_bytes = (size_t)pl->bits_frame_words * 8u * (size_t)nf;
    if ((rc = e->d_skip_bits.ensure(bits_bytes))) return rc;
    if ((rc = e->d_cv_accept.ensure(bits_bytes))) return rc;
    if (pl->tq_shift < 0) pl->tq_shift = e->cv_tq_shift;
    const bool chain_pass = pl->chains.n != 0u && pl->n_tile_scales <= 64u && e->cv_tree_queue_cap <= 0 && e->cv_tree_chains;
    const CvTqSizing sz = cv_tq_sizing(pl->tile_windows, pl->n_tile_scales, (uint32_t)nf, (uint32_t)pl->tq_shift, e->cv_tree_queue_cap, chain_pass, cc.max_frames);
    if (sz.kind == CvTqSizing::ROWS_ONLY) {
        at->outcome = CvAttempt::ROWS_ONLY;
        return VJ_OK;
    }
    if (sz.kind == CvTqSizing::RESPLIT) {
        cc.max_frames = (int)sz.n;
        pl->tq_split_frames = cc.max_frames;
        at->outcome = CvAttempt::RESPLIT;
        return VJ_OK;
    }
    const uint32_t tq_cap = (uint32_t)sz.n;
    {   // never more than a quarter of what the device has free: beyond that the rows take the call
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)tq_cap * sizeof(CvTreeEntry) > e->d_cv_tq.cap &&
            (size_t)tq_cap * sizeof(CvTreeEntry) - e->d_cv_tq.cap > free_b / 4u) {
            at->outcome = CvAttempt::ROWS_ONLY;
            return VJ_OK;
        }
    }
    if ((rc = e->d_cv_tq.ensure((size_t)tq_cap * sizeof(CvTreeEntry)))) return rc;
    at->tq_cap = tq_cap;
    at->chain_pass = chain_pass;
    HIP_TRY(hipMemsetAsync(e->d_skip_bits.p, 0, bits_bytes, e->stream));
    HIP_TRY(hipMemsetAsync(e->d_cv_accept.p, 0, bits_bytes, e->stream));
    bool two;
    rc = begin_cv_tiles(cc, a, false, true, pl->prune, false, &two);
    uint32_t* tq_count = a.det_count + 4 + 32;
    CvTileArgs t = cv_tile_base_args(a);
    t.tq_shift = chain_pass ? (uint32_t)pl->tq_shift : 0xffffffffu;   // one sub-queue per scale, or one flat queue (cv_tree_walk)
    t.n_stages = pl->tree_prefix;        // the tiles stop after the prefix
    t.bits = (unsigned long long*)e->d_skip_bits.p;
    t.bits_frame_words = pl->bits_frame_words;
    t.ws_begin = 0xffffffffu;            // no finish: whoever survives the prefix leaves the tile
    t.ws_max = 0;
    t.tq = (CvTreeEntry*)e->d_cv_tq.p;
    t.tq_count = tq_count;
    t.tq_cap = tq_cap;
    if (!rc) rc = launch_cv_tile_classes(cc, a, t, 2, false, false, 0);
    CvTreeArgs w;
    memset(&w, 0, sizeof(w));
    w.sum = a.sum;
    w.table = a.table;
    w.scales = a.scales;
    w.stages = a.stages;
    w.n_order = pl->n_order;
    w.prefix = pl->tree_prefix;
    w.sum_bytes = (uint32_t)((uint64_t)a.frame_elems * 4u * (uint64_t)nf);
    w.tq = (const CvTreeEntry*)e->d_cv_tq.p;
    w.tq_count = tq_count;
    w.tq_cap = tq_cap;
    w.reject = (unsigned long long*)e->d_skip_bits.p;
    w.accept = (unsigned long long*)e->d_cv_accept.p;
    w.bits_frame_words = pl->bits_frame_words;
    w.n_frames = (uint32_t)nf;
    w.segs = (const UnitDev*)pl->d_bit_segs.p;
    w.n_segs = pl->n_bit_segs;
    w.det = a.det;
    w.det_count = a.det_count;
    w.det_cap = a.det_cap;
    if (chain_pass) {
        // the tree is made of chains: chunks of one scale's survivors, swept like a linear cascade (cv_chain_sweep)
        const int wb = std::max(1, e->n_cu * std::max(1, std::min(e->cv_tree_chain_blocks, 4)));
        w.tq_shift = (uint32_t)pl->tq_shift;
        w.n_scales = (uint32_t)pl->scales.size();
        w.ticket = tq_count + 64;
        w.chains = pl->chains;
        w.total_waves = (uint32_t)wb * 4u;
        w.chunk = (uint32_t)std::max(64, std::min(e->cv_tree_chunk, (int)CV_TQ_CHUNK));
        int erc;
        if ((erc = e->d_cv_fail_walk.ensure((size_t)w.total_waves * CV_TQ_CHUNK * sizeof(CvTreeEntry)))) return erc;
        w.fail_scratch = e->d_cv_fail_walk.p;
        if (!rc) rc = cascade_launched(launch_cv_tree_chain_pass(w, wb, e->stream));
    } else if (!rc) {
        rc = cascade_launched(launch_cv_tree_walk(w, std::max(1, e->n_cu * 4), e->stream));
    }
    if (!rc && pl->prune) {   // pruned windows: rejects of the walk, never accepted
        CvPruneArgs pa = prune_args(e, pl, a, nf, nullptr);
        pa.accept = (unsigned long long*)e->d_cv_accept.p;
        rc = cascade_launched(launch_cv_prune_mark(pa, (int)std::max<uint32_t>(1u, (pa.n_segs * pa.n_frames + 3u) / 4u), e->stream));
    }
    if (!rc) rc = launch_cv_skip_resolve(cc, a.n_frames);
    if (!rc) rc = cascade_launched(launch_cv_tree_emit(w, std::max(1, e->n_cu * 2), e->stream));
    return end_cv_tiles(cc, two, rc);
}

// One attempt at the sub-batch of nf frames whose integral images are on the device: the arguments, then the launches of the path
// the plan, the flags and `rows_only` choose, between lane0.ev[2] and ev[3], and the chain's hand-off behind them.
static int enqueue_cv_attempt(CvCall& cc, int nf, bool rows_only, CvAttempt* at) {
    vj_env* e = cc.e;
    CvPlan* pl = cc.pl;
    int rc;
    if ((rc = e->d_cv_det.ensure((size_t)cc.det_cap * (cc.roc ? sizeof(CvRocDet) : sizeof(CvDet))))) return rc;
    HIP_TRY(hipMemsetAsync(e->d_cv_counts.p, 0, CV_COUNTS_BYTES, e->stream));
    CvArgs& a = at->a;
    a = cv_base_args(e, facts_of(*pl), tables_of(pl), CvGeom{cc.frame_elems, cc.stride, (uint32_t)cc.IH + 1u, (uint32_t)nf}, e->d_cv_det.p, cc.det_cap,
                     e->d_cv_counts.p);
    a.rows = (const UnitDev*)pl->d_rows.p;
    a.n_rows = pl->n_rows;
    if (pl->prune) {
        a.edge_sum = (const uint32_t*)e->d_edge_sum.p;
        a.prune = (const CvPruneDev*)pl->d_prune.p;
    }
    if (pl->is_tree && pl->chains.n != 0u && !cc.count && e->cv_tree_chains) {   // the rows kernel sweeps the chains too (cv_chain_sweep): a fail list per wave
        a.chains = pl->chains;
        const size_t waves = (size_t)std::max(1, e->n_cu * 4) * CV_WAVES_PER_BLOCK;
        if ((rc = e->d_cv_fail_rows.ensure(waves * CV_QCAP * 16u))) return rc;
        a.fail_scratch = e->d_cv_fail_rows.p;
    }
    HIP_TRY(hipEventRecord(e->lane0.ev[2], e->stream));
    // (a stage tree's tile path leaves no per-stage counts of the visited windows: counted calls walk the rows)
    const bool tiles = pl->n_tile_scales != 0 && pl->class_first[2] != 0 && !(pl->is_tree && (cc.count || rows_only));
    if (tiles && pl->prune && (rc = e->d_cv_prune_bits.ensure((size_t)pl->bits_frame_words * 8u * (size_t)nf))) return rc;
    if (!tiles) rc = launch_cv_rows(cc, a);
    else if (pl->is_tree) rc = launch_cv_tree_tiles(cc, at);
    else if (pl->scale_image) rc = launch_cv_scale_image_tiles(cc, a);
    else rc = launch_cv_plain_tiles(cc, a);
    if (rc || at->outcome != CvAttempt::LAUNCHED) return rc;
    HIP_TRY(hipEventRecord(e->lane0.ev[3], e->stream));
    if (cc.dev && (rc = cc.dev->enqueue(nf, pl, a, cc.det_cap))) return rc;   // (stream2 has joined: every path above ends on e->stream)
    return VJ_OK;
}

// More prefix survivors than the tree queue (or one scale's sub-queue) holds?
static bool cv_tq_overflowed(const CvCall& cc, const CvAttempt& at, const std::vector<unsigned long long>& h) {
    if (at.tq_cap == 0u) return false;
    const uint32_t* tqc = (const uint32_t*)(h.data() + 2 * VJ_MAX_STAGES) + 4 + 32;
    if (!at.chain_pass) return tqc[0] > at.tq_cap;
    for (const CvScaleDev& sd : cc.pl->scales)
        if (sd.tile_th != 0u && (uint64_t)tqc[sd.tq_slot] > cv_tq_cap(sd.end_x, sd.end_y, at.a.n_frames, (uint32_t)cc.pl->tq_shift)) return true;
    return false;
}

// A detection record as the call's rectangle.  CV_HAAR_SCALE_IMAGE (every ROC call is one): Rect(cvRound(x * factor),
// cvRound(y * factor), winSize) (tempcv.cpp:1099-1100)
template <class Det> static vj_rect cv_rect_of(const CvScaleDev* scales, const double* level_factor /* null: not scale-image */, const Det& d, int f0) {
    const CvScaleDev& sd = scales[d.slot];
    const int32_t x = level_factor ? cv_round((double)d.x * level_factor[d.slot]) : (int32_t)d.x;
    const int32_t y = level_factor ? cv_round((double)d.y * level_factor[d.slot]) : (int32_t)d.y;
    return vj_rect{x, y, (int32_t)sd.win_w, (int32_t)sd.win_h, 0.0f, f0 + (int32_t)d.frame, (int32_t)sd.scale_idx};
}

// The sub-batch [f0, f0 + nf): its integral images, then attempts until the detections, the tree queue and the hand-off's buffers
// all held what came; its candidates appended to cc.all, raw.  *resplit: nothing ran — the same frames again, cc.max_frames at a time.
static int run_cv_subbatch(CvCall& cc, int f0, int nf, bool* resplit) {
    vj_env* e = cc.e;
    CvPlan* pl = cc.pl;
    CvChainDevice* dev = cc.dev;
    vj_result* out = cc.out;
    int rc;
    *resplit = false;
    if ((rc = enqueue_cv_ingest(e, cc.frames + f0, nf, cc.W, cc.H, cc.CH, cc.equalize, pl, pl->has_tilted || cc.need_tilted))) return rc;
    bool rows_only = false, done = false;
    const size_t sub_first = cc.all.size();
    std::vector<unsigned long long> h;
    // (the device hand-off may grow three buffers in turn — this cascade's detections, the units, the second cascade's detections)
    for (int attempt = 0; attempt < (dev ? 5 : 2) && !done; ++attempt) {
        CvAttempt at;
        if ((rc = enqueue_cv_attempt(cc, nf, rows_only, &at))) return rc;
        if (at.outcome == CvAttempt::RESPLIT) {
            *resplit = true;
            return VJ_OK;
        }
        uint32_t n_det = 0;
        if (at.outcome == CvAttempt::LAUNCHED && (rc = read_cv_counts(e, CV_COUNTS_BYTES, &h, &n_det))) return rc;
        if (at.outcome == CvAttempt::ROWS_ONLY || cv_tq_overflowed(cc, at, h)) {   // (neither consumes an attempt)
            if (at.outcome == CvAttempt::ROWS_ONLY || e->cv_tree_queue_cap > 0 || pl->tq_shift <= 0) rows_only = true;
            else pl->tq_shift = std::max(0, pl->tq_shift - 2);      // 1/16 -> 1/4 -> every window, for THIS plan
            --attempt;
            continue;
        }
        if (n_det > cc.det_cap) {   // overflow: grow and redo this sub-batch's cascade
            cc.det_cap = grown_cap(cc.det_cap, n_det);
            if (dev) e->cv_chain_info.reruns += 1;
            continue;
        }
        if (dev) {
            bool again = false;
            if ((rc = dev->check(&again))) return rc;
            if (again) continue;
        }
        float ms_i = 0, ms_c = 0, ms_t = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_c, e->lane0.ev[2], e->lane0.ev[3]));
        HIP_TRY(hipEventElapsedTime(&ms_t, e->lane0.ev[0], e->lane0.ev[3]));
        out->timing.integral_ms += ms_i;
        out->timing.cascade_ms += ms_c;
        out->timing.total_ms += ms_t;
        out->timing.n_cascade_launches = 1;
        if (cc.count) add_cv_counters(h, pl->n_stages, &out->counters);
        done = true;
        const CvScaleDev* scales = pl->scales.data();
        const double* level_factor = pl->scale_image ? pl->level_factor.data() : nullptr;
        if (cc.roc) {
            std::vector<CvRocDet> raw;
            if ((rc = read_cv_dets(e, n_det, &raw))) return rc;
            for (const CvRocDet& d : raw) {
                cc.all.push_back(cv_rect_of(scales, level_factor, d, f0));
                cc.all_levels.push_back((int32_t)d.level);
                cc.all_weights.push_back(d.weight);
            }
        } else if (!(dev && dev->grouped && !dev->fallback)) {   // (else the grouped rectangles are read back instead: CvChainDevice::finish)
            std::vector<CvDet> raw;
            if ((rc = read_cv_dets(e, n_det, &raw))) return rc;
            for (const CvDet& d : raw) cc.all.push_back(cv_rect_of(scales, level_factor, d, f0));
        }
    }
    if (!done) {   // (cannot happen: the counts of a repeated pass are the counts that sized its buffers)
        set_error("vj_detect_opencv: the detection buffer overflowed twice");
        return VJ_ERR_LIMIT;
    }
    if (dev) return dev->finish(f0, nf, cc.all.data() + sub_first, cc.all.size() - sub_first, sub_first);
    if (cc.hook) return (*cc.hook)(f0, nf, cc.all.data() + sub_first, cc.all.size() - sub_first);
    return VJ_OK;
}

// The call's candidates as its result: in order, grouped, the counters' totals
static int collect_cv_result(CvCall& cc) {
    std::vector<vj_rect>& all = cc.all;
    const CvRocCall* roc = cc.roc;
    // the device grouped every frame (or, where it could not, the host hook did): the regions of all sub-batches ARE the result
    const bool pre_grouped = cc.dev && cc.dev->grouped;
    if (pre_grouped) all = *cc.dev->regions;
    if (roc) {   // the key is unique (one report per grid position of a level): levels and weights follow their rectangles
        std::vector<size_t> idx(all.size());
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
        std::sort(idx.begin(), idx.end(), [&](size_t i, size_t j) { return cv_rect_before(all[i], all[j]); });
        std::vector<vj_rect> sorted(all.size());
        roc->levels->resize(all.size());
        roc->weights->resize(all.size());
        for (size_t i = 0; i < idx.size(); ++i) {
            sorted[i] = all[idx[i]];
            (*roc->levels)[i] = cc.all_levels[idx[i]];
            (*roc->weights)[i] = cc.all_weights[idx[i]];
        }
        all.swap(sorted);
    } else if (!pre_grouped) {
        std::sort(all.begin(), all.end(), cv_rect_before);
    }
    const int rc = cv_result_epilogue(all, cc.count ? &cc.pl->prog : nullptr, cc.out);
    if (rc) return rc;
    // groupRectangles(rectList, max(minNeighbors, 1), GROUP_EPS)
    if (!roc && !pre_grouped && cc.p->min_neighbors != 0 && cc.out->count)
        return vj_group_rectangles(cc.out->rects, &cc.out->count, (int)std::max<uint32_t>(cc.p->min_neighbors, 1u), 0.2);
    return VJ_OK;
}

// vj_detect_opencv.  need_tilted: compute the tilted integral even when `c` has no tilted feature (someone after it reads it).
// roc: vj_detect_opencv_roc's scale-image call — the kernels report CvRocDet records; the rectangles come back raw (ungrouped),
// sorted, with their levels and weights in roc's vectors.
int detect_opencv_impl(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_cv_params* p, vj_result* out,
                       bool need_tilted, const CvSubBatchHook* hook, const CvRocCall* roc = nullptr, CvChainDevice* dev = nullptr) {
    if (!e || !c || !p || !out || n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (n_frames == 0) return VJ_OK;
    CvCall cc{};
    int rc = check_cv_call(frames, n_frames, p, &cc.W, &cc.H, &cc.CH);
    if (rc) return rc;
    // VJ_FLAG_EQUALIZE_HIST is read here and nowhere else: the plan, its key and the kernels see the parameters without it
    vj_cv_params p_plain = *p;
    p_plain.flags &= ~(uint32_t)VJ_FLAG_EQUALIZE_HIST;
    cc.e = e;
    cc.frames = frames;
    cc.p = &p_plain;
    cc.out = out;
    cc.equalize = (p->flags & VJ_FLAG_EQUALIZE_HIST) != 0u;
    cc.need_tilted = need_tilted;
    cc.count = (p->flags & VJ_FLAG_COUNTERS) != 0;
    cc.hook = hook;
    cc.roc = roc;
    cc.dev = dev;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = get_cv_plan(e, c, cc.W, cc.H, cc.p, n_frames, &cc.pl, roc))) return rc;
    const CvPlan* pl = cc.pl;
    if (pl->find_biggest) return detect_biggest(e, c, cc.pl, frames, n_frames, cc.W, cc.H, cc.CH, cc.p, cc.equalize, out);
    // CV_HAAR_SCALE_IMAGE: the integral images are those of the canvas that holds the pyramid's levels
    const int IW = pl->scale_image ? (int)pl->canvas_w : cc.W;
    cc.IH = pl->scale_image ? (int)pl->canvas_h : cc.H;
    cc.stride = (uint32_t)IW + 1u;
    cc.frame_elems = frame_elems_for(IW, cc.IH);
    if ((rc = e->d_cv_counts.ensure(CV_COUNTS_BYTES))) return rc;
    cc.max_frames = cv_max_frames(e, n_frames, cc.frame_elems);
    {   // the detection counter is 32-bit: a sub-batch holds fewer than 2^32 windows, so it cannot wrap
        uint64_t frame_windows = 0;
        for (const CvScaleDev& sd : pl->scales) frame_windows += (uint64_t)sd.end_x * sd.end_y;
        if (frame_windows > 0xffffffffull) {
            set_error("vj_detect_opencv: %llu windows per frame, more than a 32-bit detection count holds",
                      (unsigned long long)frame_windows);
            return VJ_ERR_LIMIT;
        }
        if (frame_windows) cc.max_frames = (int)std::min<uint64_t>((uint64_t)cc.max_frames, 0xffffffffull / frame_windows);
    }
    // (a ROC call reports several times as many windows: its buffer starts at the configured "det_cap" and grows the same way)
    // (the chain's device hand-off too: its buffers all start at "det_cap", so that a small value drives every regrow path)
    cc.det_cap = roc || dev ? std::max(1u, e->det_cap_init) : 1u << 16;
    for (int f0 = 0, nf = 0; f0 < n_frames && pl->n_rows != 0; f0 += nf) {
        nf = std::min(cc.max_frames, n_frames - f0);
        bool resplit = false;
        if ((rc = run_cv_subbatch(cc, f0, nf, &resplit))) return rc;
        if (resplit) nf = 0;   // the same frames again, in sub-batches of cc.max_frames
    }
    return collect_cv_result(cc);
}

// ------------------------------------------------------------------------ a cascade inside regions
// (what needs no device — argument checks, factors, the unit list, grouping by size, result shaping — is vj_cv_roi_host.cpp)

// The region pass's tables for (cascade, frame width, scale factor) with at least n_factors factors.  cvSetImagesForHaarClassifierCascade
// (tempcv.cpp:549-768) reads the image only through its row step — equRect, the rectangles and the weights come from the factor and the
// window alone — so a factor's records serve every region of every frame of this width.
int get_cv_roi_plan(vj_env* e, const vj_cascade* c, int W, const vj_cv_params* p, int n_factors, CvRoiPlan** out) {
    uint64_t sf_bits;
    memcpy(&sf_bits, &p->scale_factor, 8);
    const vj_env::CvRoiPlanKey key(c->uid, W, sf_bits);
    auto it = e->cv_roi_plans.find(key);
    CvRoiPlan* pl = it != e->cv_roi_plans.end() ? it->second.get() : nullptr;
    if (pl && (int)pl->factors.size() >= n_factors) {
        pl->last_used = ++e->plan_tick;
        *out = pl;
        return VJ_OK;
    }
    CvCascadeHost ch;   // (a plan that only grows was built from this cascade before)
    if (!pl)
        if (const int crc = cv_cascade_host(c, &ch)) return crc;
    const size_t n_nodes = c->nodes.size();
    if ((uint64_t)n_factors * n_nodes > (1ull << 26)) {
        set_error("scale_factor %.17g gives %d factors: the node tables would exceed 4 GiB", p->scale_factor, n_factors);
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));   // (tables are released below)
    std::unique_ptr<CvRoiPlan> fresh;
    if (!pl) {
        cache_make_room(e, e->cv_roi_plans);
        fresh = std::make_unique<CvRoiPlan>();
        pl = fresh.get();
        pl->prog = ch.prog;
        pl->trees = ch.shape.trees;
        pl->is_tree = ch.shape.is_tree;
        pl->has_tilted = ch.shape.has_tilted;
        pl->tree2 = ch.shape.tree2;
        pl->n_order = (uint32_t)ch.order.size();
        pl->n_stages = (uint32_t)c->stages.size();
        int rc = pl->d_stages.ensure(ch.stages.size() * sizeof(StageDev));
        if (!rc && hipMemcpy(pl->d_stages.p, ch.stages.data(), ch.stages.size() * sizeof(StageDev), hipMemcpyHostToDevice) != hipSuccess) {
            set_error("uploading the stage records failed");
            rc = VJ_ERR_HIP;
        }
        if (rc) {
            pl->release_device();
            return rc;
        }
    }
    // every factor again (the table is one allocation): the doubles of the enumeration, factor *= scale_factor
    const uint32_t stride = (uint32_t)W + 1u;
    std::vector<CvScaleDev> scales((size_t)n_factors);
    std::vector<CvRoiFactor> factors((size_t)n_factors);
    std::vector<double> factor_values((size_t)n_factors);
    std::vector<CvNodeRec> table((size_t)n_factors * n_nodes);
    double factor = 1;
    int rc = VJ_OK;
    for (int k = 0; k < n_factors && !rc; ++k, factor *= p->scale_factor) {
        factor_values[(size_t)k] = factor;
        CvScaleDev& sd = scales[(size_t)k];
        memset(&sd, 0, sizeof(sd));
        CvRoiFactor& f = factors[(size_t)k];
        f = cv_roi_factor(c->win_w, c->win_h, factor);
        sd.ystep = f.ystep;
        const CvEquRect q = cv_equ_rect(c->win_w, c->win_h, factor);
        cv_set_equ_rect(&sd, q, stride);
        sd.win_w = (uint32_t)f.win_w;
        sd.win_h = (uint32_t)f.win_h;
        sd.table_first = (uint32_t)((size_t)k * n_nodes);
        sd.scale_idx = (uint32_t)k;
        rc = build_cv_node_recs(c, factor, stride, q.inv_area, table.data() + sd.table_first, &f.max_reach);
    }
    if (!rc) rc = pl->d_table.ensure(std::max<size_t>(table.size(), 1) * sizeof(CvNodeRec));
    if (!rc) rc = pl->d_scales.ensure(std::max<size_t>(scales.size(), 1) * sizeof(CvScaleDev));
    if (!rc && !table.empty() &&
        (hipMemcpy(pl->d_table.p, table.data(), table.size() * sizeof(CvNodeRec), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(pl->d_scales.p, scales.data(), scales.size() * sizeof(CvScaleDev), hipMemcpyHostToDevice) != hipSuccess)) {
        set_error("uploading the region pass's tables failed");
        rc = VJ_ERR_HIP;
    }
    if (rc) {   // (a plan that failed to grow is dropped: its tables may be gone)
        pl->release_device();
        if (!fresh) e->cv_roi_plans.erase(key);
        return rc;
    }
    pl->factors = std::move(factors);
    pl->factor_values = std::move(factor_values);
    pl->chain_factors_n = 0;
    pl->last_used = ++e->plan_tick;
    if (fresh) e->cv_roi_plans[key] = std::move(fresh);
    *out = pl;
    return VJ_OK;
}

// `second` inside `regs`, regions of the nf frames whose integral images (W x H; sum, sqsum, the tilted integral when the cascade
// has tilted nodes) are on the device: one launch of cv_roi_pass for all of them.  Appends the raw candidates (rect.frame = the
// region's id, x / y relative to the region) to *all, adds counters and times to *out.  *plan_out: the tables used (prog, n_stages).
int run_cv_roi_pass(vj_env* e, const vj_cascade* c, int W, int H, int nf, const std::vector<CvRoiHost>& regs, const vj_cv_params* p,
                    std::vector<vj_rect>* all, vj_result* out, CvRoiPlan** plan_out, uint64_t* units_out = nullptr, uint64_t* windows_out = nullptr) {
    const int cap = (int)((1ull << 26) / std::max<size_t>(c->nodes.size(), 1));   // (what get_cv_roi_plan's tables may hold)
    // the tables are sized once for the frame's own last factor: no region inside it takes more, so a plan grows only when a
    // taller frame of the same width comes, never in the middle of a batch
    const int n_factors = cv_count_factors(c->win_w, c->win_h, W, H, p->scale_factor, cap);
    if (n_factors == 0) return VJ_OK;   // the frame, so every region, is too small for any scale
    CvRoiPlan* pl;
    int rc = get_cv_roi_plan(e, c, W, p, n_factors, &pl);
    if (rc) return rc;
    *plan_out = pl;
    const uint32_t stride = (uint32_t)W + 1u;
    const uint32_t frame_elems = frame_elems_for(W, H);
    const bool count = (p->flags & VJ_FLAG_COUNTERS) != 0;
    std::vector<CvRoiDev> rois;
    std::vector<CvRoiUnit> units;
    uint64_t windows = 0;
    if ((rc = cv_roi_build_units(regs, c->win_w, c->win_h, p->scale_factor, pl->factors, stride, frame_elems, p->min_w, p->min_h, &rois, &units,
                                 &windows)))
        return rc;
    if (units_out) *units_out = units.size();
    if (windows_out) *windows_out = windows;
    if (units.empty()) return VJ_OK;
    if ((rc = e->d_cv_rois.ensure(rois.size() * sizeof(CvRoiDev)))) return rc;
    if ((rc = e->d_cv_roi_units.ensure(units.size() * sizeof(CvRoiUnit)))) return rc;
    HIP_TRY(hipMemcpy(e->d_cv_rois.p, rois.data(), rois.size() * sizeof(CvRoiDev), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_cv_roi_units.p, units.data(), units.size() * sizeof(CvRoiUnit), hipMemcpyHostToDevice));
    DevBuf& d_det = e->d_cv_det;
    DevBuf& d_counts = e->d_cv_counts;
    const size_t counts_bytes = 2 * VJ_MAX_STAGES * sizeof(uint64_t) + 16;   // stage_entered | visited ... | detection count
    if ((rc = d_counts.ensure(counts_bytes))) return rc;
    uint32_t det_cap = 1u << 16;
    std::vector<unsigned long long> h;
    uint32_t n_det = 0;
    rc = run_cv_pass_until_fit(e, counts_bytes, &det_cap, "vj_detect_opencv_rois: the detection buffer overflowed twice", [&](uint32_t cap) {
        CvRoiArgs ra;
        memset(&ra, 0, sizeof(ra));
        CvArgs& a = ra.cv;
        a = cv_base_args(e, facts_of(*pl), tables_of(pl), CvGeom{frame_elems, stride, (uint32_t)H + 1u, (uint32_t)nf}, d_det.p, cap, d_counts.p);
        ra.rois = (const CvRoiDev*)e->d_cv_rois.p;
        ra.units = (const CvRoiUnit*)e->d_cv_roi_units.p;
        ra.n_units = (uint32_t)units.size();
        // one wave per unit, at most four workgroups (16 waves) per CU; the rest by stride
        const int n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((units.size() + CV_WAVES_PER_BLOCK - 1) / CV_WAVES_PER_BLOCK, (uint64_t)std::max(1, e->n_cu * 4)));
        a.total_waves = (uint32_t)n_blocks * CV_WAVES_PER_BLOCK;
        return cascade_launched(launch_cv_roi_pass(ra, pl->trees, count, pl->is_tree, n_blocks, e->stream));
    }, &h, &n_det);
    if (rc) return rc;
    float ms_c = 0;
    HIP_TRY(hipEventElapsedTime(&ms_c, e->lane0.ev[2], e->lane0.ev[3]));
    out->timing.cascade_ms += ms_c;
    out->timing.total_ms += ms_c;
    out->timing.n_cascade_launches += 1;
    if (count) add_cv_counters(h, pl->n_stages, &out->counters);
    std::vector<CvDet> raw;
    if ((rc = read_cv_dets(e, n_det, &raw))) return rc;
    return cv_roi_rects_of(raw.data(), raw.size(), pl->factors, regs, all);
}

// ------------------------------------------------------------------------ the chain's device hand-off
// (what needs no device — the route, the index remap, the info record, the state block's errors — is vj_cv_roi_host.cpp)

// Before the first cascade runs: the second cascade's tables for the frame, and its factor slots as the device's unit builder reads
// them.  rp stays null when the frame is too small for any scale of the second cascade (the caller takes the host route).
int CvChainDevice::begin() {
    const int cap = (int)((1ull << 26) / std::max<size_t>(second->nodes.size(), 1));
    const int n_factors = cv_count_factors(second->win_w, second->win_h, W, H, p_second->scale_factor, cap);
    if (n_factors == 0) return VJ_OK;
    int rc = get_cv_roi_plan(e, second, W, p_second, n_factors, &rp);
    if (rc) return rc;
    if (rp->chain_factors_n != (uint32_t)rp->factors.size()) {
        std::vector<CvChainFactor> t(rp->factors.size());
        for (size_t k = 0; k < t.size(); ++k)
            t[k] = CvChainFactor{rp->factor_values[k], rp->factors[k].ystep, rp->factors[k].win_w, rp->factors[k].win_h, rp->factors[k].max_reach};
        if ((rc = rp->d_chain_factors.ensure(t.size() * sizeof(CvChainFactor)))) return rc;
        HIP_TRY(hipMemcpy(rp->d_chain_factors.p, t.data(), t.size() * sizeof(CvChainFactor), hipMemcpyHostToDevice));
        rp->chain_factors_n = (uint32_t)t.size();
    }
    unit_cap = (uint32_t)std::min<uint64_t>(4ull * std::max(1u, e->det_cap_init), 0x7fffffffull);
    det2_cap = std::max(1u, e->det_cap_init);
    return VJ_OK;
}

int CvChainDevice::enqueue(int nf, const CvPlan* pl, const CvArgs& a, uint32_t det_cap) {
    int rc;
    fallback = false;
    const size_t counts2_bytes = 2 * VJ_MAX_STAGES * sizeof(uint64_t) + 16;   // stage_entered | visited ... | detection count
    // frame_count | frame_cursor | grouped_count | frame_first [nf + 1] | the state block (8-byte aligned)
    const size_t state_at = ((size_t)(4 * nf + 1) * sizeof(uint32_t) + 7u) & ~(size_t)7u;
    const size_t small_bytes = state_at + sizeof(CvChainState);
    if ((rc = e->d_cv_chain.ensure(small_bytes))) return rc;
    if (grouped && (rc = e->d_cv_chain_keys.ensure((size_t)det_cap * sizeof(uint64_t)))) return rc;
    if (grouped && (rc = e->d_cv_chain_staged.ensure((size_t)det_cap * sizeof(CvRoiDev)))) return rc;
    if ((rc = e->d_cv_rois.ensure((size_t)det_cap * sizeof(CvRoiDev)))) return rc;
    if ((rc = e->d_cv_roi_first.ensure((size_t)det_cap * 2u * sizeof(uint32_t)))) return rc;
    if ((rc = e->d_cv_roi_units.ensure((size_t)unit_cap * sizeof(CvRoiUnit)))) return rc;
    if ((rc = e->d_cv_det2.ensure((size_t)det2_cap * sizeof(CvDet)))) return rc;
    if ((rc = e->d_cv_counts2.ensure(counts2_bytes))) return rc;
    h_counts2.assign((counts2_bytes + 7) / 8, 0ull);
    const uint32_t stride = (uint32_t)W + 1u;
    const uint32_t frame_elems = frame_elems_for(W, H);
    CvChainArgs g;
    memset(&g, 0, sizeof(g));
    g.det = a.det;
    g.det_count = a.det_count;
    g.det_cap = det_cap;
    g.scales = (const CvScaleDev*)pl->d_scales.p;
    g.n_scales = (uint32_t)pl->scales.size();
    g.n_frames = (uint32_t)nf;
    g.width = (uint32_t)W;
    g.height = (uint32_t)H;
    g.stride = stride;
    g.frame_elems = frame_elems;
    g.grouped = grouped ? 1u : 0u;
    g.threshold = threshold;
    g.group_max = (uint32_t)std::max(1, e->group_max);
    g.eps = 0.2;
    g.frame_count = (uint32_t*)e->d_cv_chain.p;
    g.frame_cursor = g.frame_count + nf;
    g.grouped_count = g.frame_cursor + nf;
    g.frame_first = g.grouped_count + nf;
    g.keys = (uint64_t*)e->d_cv_chain_keys.p;
    g.staged = (CvRoiDev*)e->d_cv_chain_staged.p;
    g.rois = (CvRoiDev*)e->d_cv_rois.p;
    g.factors = (const CvChainFactor*)rp->d_chain_factors.p;
    g.n_factors = rp->chain_factors_n;
    g.scale_factor = p_second->scale_factor;
    g.win_w = second->win_w;
    g.win_h = second->win_h;
    g.min_w = p_second->min_w;
    g.min_h = p_second->min_h;
    g.roi_units = (uint32_t*)e->d_cv_roi_first.p;
    g.roi_first = g.roi_units + det_cap;
    g.units = (CvRoiUnit*)e->d_cv_roi_units.p;
    g.unit_cap = unit_cap;
    g.state = (CvChainState*)((char*)e->d_cv_chain.p + state_at);
    HIP_TRY(hipEventRecord(e->cv_chain_ev[0], e->stream));
    HIP_TRY(hipMemsetAsync(e->d_cv_chain.p, 0, small_bytes, e->stream));
    int hrc = launch_cv_chain_handoff(g, e->n_cu, e->stream);
    if (hrc) {
        set_error("hand-off launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    HIP_TRY(hipEventRecord(e->cv_chain_ev[1], e->stream));
    // the region pass as run_cv_roi_pass launches it, on the units the kernels above left: their count comes from the state block
    HIP_TRY(hipMemsetAsync(e->d_cv_counts2.p, 0, counts2_bytes, e->stream));
    CvRoiArgs ra;
    memset(&ra, 0, sizeof(ra));
    CvArgs& b = ra.cv;
    b = cv_base_args(e, facts_of(*rp), tables_of(rp), CvGeom{frame_elems, stride, (uint32_t)H + 1u, (uint32_t)nf}, e->d_cv_det2.p, det2_cap, e->d_cv_counts2.p);
    ra.rois = (const CvRoiDev*)e->d_cv_rois.p;
    ra.units = (const CvRoiUnit*)e->d_cv_roi_units.p;
    ra.n_units_dev = &g.state->n_units_run;
    // (the host does not know the unit count: the full four workgroups per CU; the units go round by stride)
    const int n_blocks = std::max(1, e->n_cu * 4);
    b.total_waves = (uint32_t)n_blocks * CV_WAVES_PER_BLOCK;
    if (const int rc2 = cascade_launched(launch_cv_roi_pass(ra, rp->trees, (p_second->flags & VJ_FLAG_COUNTERS) != 0, rp->is_tree, n_blocks, e->stream))) return rc2;
    HIP_TRY(hipEventRecord(e->cv_chain_ev[2], e->stream));
    HIP_TRY(hipMemcpyAsync(&h_state, g.state, sizeof(CvChainState), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(h_counts2.data(), e->d_cv_counts2.p, counts2_bytes, hipMemcpyDeviceToHost, e->stream));
    return VJ_OK;
}

// After the synchronisation, when the first cascade's detections fitted
int CvChainDevice::check(bool* again) {
    *again = false;
    if (h_state.overflow != 0u) {   // a frame with more candidates than the device groups: this sub-batch through the host
        fallback = true;
        return VJ_OK;
    }
    const int rc = cv_chain_state_error(h_state);
    if (rc) return rc;
    const uint32_t n_det2 = (uint32_t)(h_counts2[2 * VJ_MAX_STAGES] & 0xffffffffull);
    if (h_state.n_units > (uint64_t)unit_cap) unit_cap = grown_cap(unit_cap, h_state.n_units);   // (the count pass's total is exact)
    else if (n_det2 > det2_cap) det2_cap = grown_cap(det2_cap, n_det2);
    else return VJ_OK;
    e->cv_chain_info.reruns += 1;
    *again = true;
    return VJ_OK;
}

// The sub-batch stands.  raw: the first cascade's candidates of the sub-batch as the loop appended them (not there when the device
// grouped them); base: their place in the call's list.
int CvChainDevice::finish(int f0, int nf, const vj_rect* raw, size_t n_raw, size_t base) {
    if (fallback) return (*host_hook)(f0, nf, raw, n_raw);
    float ms_h = 0, ms_c = 0;
    HIP_TRY(hipEventElapsedTime(&ms_h, e->cv_chain_ev[0], e->cv_chain_ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_c, e->cv_chain_ev[1], e->cv_chain_ev[2]));
    e->cv_chain_info.handoff_ms += ms_h;
    if (h_state.n_units_run != 0u) {
        out_second->timing.cascade_ms += ms_c;
        out_second->timing.total_ms += ms_c;
        out_second->timing.n_cascade_launches += 1;
    }
    if ((p_second->flags & VJ_FLAG_COUNTERS) != 0) {
        for (size_t s = 0; s < rp->n_stages; ++s) out_second->counters.stage_entered[s] += h_counts2[s];
        out_second->counters.windows += h_counts2[VJ_MAX_STAGES];
    }
    const uint32_t n_regions = h_state.n_regions, n_det2 = (uint32_t)(h_counts2[2 * VJ_MAX_STAGES] & 0xffffffffull);
    std::vector<CvRoiDev> rois(n_regions);
    if (n_regions) HIP_TRY(hipMemcpy(rois.data(), e->d_cv_rois.p, (size_t)n_regions * sizeof(CvRoiDev), hipMemcpyDeviceToHost));
    std::vector<CvDet> det2(n_det2);
    if (n_det2) HIP_TRY(hipMemcpy(det2.data(), e->d_cv_det2.p, (size_t)n_det2 * sizeof(CvDet), hipMemcpyDeviceToHost));
    std::vector<int> ids;
    int rc = grouped ? cv_chain_grouped_regions(rois.data(), rois.size(), f0, nf, regions, &ids)
                     : cv_chain_region_ids(rois.data(), rois.size(), raw, n_raw, f0, base, &ids);
    if (rc) return rc;
    if ((rc = cv_chain_rects_of(det2.data(), det2.size(), rp->factors, ids, all2))) return rc;
    cv_chain_info_add(&e->cv_chain_info, true, n_regions, h_state.n_units, h_state.windows);
    return VJ_OK;
}

// ------------------------------------------------------------------------ a cascade on a caller's windows
// vj_run_windows_opencv: what the shared driver (vj_points_driver.hpp) needs of this profile (device-free: vj_cv_points_host.cpp)
struct CvPoints {
    static constexpr const char* name = "vj_run_windows_opencv";
    typedef CvPointScale Geom;
    typedef CvPointScaleDev ScaleDev;
    typedef CvPointResult Result;
    typedef CvPointArgs Args;
    static constexpr int waves = CV_WAVES_PER_BLOCK;
    static constexpr auto scatter = cv_points_scatter;
    static int check(const vj_cascade* c, const vj_image* frames, int n_frames, const double* scales, int n_scales, const vj_window* windows,
                     uint32_t n_windows, int start_stage, uint32_t, const vj_window_result* out, int* W, int* H, int* CH) {
        return cv_points_check(c, frames, n_frames, scales, n_scales, windows, n_windows, start_stage, out, W, H, CH);
    }
    static auto& cascades(vj_env* e) { return e->cv_point_cascades; }
    static auto& plans(vj_env* e) { return e->cv_point_plans; }
    static vj_env::CvPointPlanKey plan_key(const vj_cascade* c, int W, double scale, uint32_t) {
        uint64_t bits;
        memcpy(&bits, &scale, 8);
        return vj_env::CvPointPlanKey(c->uid, W, bits);
    }
    // the stage records vj_detect_opencv's plans hold
    static void build_stages(const vj_cascade* c, const StageProgram& prog, const std::vector<uint32_t>& order, PointCascade* pc,
                             std::vector<StageDev>* stages) {
        const CvShape shape = cv_shape_of(c);
        pc->trees = shape.trees;
        pc->is_tree = shape.is_tree;
        pc->has_tilted = shape.has_tilted;
        pc->tree2 = shape.tree2;
        *stages = build_cv_stage_recs(c, prog, order, shape.two_rects, shape.trees, shape.is_tree);
    }
    static int geometry(const vj_cascade* c, double scale, int W, int H, CvPointScale* g) {
        *g = cv_point_scale(c->win_w, c->win_h, scale, W, H);
        return VJ_OK;
    }
    // cvSetImagesForHaarClassifierCascade (tempcv.cpp:549-768) reads the image only through its row step
    static int build_scale(const vj_cascade* c, double scale, int W, const CvPointScale& sc, CvPointScaleDev* rec, CvNodeRec* table,
                           uint64_t* max_reach) {
        const uint32_t stride = (uint32_t)W + 1u;
        cv_set_equ_rect(rec, CvEquRect{sc.ex, sc.ew, sc.eh, sc.weight_scale}, stride);   // (cv_point_scale's equRect: clamped so that no scale overflows an int)
        *max_reach = rec->q3;
        return build_cv_node_recs(c, scale, stride, sc.weight_scale, table, max_reach);
    }
    static int extra_images(vj_env* e, const PointCascade& pc, const uint8_t* d_gray, size_t gray_frame_bytes, int gray_stride, int W, int H,
                            int nf, int CH) {
        return pc.has_tilted ? enqueue_tilted(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, CH) : VJ_OK;
    }
    static void fill_args(const vj_env* e, const PointCascade& pc, uint32_t, CvPointArgs* a) {
        fill_shape_args(e, facts_of(pc), a);
    }
    static int launch(const CvPointArgs& a, const PointCascade& pc, int n_blocks, void* stream) {
        return launch_cv_points_pass(a, pc.trees, pc.is_tree, n_blocks, stream);
    }
};

const uint32_t CV_ROI_FAST_FLAGS = VJ_FLAG_COUNTERS;   // a flag word within these takes the region pass

// ------------------------------------------------------------------------ CV_HAAR_SCALE_IMAGE inside regions
// A flag word with VJ_FLAG_CV_SCALE_IMAGE and within these takes the level canvases (canny pruning and rough search are not read
// by the scale-image branch; VJ_FLAG_CV_FIND_BIGGEST clears scale-image and is not among them)
const uint32_t CV_ROI_LEVEL_FLAGS = VJ_FLAG_COUNTERS | VJ_FLAG_CV_SCALE_IMAGE | VJ_FLAG_CV_CANNY_PRUNING | VJ_FLAG_CV_ROUGH_SEARCH | VJ_FLAG_CV_CHAIN_DEVICE;
// Pixels of a canvas of level images: 64 MiB of sum image, 128 MiB of square sums (and 64 MiB of tilted integral); far below the
// (w + 1) * (h + 3) < 2^30 of a frame's 32-bit offsets
const uint64_t CV_ROI_CANVAS_PX = 1ull << 24;

// vj_detect_opencv_rois with VJ_FLAG_CV_SCALE_IMAGE on uniform frames: per canvas ONE pyramid launch for every level image of its
// regions (pyramid_regions), the integral kernels on the canvas as on a frame, and the exhaustive-grid row kernel with one scale
// record per level image and the node table at factor 1 in the canvas's pitch.  ONE loop: an iteration either moves on to the next
// sub-batch of frames or runs the next canvas of the current one (a sub-batch's host frames are uploaded once, before its first
// canvas).  Appends the raw candidates (rect.frame = the region's index) to *all; *oversized: regions no canvas holds.
int run_cv_rois_levels(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois, int W, int H, int CH,
                       const vj_cv_params* p, uint64_t budget_px, std::vector<vj_rect>* all, vj_result* out, StageProgram* prog_out,
                       std::vector<int>* oversized) {
    CvCascadeHost ch;
    int rc = cv_cascade_host(c, &ch);
    if (rc) return rc;
    *prog_out = ch.prog;
    const std::vector<uint32_t>& order = ch.order;
    const CvShape& shape = ch.shape;
    const std::vector<StageDev>& stages = ch.stages;
    const bool count = (p->flags & VJ_FLAG_COUNTERS) != 0;
    const size_t n_nodes = c->nodes.size();
    if ((rc = e->d_cv_rl_stages.ensure(stages.size() * sizeof(StageDev)))) return rc;
    HIP_TRY(hipMemcpy(e->d_cv_rl_stages.p, stages.data(), stages.size() * sizeof(StageDev), hipMemcpyHostToDevice));
    DevBuf& d_det = e->d_cv_det;
    DevBuf& d_counts = e->d_cv_counts;
    const size_t counts_bytes = 2 * VJ_MAX_STAGES * sizeof(uint64_t) + 16;   // stage_entered | visited ... | detection count
    if ((rc = d_counts.ensure(counts_bytes))) return rc;
    const int max_frames = cv_max_frames(e, n_frames, frame_elems_for(W, H));
    const std::vector<int> by_frame = cv_rois_by_frame(rois, n_rois);
    std::vector<CvRoiHost> regs;
    CvTapCache taps;
    size_t taps_uploaded = 0;
    CvRegionCanvas cv;
    std::vector<CvNodeRec> table(n_nodes);
    uint32_t table_stride = 0;
    uint64_t max_reach = 0;
    std::vector<CvScaleDev> scales;
    std::vector<UnitDev> rows;
    uint32_t det_cap = 1u << 16;
    const uint8_t* d_gray = nullptr;
    size_t gray_frame_bytes = 0;
    int gray_stride = 0;
    bool staged = false;
    size_t next = 0, pos = 0;
    int f0 = 0, nf = 0;
    vj_cv_rois_info& info = e->cv_rois_info;
    for (;;) {
        if (pos == regs.size()) {   // ---- the next sub-batch of frames
            f0 += nf;
            if (f0 >= n_frames || next >= by_frame.size()) break;
            nf = std::min(max_frames, n_frames - f0);
            cv_rois_of_subbatch(rois, by_frame, &next, f0, nf, &regs);
            pos = 0;
            staged = false;
            continue;
        }
        // ---- the next canvas of this sub-batch
        if ((rc = cv_roi_plan_canvas(regs, pos, c->win_w, c->win_h, p->scale_factor, p->min_w, p->min_h, budget_px, &taps, &cv))) return rc;
        if (cv.oversized) oversized->push_back(regs[pos].id);
        pos += cv.n_regions;
        info.level_images += cv.n_empty_levels;
        if (cv.oversized || cv.levels.empty()) continue;   // (regions too small for any level leave nothing to run)
        if (!staged) {   // (a sub-batch no level image comes from is not uploaded)
            if ((rc = ensure_gray_staging(e, W, H, nf, CH))) return rc;
            if ((rc = stage_frames(e, frames + f0, nf, W, H, &d_gray, &gray_frame_bytes, &gray_stride))) return rc;
            staged = true;
        }
        const int IW = (int)cv.w, IH = (int)cv.h;
        const uint32_t stride = cv.w + 1u;
        const uint32_t frame_elems = frame_elems_for(IW, IH);
        if ((rc = ensure_image_buffers(e, IW, IH, 1, false))) return rc;
        if ((rc = e->d_pyr.ensure((size_t)cv.pitch * (size_t)cv.h))) return rc;
        // the cascade at factor 1 (cvSetImagesForHaarClassifierCascade(.., 1.), tempcv.cpp:1321) in this canvas's pitch
        const CvEquRect q = cv_equ_rect(c->win_w, c->win_h, 1.);
        if (table_stride != stride) {
            max_reach = 0;
            if ((rc = build_cv_node_recs(c, 1., stride, q.inv_area, table.data(), &max_reach))) return rc;
            if ((rc = e->d_cv_rl_table.ensure(std::max<size_t>(table.size(), 1) * sizeof(CvNodeRec)))) return rc;
            HIP_TRY(hipStreamSynchronize(e->stream));   // (the last canvas's pass is done: every iteration ends in a synchronise)
            if (!table.empty()) HIP_TRY(hipMemcpy(e->d_cv_rl_table.p, table.data(), table.size() * sizeof(CvNodeRec), hipMemcpyHostToDevice));
            table_stride = stride;
        }
        scales.assign(cv.levels.size(), CvScaleDev{});
        rows.clear();
        rows.reserve(cv.n_rows);
        for (size_t k = 0; k < cv.levels.size(); ++k) {
            const CvLevelHost& l = cv.levels[k].lv;
            const PyrRegionLevelDev& d = cv.dev[k];
            CvScaleDev& sd = scales[k];
            memset(&sd, 0, sizeof(sd));
            sd.ystep = (double)l.step;
            cv_set_equ_rect(&sd, q, stride);
            sd.win_w = (uint32_t)l.win_w;
            sd.win_h = (uint32_t)l.win_h;
            sd.end_x = (uint32_t)l.end_x;
            sd.end_y = (uint32_t)l.end_y;
            sd.table_first = 0u;
            sd.scale_idx = (uint32_t)l.idx;
            // a level image's windows lie inside it, and it inside the canvas
            const uint64_t origin_max = (uint64_t)(d.oy + d.h - (uint32_t)c->win_h) * stride + (uint64_t)(d.ox + d.w - (uint32_t)c->win_w);
            if (d.ox + d.w > cv.w || d.oy + d.h > cv.h || origin_max + std::max<uint64_t>(max_reach, sd.q3) >= (uint64_t)frame_elems) {
                set_error("feature reach exceeds the canvas allocation");
                return VJ_ERR_LIMIT;
            }
            for (uint32_t iy = 0; iy < sd.end_y; ++iy) rows.push_back(UnitDev{(uint32_t)k, iy, d.oy * stride + d.ox, 0});
        }
        if ((rc = e->d_cv_rl_levels.ensure(cv.dev.size() * sizeof(PyrRegionLevelDev)))) return rc;
        if ((rc = e->d_cv_rl_scales.ensure(scales.size() * sizeof(CvScaleDev)))) return rc;
        if ((rc = e->d_cv_rl_rows.ensure(rows.size() * sizeof(UnitDev)))) return rc;
        HIP_TRY(hipMemcpy(e->d_cv_rl_levels.p, cv.dev.data(), cv.dev.size() * sizeof(PyrRegionLevelDev), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_cv_rl_scales.p, scales.data(), scales.size() * sizeof(CvScaleDev), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(e->d_cv_rl_rows.p, rows.data(), rows.size() * sizeof(UnitDev), hipMemcpyHostToDevice));
        if (taps_uploaded != taps.taps.size()) {   // (the call's taps grow by the pairs this canvas saw first)
            if ((rc = e->d_cv_rl_taps.ensure(taps.taps.size() * sizeof(PyrTap)))) return rc;
            HIP_TRY(hipMemcpy(e->d_cv_rl_taps.p, taps.taps.data(), taps.taps.size() * sizeof(PyrTap), hipMemcpyHostToDevice));
            taps_uploaded = taps.taps.size();
        }
        PyrRegionArgs pa;
        memset(&pa, 0, sizeof(pa));
        pa.gray = d_gray;
        pa.gray_frame_bytes = gray_frame_bytes;
        pa.gray_stride = (uint32_t)gray_stride;
        pa.channels = (uint32_t)CH;
        pa.width = (uint32_t)W;
        pa.height = (uint32_t)H;
        pa.n_frames = (uint32_t)nf;
        pa.levels = (const PyrRegionLevelDev*)e->d_cv_rl_levels.p;
        pa.n_levels = (uint32_t)cv.dev.size();
        pa.n_units = cv.n_pyr_units;
        pa.taps = (const PyrTap*)e->d_cv_rl_taps.p;
        pa.canvas = (uint8_t*)e->d_pyr.p;
        pa.canvas_pitch = cv.pitch;
        pa.canvas_w = cv.w;
        pa.canvas_h = cv.h;
        HIP_TRY(hipEventRecord(e->lane0.ev[0], e->stream));
        int hrc = launch_pyramid_regions(pa, e->stream);
        if (hrc) {
            set_error("pyramid launch failed: %s", hipGetErrorString((hipError_t)hrc));
            return VJ_ERR_HIP;
        }
        HIP_TRY(hipEventRecord(e->cv_rois_ev[0], e->stream));
        // from here on the "frame" is the gray canvas
        const uint8_t* d_canvas = (const uint8_t*)e->d_pyr.p;
        const size_t canvas_bytes = (size_t)cv.pitch * (size_t)cv.h;
        if ((rc = enqueue_integral(e, d_canvas, canvas_bytes, (int)cv.pitch, IW, IH, 1, 1))) return rc;
        if (shape.has_tilted && (rc = enqueue_tilted(e, d_canvas, canvas_bytes, (int)cv.pitch, IW, IH, 1, 1))) return rc;
        HIP_TRY(hipEventRecord(e->lane0.ev[1], e->stream));
        std::vector<unsigned long long> h;
        uint32_t n_det = 0;
        rc = run_cv_pass_until_fit(e, counts_bytes, &det_cap, "vj_detect_opencv_rois: the detection buffer overflowed twice", [&](uint32_t cap) {
            const CvTables tables{e->d_cv_rl_table.p, e->d_cv_rl_scales.p, e->d_cv_rl_stages.p, (uint32_t)order.size(), (uint32_t)c->stages.size()};
            CvArgs a = cv_base_args(e, facts_of(shape), tables, CvGeom{frame_elems, stride, (uint32_t)IH + 1u, 1u}, d_det.p, cap, d_counts.p);
            a.rows = (const UnitDev*)e->d_cv_rl_rows.p;
            a.n_rows = (uint32_t)rows.size();
            // one wave per row unit, at most four workgroups (16 waves) per CU; the rest by stride
            // (a stage tree walks every position to the end of the tree: a.chains stays empty, the per-lane target-stage sweep)
            const int n_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((rows.size() + CV_WAVES_PER_BLOCK - 1) / CV_WAVES_PER_BLOCK, (uint64_t)std::max(1, e->n_cu * 4)));
            a.total_waves = (uint32_t)n_blocks * CV_WAVES_PER_BLOCK;
            return cascade_launched(launch_cv_profile_pass(a, shape.trees, count, shape.is_tree, n_blocks, e->stream, false, true));
        }, &h, &n_det);
        if (rc) return rc;
        float ms_p = 0, ms_i = 0, ms_c = 0;
        HIP_TRY(hipEventElapsedTime(&ms_p, e->lane0.ev[0], e->cv_rois_ev[0]));
        HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_c, e->lane0.ev[2], e->lane0.ev[3]));
        out->timing.integral_ms += ms_i;
        out->timing.cascade_ms += ms_c;
        out->timing.total_ms += ms_i + ms_c;
        out->timing.n_cascade_launches += 1;
        info.pyramid_ms += ms_p;
        if (count) add_cv_counters(h, c->stages.size(), &out->counters);
        std::vector<CvDet> raw;
        if ((rc = read_cv_dets(e, n_det, &raw))) return rc;
        for (const CvDet& d : raw) {
            if (d.slot >= cv.levels.size()) {
                set_error("the level pass returned a detection outside its level images");
                return VJ_ERR_HIP;
            }
            // Rect(cvRound(x * factor), cvRound(y * factor), winSize) (tempcv.cpp:1099-1100), relative to the region
            const CvRegionLevel& L = cv.levels[d.slot];
            all->push_back(vj_rect{cv_round((double)d.x * L.lv.factor), cv_round((double)d.y * L.lv.factor), L.lv.win_w, L.lv.win_h, 0.0f,
                                   regs[(size_t)L.region].id, L.lv.idx});
        }
        info.canvases += 1;
        info.level_images += cv.levels.size();
        info.windows += cv.windows;
        if ((uint64_t)cv.w * cv.h > (uint64_t)info.canvas_w * info.canvas_h) {
            info.canvas_w = cv.w;
            info.canvas_h = cv.h;
        }
    }
    return VJ_OK;
}

}  // namespace

extern "C" {

int vj_detect_opencv(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_cv_params* p,
                     vj_result* out) {
    return detect_opencv_impl(e, c, frames, n_frames, p, out, false, nullptr);
}

void vj_cv_roc_params_default(vj_cv_roc_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->scale_factor = 1.1;
    p->flags = VJ_FLAG_CV_SCALE_IMAGE;
}

void vj_roc_result_free(vj_roc_result* r) {
    if (!r) return;
    free(r->r.rects);
    free(r->reject_levels);
    free(r->level_weights);
    r->r.rects = nullptr;
    r->r.count = 0;
    r->reject_levels = nullptr;
    r->level_weights = nullptr;
}

// cvHaarDetectObjectsForROC(..., outputRejectLevels = true) (tempcv.cpp:1188-1503)
int vj_detect_opencv_roc(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_cv_roc_params* p, vj_roc_result* out) {
    if (!e || !c || !p || !out) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (p->max_w < 0 || p->max_h < 0) {
        set_error("max_w / max_h must be >= 0");
        return VJ_ERR_ARG;
    }
    if ((p->flags & VJ_FLAG_CV_FIND_BIGGEST) != 0u) {   // clears scale-image (:1227), then reads an empty rweights (:1486)
        set_error("vj_detect_opencv_roc: reject levels with VJ_FLAG_CV_FIND_BIGGEST are not a meaningful result");
        return VJ_ERR_UNSUPPORTED;
    }
    if ((p->flags & VJ_FLAG_CV_SCALE_IMAGE) == 0u) {    // the scale-cascade invoker (:1116-1185) never pushes a level
        set_error("vj_detect_opencv_roc: reject levels exist in the VJ_FLAG_CV_SCALE_IMAGE branch only");
        return VJ_ERR_UNSUPPORTED;
    }
    if (c->stages.size() < 4) {                         // n + result < 4 would hold for rejects at stage 0: every grid position
        set_error("vj_detect_opencv_roc: a cascade of %zu stages; reject levels need at least 4", c->stages.size());
        return VJ_ERR_UNSUPPORTED;
    }
    if (n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    if (n_frames == 0) return VJ_OK;
    vj_cv_params q;
    memset(&q, 0, sizeof(q));
    q.min_w = p->min_w;
    q.min_h = p->min_h;
    q.scale_factor = p->scale_factor;
    q.min_neighbors = p->min_neighbors;
    q.flags = p->flags & (VJ_FLAG_COUNTERS | VJ_FLAG_CV_SCALE_IMAGE | VJ_FLAG_EQUALIZE_HIST);   // (canny pruning and rough search: not read by this branch)
    std::vector<int32_t> levels;
    std::vector<double> weights;
    const bool whole = p->max_w == 0 || p->max_h == 0;   // maxSize with a zero member is the frame (:1230-1234)
    const CvRocCall roc{{whole ? frames[0].width : p->max_w, whole ? frames[0].height : p->max_h}, &levels, &weights};
    int rc = detect_opencv_impl(e, c, frames, n_frames, &q, &out->r, false, nullptr, &roc);
    if (rc) {
        vj_roc_result_free(out);
        return rc;
    }
    int n = (int)out->r.count;
    if (p->min_neighbors != 0 && n != 0) {   // groupRectangles(rectList, rejectLevels, levelWeights, minNeighbors, GROUP_EPS) (:1466)
        n = vj_group_rectangles_levels(out->r.rects, levels.data(), weights.data(), n, (int)std::min<uint32_t>(p->min_neighbors, 0x7fffffffu), 0.2);
        if (n < 0) {
            vj_roc_result_free(out);
            return -n;
        }
        out->r.count = (uint32_t)n;
    }
    if (n != 0) {
        out->reject_levels = (int32_t*)malloc((size_t)n * sizeof(int32_t));
        out->level_weights = (double*)malloc((size_t)n * sizeof(double));
        if (!out->reject_levels || !out->level_weights) {
            vj_roc_result_free(out);
            return VJ_ERR_NOMEM;
        }
        memcpy(out->reject_levels, levels.data(), (size_t)n * sizeof(int32_t));
        memcpy(out->level_weights, weights.data(), (size_t)n * sizeof(double));
    } else {
        free(out->r.rects);
        out->r.rects = nullptr;
    }
    return VJ_OK;
}

int vj_detect_opencv_rois(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                          const vj_cv_params* p, vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || n_rois < 0 || (n_rois > 0 && (!frames || !rois))) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (refuse_equalize(p->flags, "vj_detect_opencv_rois")) return VJ_ERR_UNSUPPORTED;
    if (!(p->scale_factor > 1.0)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    for (int i = 0; i < n_rois; ++i)
        if (!cv_roi_inside(rois[i], frames, n_frames)) {
            set_error("roi %d lies outside its frame", i);
            return VJ_ERR_ARG;
        }
    e->cv_rois_info = vj_cv_rois_info{};
    e->cv_rois_info.regions = (uint64_t)n_rois;
    if (n_rois == 0) return VJ_OK;
    int W, H, CH;
    // (many regions of few sizes stay on the per-size route, which is faster for them: cv_rois_levels_pay)
    if ((p->flags & VJ_FLAG_CV_SCALE_IMAGE) != 0u && (p->flags & ~CV_ROI_LEVEL_FLAGS) == 0u && cv_frames_uniform(frames, n_frames, &W, &H, &CH) &&
        cv_rois_levels_pay(rois, n_rois)) {
        // ---- CV_HAAR_SCALE_IMAGE: every region's level images on canvases, one pass per canvas
        HIP_TRY(hipSetDevice(e->device));
        e->cv_rois_info.route = 2;
        std::vector<vj_rect> all;
        std::vector<int> oversized;
        StageProgram prog;
        int rc = run_cv_rois_levels(e, c, frames, n_frames, rois, n_rois, W, H, CH, p, CV_ROI_CANVAS_PX, &all, out, &prog, &oversized);
        if (rc) return rc;
        if (oversized.empty()) return finish_cv_roi_result(all, &prog, p, out);
        // regions too large for a canvas: the per-size route below for them, merged region by region (each part is in its final
        // order and a region's rectangles all come from one part)
        e->cv_rois_info.route = 4;
        if ((rc = finish_cv_roi_result(all, &prog, p, out))) return rc;
        all.assign(out->rects, out->rects + out->count);
        free(out->rects);
        out->rects = nullptr;
        out->count = 0;
        std::vector<vj_roi> big(oversized.size());
        for (size_t i = 0; i < big.size(); ++i) big[i] = rois[oversized[i]];
        for (const CvRoiSizeGroup& g : cv_roi_size_groups(frames, big.data(), (int)big.size())) {
            std::vector<int> idx(g.idx.size());
            for (size_t i = 0; i < idx.size(); ++i) idx[i] = oversized[(size_t)g.idx[i]];
            vj_result part;
            rc = vj_detect_opencv(e, c, g.views.data(), (int)g.views.size(), p, &part);
            if (!rc) rc = cv_roi_take_part(part, idx, &all, out);
            vj_result_free(&part);
            if (rc) return rc;
        }
        return cv_roi_emit_parts(all, out);
    }
    // (VJ_FLAG_CV_CHAIN_DEVICE belongs to vj_detect_opencv_chain: ignored here)
    if ((p->flags & ~(CV_ROI_FAST_FLAGS | (uint32_t)VJ_FLAG_CV_CHAIN_DEVICE)) == 0u && cv_frames_uniform(frames, n_frames, &W, &H, &CH)) {
        e->cv_rois_info.route = 1;
    // ---- every region in one pass per sub-batch, on the frames' own integral images
        HIP_TRY(hipSetDevice(e->device));
        const std::vector<int> by_frame = cv_rois_by_frame(rois, n_rois);
        bool has_tilted = false;
        for (const auto& nd : c->nodes) has_tilted |= nd.tilted != 0;
        const int max_frames = cv_max_frames(e, n_frames, frame_elems_for(W, H));
        std::vector<vj_rect> all;
        std::vector<CvRoiHost> regs;
        CvRoiPlan* pl = nullptr;
        size_t next = 0;
        int rc;
        for (int f0 = 0; f0 < n_frames && next < by_frame.size(); f0 += max_frames) {
            const int nf = std::min(max_frames, n_frames - f0);
            cv_rois_of_subbatch(rois, by_frame, &next, f0, nf, &regs);
            if (regs.empty()) continue;   // (a sub-batch no region looks at is not uploaded; within one, every frame is)
            if ((rc = enqueue_cv_ingest(e, frames + f0, nf, W, H, CH, false, nullptr, has_tilted))) return rc;
            uint64_t n_windows = 0;
            if ((rc = run_cv_roi_pass(e, c, W, H, nf, regs, p, &all, out, &pl, nullptr, &n_windows))) return rc;   // (ends in a stream synchronise)
            e->cv_rois_info.windows += n_windows;
            HIP_TRY(hipEventSynchronize(e->lane0.ev[1]));   // (so this returns at once, also when the pass had nothing to launch)
            float ms_i = 0;
            HIP_TRY(hipEventElapsedTime(&ms_i, e->lane0.ev[0], e->lane0.ev[1]));
            out->timing.integral_ms += ms_i;
            out->timing.total_ms += ms_i;
        }
        return finish_cv_roi_result(all, pl ? &pl->prog : nullptr, p, out);
    }
    // ---- frames of differing sizes, or a flag whose result on a crop is not a crop of its result on the frame (the edge map, the
    // find-biggest search; the resized image when the frames differ in size): one vj_detect_opencv call per region size (and channel
    // count) on the sub-images
    e->cv_rois_info.route = 3;
    std::vector<vj_rect> all;
    for (const CvRoiSizeGroup& g : cv_roi_size_groups(frames, rois, n_rois)) {
        vj_result part;
        int rc = vj_detect_opencv(e, c, g.views.data(), (int)g.views.size(), p, &part);
        if (!rc) rc = cv_roi_take_part(part, g.idx, &all, out);
        vj_result_free(&part);
        if (rc) return rc;
    }
    return cv_roi_emit_parts(all, out);
}

int vj_detect_opencv_chain(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames, int n_frames,
                           const vj_cv_params* p_first, const vj_cv_params* p_second, vj_result* out_first, vj_result* out_second) {
    if (!e || !first || !second || !p_first || !p_second || !out_first || !out_second || n_frames < 0 || (n_frames > 0 && !frames))
        return VJ_ERR_ARG;
    memset(out_first, 0, sizeof(*out_first));
    memset(out_second, 0, sizeof(*out_second));
    if (refuse_equalize(p_first->flags | p_second->flags, "vj_detect_opencv_chain")) return VJ_ERR_UNSUPPORTED;
    if (n_frames == 0) return VJ_OK;
    if (!(p_first->scale_factor > 1.0) || !(p_second->scale_factor > 1.0)) {
        set_error("scale_factor must be > 1");
        return VJ_ERR_ARG;
    }
    // VJ_FLAG_CV_CHAIN_DEVICE is read here and nowhere else: from now on both parameter blocks are without it
    const CvChainRoute route = cv_chain_route(p_first->flags, p_second->flags);
    vj_cv_params q_first = *p_first, q_second = *p_second;
    q_first.flags = route.flags_first;
    q_second.flags = route.flags_second;
    p_first = &q_first;
    p_second = &q_second;
    e->cv_chain_info = vj_cv_chain_info{};
    e->cv_chain_info.handoff = route.handoff;
    if (((p_first->flags | p_second->flags) & ~CV_ROI_FAST_FLAGS) != 0u) {
        // the two public calls back to back: what `first` finds are the regions
        int rc = vj_detect_opencv(e, first, frames, n_frames, p_first, out_first);
        if (rc) return rc;
        std::vector<vj_roi> rois(out_first->count);
        for (uint32_t i = 0; i < out_first->count; ++i) {
            const vj_rect& r = out_first->rects[i];
            rois[i] = vj_roi{r.frame, r.x, r.y, r.w, r.h};
        }
        e->cv_chain_info.regions = out_first->count;
        return vj_detect_opencv_rois(e, second, frames, n_frames, rois.data(), (int)rois.size(), p_second, out_second);
    }
    // ---- per sub-batch: the frames' integral images once (with the tilted integral when either cascade reads it), `first` on the
    // frames, its candidates — sorted, grouped per frame when p_first asks for it — as regions, `second` inside them
    bool second_tilted = false;
    for (const auto& nd : second->nodes) second_tilted |= nd.tilted != 0;
    const int W = frames[0].width, H = frames[0].height;
    std::vector<vj_rect> all, regions;
    std::vector<CvRoiHost> regs;
    CvRoiPlan* pl = nullptr;
    const CvSubBatchHook hook = [&](int f0, int nf, const vj_rect* raw, size_t n_raw) -> int {
        int hrc = cv_chain_regions(raw, n_raw, p_first->min_neighbors, W, H, f0, nf, &regs, &regions);
        if (hrc) return hrc;
        uint64_t n_units = 0, n_windows = 0;
        if (!regs.empty() && (hrc = run_cv_roi_pass(e, second, W, H, nf, regs, p_second, &all, out_second, &pl, &n_units, &n_windows))) return hrc;
        cv_chain_info_add(&e->cv_chain_info, false, regs.size(), n_units, n_windows);
        return VJ_OK;
    };
    int uW, uH, uCH;   // (frames the profile does not take as a batch: the host route reports them as it always did)
    if (route.handoff == 1 && cv_frames_uniform(frames, n_frames, &uW, &uH, &uCH)) {
        // ---- the hand-off on the device: both cascades are enqueued before the host waits, once per sub-batch
        HIP_TRY(hipSetDevice(e->device));
        CvChainDevice dev;
        dev.e = e;
        dev.second = second;
        dev.p_second = p_second;
        dev.grouped = p_first->min_neighbors != 0;
        dev.threshold = (int32_t)std::min<uint32_t>(std::max<uint32_t>(p_first->min_neighbors, 1u), 0x7fffffffu);
        dev.W = W;
        dev.H = H;
        dev.host_hook = &hook;
        dev.out_second = out_second;
        dev.all2 = &all;
        dev.regions = &regions;
        int rc = dev.begin();
        if (rc) return rc;
        if (dev.rp) {
            pl = dev.rp;
            if ((rc = detect_opencv_impl(e, first, frames, n_frames, p_first, out_first, second_tilted, &hook, nullptr, &dev))) return rc;
            return finish_cv_roi_result(all, &pl->prog, p_second, out_second);
        }
        // (a frame too small for any scale of the second cascade: nothing to hand off)
    }
    if (route.handoff == 1) e->cv_chain_info.handoff = 2;
    int rc = detect_opencv_impl(e, first, frames, n_frames, p_first, out_first, second_tilted, &hook);
    if (rc) return rc;
    // (grouping is per frame and the sub-batches are runs of frames: the regions are out_first's rectangles, in order)
    if (!cv_chain_regions_match(regions, *out_first)) {
        set_error("vj_detect_opencv_chain: the regions are not the first cascade's rectangles");
        return VJ_ERR_UNSUPPORTED;
    }
    return finish_cv_roi_result(all, pl ? &pl->prog : nullptr, p_second, out_second);
}

// cvSetImagesForHaarClassifierCascade + cvRunHaarClassifierCascade on a caller's windows (tempcv.cpp:549-768, :795-984)
int vj_run_windows_opencv(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const double* scales, int n_scales,
                          const vj_window* windows, uint32_t n_windows, int start_stage, vj_window_result* out) {
    return run_points<CvPoints>(e, c, frames, n_frames, scales, n_scales, windows, n_windows, start_stage, 0u, out);
}

int vj_cv_rois_info_get(const vj_env* e, vj_cv_rois_info* out) {
    if (!e || !out) return VJ_ERR_ARG;
    *out = e->cv_rois_info;
    return VJ_OK;
}

int vj_cv_chain_info_get(const vj_env* e, vj_cv_chain_info* out) {
    if (!e || !out) return VJ_ERR_ARG;
    *out = e->cv_chain_info;
    return VJ_OK;
}

int vj_run_windows_timing(const vj_env* e, float* integral_ms, float* pass_ms) {
    if (!e) return VJ_ERR_ARG;
    if (integral_ms) *integral_ms = e->points_integral_ms;
    if (pass_ms) *pass_ms = e->points_pass_ms;
    return VJ_OK;
}

}  // extern "C"
