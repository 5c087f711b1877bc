// Host driver of the HIP path: device buffers, per-(cascade, size, params) plans and
// the launch sequence of one vj_detect call.  It replaces clodInitEnvironment /
// clodInitBuffers / clodDetectObjectsOpenCL (clod.cpp:72-163, 1176-1336): where the
// reference does, per frame, one blocking launch + count read-back per (scale, stage)
// — up to 924 round trips at 1080p — this driver enqueues 3 integral launches and a
// handful of cascade passes for the WHOLE batch and synchronises once.
#include "vj_internal.hpp"
#include "vj_device.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>

#include "vj_slice.hpp"
#include "vj_grid_parts.hpp"
#include "vj_atlas_units.hpp"

using namespace vj;

namespace vj {

static uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// The device copies of a plan: every table at the size its kernels index, at least one element where a launch binds the
// pointer of an empty list.  (The scale records are only allocated: layout_queues copies them once the queue segments of
// the call's frame count are laid out.)
static int upload_plan(Plan* pl, const PlanTables& tab) {
    struct Row { DevBuf* buf; const void* src; size_t bytes, min_bytes; };
    const Row rows[] = {
        {&pl->d_skip_units, tab.skip_units.data(), tab.skip_units.size() * sizeof(UnitDev), 0},
        {&pl->d_skip_segs, tab.skip_segs.data(), tab.skip_segs.size() * sizeof(UnitDev), 0},
        {&pl->d_table, tab.table.data(), tab.table.size() * sizeof(NodeRec), sizeof(NodeRec)},
        {&pl->d_scales, nullptr, pl->scales.size() * sizeof(ScaleDev), sizeof(ScaleDev)},
        {&pl->d_stages, pl->stages.data(), pl->stages.size() * sizeof(StageDev), 0},
        {&pl->d_units, pl->units.data(), pl->units.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_tile_units, pl->tile_units.data(), pl->tile_units.size() * sizeof(UnitDev), sizeof(UnitDev)},
        {&pl->d_pos_tab, tab.pos_tab.data(), tab.pos_tab.size() * sizeof(uint32_t), 0},
        {&pl->d_unit_groups, pl->unit_groups.data(), pl->unit_groups.size() * sizeof(UnitDev), 0},
        {&pl->d_sp_blocks, tab.sp_blocks.data(), tab.sp_blocks.size() * sizeof(SpBlock), sizeof(SpBlock)},
    };
    for (const Row& r : rows) {
        const size_t want = std::max(r.bytes, r.min_bytes);
        if (!want) continue;   // (an empty list nothing binds; the stage records too: the loader refuses a cascade without stages)
        if (const int rc = r.buf->ensure(want)) return rc;
        if (r.src && r.bytes) HIP_TRY(hipMemcpy(r.buf->p, r.src, r.bytes, hipMemcpyHostToDevice));
    }
    return VJ_OK;
}

// The plan of a call of n_frames frames under the environment's settings (plan_clod, vj_clod_plan.cpp), then its device copies.
static int plan_and_upload(const vj_env* e, const vj_cascade& c, int W, int H, const vj_params& p, Plan* pl, float tile_split,
                           const TileThresholds& thresholds, int n_frames, bool one_pass) {
    PlanTables tab;
    const int rc = plan_clod(*e, e->tile_group, e->sq32, c, W, H, p, tile_split, thresholds, n_frames, one_pass, false, pl, &tab);
    return rc ? rc : upload_plan(pl, tab);
}

// (Re)lay out the per-scale queue segments for `frames` frames in flight.
static int layout_queues(Plan* pl, int frames, uint64_t* total_entries) {
    // a scale's segment: Q_PARTS parts, part x takes the windows of frames with frame * Q_PARTS / frames == x,
    // i.e. at most ceil(frames / Q_PARTS) frames (fewer frames than parts: one part per frame, the rest unused)
    const uint64_t frames_per_part = frames >= (int)Q_PARTS ? ((uint64_t)frames + Q_PARTS - 1) / Q_PARTS : 1;
    uint64_t base = 0;
    for (ScaleDev& sd : pl->scales) {
        sd.q_base = (uint32_t)base;
        sd.q_cap = (uint32_t)((uint64_t)sd.nwin * frames_per_part);
        base += (uint64_t)sd.nwin * frames_per_part * std::min<uint64_t>(Q_PARTS, (uint64_t)frames);
    }
    *total_entries = base;
    if (base > 0xffffffffull) {
        set_error("survivor queue needs %llu entries", (unsigned long long)base);
        return VJ_ERR_LIMIT;
    }
    if (pl->frames_q != frames && !pl->scales.empty()) {
        HIP_TRY(hipMemcpy(pl->d_scales.p, pl->scales.data(), pl->scales.size() * sizeof(ScaleDev),
                          hipMemcpyHostToDevice));
        pl->frames_q = frames;
    }
    return VJ_OK;
}

// The workload whose chain balance is being found (or was found) by feedback: batches of >= 8 frames through vj_detect.
static vj_env::BalanceKey balance_key(const vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, int n_frames) {
    return vj_env::BalanceKey(vj_env::PlanKey(c->content_hash, W, H, p.min_w, p.min_h, p.max_w, p.max_h, f2u(p.scale_factor), p.scale_mask[0],
                                              p.scale_mask[1], p.flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW | VJ_FLAG_GRID_F64 | VJ_FLAG_TILTED_AS_UPRIGHT), 0u),
                              e->balance_class(n_frames));
}

static vj_env::Balance* balance_of(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, int n_frames, bool create) {
    // (calls of at least eight frames or sixteen megapixels: below that a call is a millisecond and its time says little)
    if (!e->auto_balance || e->tile_split_set || !e->concurrent || n_frames >= (1 << 20) ||
        (n_frames < 8 && (uint64_t)W * (uint64_t)H * (uint64_t)n_frames < 16000000ull))
        return nullptr;
    const vj_env::BalanceKey key = balance_key(e, c, W, H, p, n_frames);
    auto it = e->balance.find(key);
    if (it != e->balance.end()) {
        it->second.last_used = ++e->balance_tick;
        return &it->second;
    }
    if (!create) return nullptr;
    while (e->balance.size() >= 256) {   // bounded: the least recently used workload goes (a frozen result is cheap to find again)
        auto lru = e->balance.begin();
        for (auto i = e->balance.begin(); i != e->balance.end(); ++i)
            if (i->second.last_used < lru->second.last_used) lru = i;
        e->balance.erase(lru);
    }
    vj_env::Balance b;
    b.cur = b.best = e->split_for(n_frames, p, linear_stumps(*c));
    b.n_ref = n_frames;
    b.last_used = ++e->balance_tick;
    return &(e->balance[key] = b);
}

// What a call of n_frames frames runs: the candidate under test when it is one of the workload's sampling calls (the class's
// reference size, search not finished), else the best split known.
struct BalanceChoice {
    float split;
    int thr;
    bool candidate;
};
static BalanceChoice balance_choice(const vj_env::Balance* b, int n_frames) {
    if (b->phase != 3 && n_frames == b->n_ref) return BalanceChoice{b->cur, b->thr, b->cur != b->best || b->phase == 4};
    return BalanceChoice{b->best, b->phase == 4 ? 0 : b->thr, false};
}

// Called once per vj_detect / vj_detect_chain call of a balanced workload, before its plan is looked up: bookkeeping, and the
// reference size follows the traffic (a class whose reference size stopped coming — 32 calls of other sizes — restarts the
// measurement of its current best at the size that does come; what was found so far stays the starting point).
static void balance_touch(vj_env::Balance* b, int n_frames) {
    ++b->calls_total;
    if (b->phase == 3) return;
    if (n_frames == b->n_ref) {
        b->off_ref = 0;
    } else if (++b->off_ref > 32) {
        b->n_ref = n_frames;
        b->off_ref = 0;
        b->cur = b->best;
        b->phase = 0;
        b->samples = 0;
        b->moved = 0;
    }
    if (balance_choice(b, n_frames).candidate) ++b->calls_on_candidate;
}

// One more measured call (cascade kernels' time per frame, uncounted variants, the class's reference batch size) of a workload
// that is still being balanced.  Three calls per candidate — the first unrated (a new plan's tables were just uploaded: the
// device idled), the faster of the other two counts — or two when both the unrated call and the first rated one were already
// more than 3 % slower than the best: such a candidate is dropped at once.  Steps of a quarter of a scale; a move needs 0.7 %;
// at most 40 calls per workload.
static void balance_report(vj_env::Balance* b, float ms, bool try_thresholds) {
    if (!b || b->phase == 3 || !(ms > 0.0f)) return;
    ++b->calls;
    bool early_drop = false;
    if (++b->samples == 1) {
        b->cand_ms = 1e30f;
        b->first_slow = b->phase != 0 && ms > b->best_ms * 1.03f;
        return;
    }
    b->cand_ms = std::min(b->cand_ms, ms);
    if (b->samples == 2 && b->first_slow && b->phase != 0 && ms > b->best_ms * 1.03f) early_drop = true;
    if (b->samples < 3 && !early_drop) return;
    b->samples = 0;
    const float step = 0.25f, max_split = 3.0f;
    const int max_calls = 40;
    // the split is settled: one more candidate — the same split with the lower tile thresholds (how many scales the tile chain
    // can take at all: the better value depends on the frames' content, profiles/r03_notes.md #6e) — then the search ends
    // — and before that one probe a whole scale further: the response is not always convex (a scale split between the two
    // chains can cost more than the same scale moved entirely), and a climb in quarters stops at the first rise
    auto freeze = [&]() {
        b->cur = b->best;
        if (!b->far_tried && b->best + 1.0f <= max_split && b->calls <= max_calls) {
            b->far_tried = true;
            b->cur = b->best + 1.0f;
            b->phase = 5;
        } else if (try_thresholds && !b->thr_tried && b->calls <= max_calls) {
            b->thr_tried = true;
            b->thr = 1;
            b->phase = 4;
        } else {
            b->phase = 3;
        }
    };
    if (b->phase == 4) {
        if (b->cand_ms < b->best_ms * 0.993f) b->best_ms = b->cand_ms;
        else b->thr = 0;
        b->phase = 3;
        return;
    }
    if (b->phase == 5) {
        if (b->cand_ms < b->best_ms * 0.993f) {   // the far side is better: climb on from there
            b->best = b->cur;
            b->best_ms = b->cand_ms;
            b->moved = 0;
            b->phase = 1;
            if (b->best + step <= max_split) b->cur = b->best + step;
            else { b->phase = 2; b->cur = b->best - step; }
        } else {
            freeze();
        }
        return;
    }
    if (b->phase == 0) {
        b->best_ms = b->cand_ms;
        b->phase = 1;
        if (b->best + step <= max_split) b->cur = b->best + step;
        else if (b->best >= step) { b->phase = 2; b->cur = b->best - step; }
        else freeze();
        return;
    }
    const bool better = b->cand_ms < b->best_ms * 0.993f;
    if (better) {
        b->best = b->cur;
        b->best_ms = b->cand_ms;
        b->moved = 1;
        const float next = b->phase == 1 ? b->cur + step : b->cur - step;
        if (next < 0.0f || next > max_split || b->calls > max_calls) freeze();
        else b->cur = next;
    } else if (b->phase == 1 && !b->moved && b->best >= step) {
        b->phase = 2;
        b->cur = b->best - step;
    } else {
        freeze();
    }
}

// The found balances as text, one workload per line, so that another environment (or process) can start from them:
//   vjbal1 <cascade content hash> W H min_w min_h max_w max_h <scale factor bits> <mask0> <mask1> <flags> <class> <split> <thr>
static int balance_export(const vj_env* e, const char* path) {
    FILE* f = fopen(path, "w");
    if (!f) {
        set_error("cannot write %s", path);
        return VJ_ERR_IO;
    }
    for (const auto& kv : e->balance) {
        const vj_env::PlanKey& k = std::get<0>(kv.first);
        const vj_env::Balance& b = kv.second;
        // (the last four fields are for the reader of the file: search state — 0 = nothing measured yet, 3 = finished —, calls of
        // the workload, those that ran a split other than the best known, calls the search measured; import skips state 0)
        fprintf(f, "vjbal1 %llx %d %d %d %d %d %d %x %llx %llx %x %d %.4f %d %d %u %u %d\n", (unsigned long long)std::get<0>(k), std::get<1>(k),
                std::get<2>(k), std::get<3>(k), std::get<4>(k), std::get<5>(k), std::get<6>(k), std::get<7>(k), (unsigned long long)std::get<8>(k),
                (unsigned long long)std::get<9>(k), std::get<10>(k), std::get<1>(kv.first), (double)b.best, b.phase == 4 ? 0 : b.thr, b.phase,
                b.calls_total, b.calls_on_candidate, b.calls);
    }
    fclose(f);
    return VJ_OK;
}

static int balance_import(vj_env* e, const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) {
        set_error("cannot read %s", path);
        return VJ_ERR_IO;
    }
    char line[512];
    int n_bad = 0;
    while (fgets(line, sizeof(line), f)) {
        unsigned long long hash, m0, m1;
        int W, H, a, b2, c2, d, cls, thr, state = 3;
        unsigned sf, flags;
        double split;
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, "vjbal1 %llx %d %d %d %d %d %d %x %llx %llx %x %d %lf %d %d", &hash, &W, &H, &a, &b2, &c2, &d, &sf, &m0, &m1, &flags, &cls,
                   &split, &thr, &state) < 14 || !(split >= 0.0 && split <= 3.0) || cls < 1) {
            ++n_bad;
            continue;
        }
        if (state == 0) continue;
        vj_env::Balance b;
        b.cur = b.best = (float)split;
        b.thr = thr ? 1 : 0;
        b.phase = 3;          // frozen: an imported workload does not search again ("auto_balance" "reset" forgets it)
        b.thr_tried = b.far_tried = true;
        b.last_used = ++e->balance_tick;
        e->balance[vj_env::BalanceKey(vj_env::PlanKey((uint64_t)hash, W, H, a, b2, c2, d, (uint32_t)sf, (uint64_t)m0, (uint64_t)m1, (uint32_t)flags, 0u), cls)] = b;
    }
    fclose(f);
    if (n_bad) {
        set_error("%s: %d lines are not balance records", path, n_bad);
        return VJ_ERR_PARSE;
    }
    return VJ_OK;
}

static int get_plan(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, Plan** out, int n_frames = 1 << 20) {
    const vj_env::Balance* bal = balance_of(e, c, W, H, p, n_frames, false);
    const BalanceChoice choice = bal ? balance_choice(bal, n_frames) : BalanceChoice{e->split_for(n_frames, p, linear_stumps(*c)), 0, false};
    const float split = choice.split;
    int small = small_frame_class(*e, W, H, n_frames);
    if (small == 0 && choice.thr == 1 && !e->tile_thresholds_set) small = 3;   // the feedback's lower thresholds
    const bool one_pass = one_pass_for(*e, W, H, n_frames);
    vj_env::PlanKey key(c->uid, W, H, p.min_w, p.min_h, p.max_w, p.max_h, f2u(p.scale_factor), p.scale_mask[0],
                        p.scale_mask[1], (p.flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW | VJ_FLAG_GRID_F64 | VJ_FLAG_TILTED_AS_UPRIGHT)) | ((uint32_t)small << 8) | ((uint32_t)one_pass << 12) |
                            ((e->unit_cap_for(n_frames, false, has_trees(*c)) / 64u) << 16), f2u(split));   // (bits 16-19: the first-pass units' size, which follows the wave count)
    auto it = e->plans.find(key);
    if (it != e->plans.end()) {
        it->second->last_used = ++e->plan_tick;
        *out = it->second.get();
        return VJ_OK;
    }
    // bounded cache: release the least recently used plans first (their kernels may still be running)
    if ((int)e->plans.size() >= std::max(2, e->plan_cache_max)) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->stream2) HIP_TRY(hipStreamSynchronize(e->stream2));
        while ((int)e->plans.size() >= std::max(2, e->plan_cache_max)) {
            auto lru = e->plans.begin();
            for (auto i = e->plans.begin(); i != e->plans.end(); ++i)
                if (i->second->last_used < lru->second->last_used) lru = i;
            lru->second->release_device();
            e->plans.erase(lru);
        }
    }
    auto pl = std::make_unique<Plan>();
    int rc = plan_and_upload(e, *c, W, H, p, pl.get(), split, thresholds_for(*e, small), n_frames, one_pass);
    if (rc) {
        pl->release_device();
        return rc;
    }
    pl->last_used = ++e->plan_tick;
    *out = pl.get();
    e->plans[key] = std::move(pl);
    return VJ_OK;
}

int Lane::create() {
    for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
    for (auto& x : pass_ev) HIP_TRY(hipEventCreate(&x));
    for (auto& x : launch_ev) HIP_TRY(hipEventCreate(&x));
    HIP_TRY(hipEventCreateWithFlags(&upload_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&integral_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    h_pinned_bytes = (size_t)1 << 20;   // counters block (~100 KiB) + the first detections
    HIP_TRY(hipHostMalloc(&h_pinned, h_pinned_bytes, hipHostMallocDefault));
    return VJ_OK;
}

void Lane::destroy() {
    for (DevBuf* b : {&d_gray, &d_counts, &d_det, &d_eq_frames, &d_eq_hist, &d_eq_lut, &d_eq_gray}) b->release();
    if (h_pinned) (void)hipHostFree(h_pinned);
    if (h_stage) (void)hipHostFree(h_stage);
    h_pinned = h_stage = nullptr;
    for (auto& x : ev) if (x) (void)hipEventDestroy(x);
    for (auto& x : pass_ev) if (x) (void)hipEventDestroy(x);
    for (auto& x : launch_ev) if (x) (void)hipEventDestroy(x);
    for (hipEvent_t* x : {&upload_done, &integral_done, &done}) if (*x) (void)hipEventDestroy(*x);
}

int ensure_image_buffers(vj_env* e, int W, int H, int frames, bool need_gray, int channels, Lane* lane) {
    if (!lane) lane = &e->lane0;
    const size_t fe = frame_elems_for(W, H);
    const uint32_t n_bands = ((uint32_t)H + BAND_ROWS - 1) / BAND_ROWS;
    const uint32_t band_pitch = ((uint32_t)W + 3u) & ~3u;
    int rc;
    const size_t sum_bytes = fe * 4 * (size_t)frames, sq_bytes = fe * 8 * (size_t)frames;
    const bool grow = sum_bytes > e->d_sum.cap || sq_bytes > e->d_sqsum.cap;
    if ((rc = e->d_sum.ensure(sum_bytes))) return rc;
    if ((rc = e->d_sqsum.ensure(sq_bytes))) return rc;
    (void)grow;
    if (need_gray) {
        const size_t gstride = align4((size_t)W * (size_t)channels);
        if ((rc = lane->d_gray.ensure(gstride * (size_t)H * (size_t)frames))) return rc;
    }
    const size_t band_elems = (size_t)frames * n_bands * band_pitch;
    if ((rc = e->d_band_sum.ensure(band_elems * 4))) return rc;
    if ((rc = e->d_band_sq.ensure(band_elems * 4))) return rc;
    if ((rc = e->d_band_sqp.ensure(band_elems * 8))) return rc;
    return VJ_OK;
}

// Enqueue the three integral kernels for `frames` frames already on the device.
int enqueue_integral(vj_env* e, const uint8_t* d_gray, size_t frame_bytes, int stride, int W, int H, int frames,
                     int channels, bool sq_u32) {
    IntegralArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.channels = (uint32_t)channels;
    ia.gray = d_gray;
    ia.gray_frame_bytes = frame_bytes;
    ia.gray_stride = (uint32_t)stride;
    ia.width = (uint32_t)W;
    ia.height = (uint32_t)H;
    ia.n_frames = (uint32_t)frames;
    ia.n_bands = ((uint32_t)H + BAND_ROWS - 1) / BAND_ROWS;
    ia.band_pitch = ((uint32_t)W + 3u) & ~3u;
    ia.band_sum = (uint32_t*)e->d_band_sum.p;
    ia.band_sq = (uint32_t*)e->d_band_sq.p;
    ia.band_sq_prefix = (uint64_t*)e->d_band_sqp.p;
    ia.sum = (uint32_t*)e->d_sum.p;
    ia.sqsum = (uint64_t*)e->d_sqsum.p;
    ia.frame_elems = frame_elems_for(W, H);
    ia.rows_mode = (uint32_t)e->integral_rows_mode;
    ia.sq_u32 = sq_u32 ? 1u : 0u;   // (u32 elements: frame f at element f * frame_elems of the same buffer, its first half)
    // the slack rows after row H (and the alignment tail) must read as zero
    // (the kernels never write there, so once per buffer layout is enough)
    const size_t used = (size_t)(W + 1) * (size_t)(H + 1);
    const bool zeroed = e->slack_w == W && e->slack_h == H && e->slack_frames >= frames && e->slack_sum == e->d_sum.p &&
                        e->slack_sq == e->d_sqsum.p && e->slack_sq_u32 == sq_u32;
    const size_t sq_elem = sq_u32 ? 4 : 8;
    for (int f = 0; f < frames && !zeroed; ++f) {
        HIP_TRY(hipMemsetAsync((uint32_t*)e->d_sum.p + (size_t)f * ia.frame_elems + used, 0,
                               (ia.frame_elems - used) * 4, e->stream));
        HIP_TRY(hipMemsetAsync((char*)e->d_sqsum.p + ((size_t)f * ia.frame_elems + used) * sq_elem, 0,
                               (ia.frame_elems - used) * sq_elem, e->stream));
    }
    if (!zeroed) {
        e->slack_w = W;
        e->slack_h = H;
        e->slack_frames = frames;
        e->slack_sum = e->d_sum.p;
        e->slack_sq = e->d_sqsum.p;
        e->slack_sq_u32 = sq_u32;
    }
    int hrc = launch_integral(ia, e->stream);
    if (hrc) {
        set_error("integral launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    return VJ_OK;
}

// The tilted integral of `frames` frames already on the device, into e->d_tilted (same geometry as d_sum).
int enqueue_tilted(vj_env* e, const uint8_t* d_gray, size_t frame_bytes, int stride, int W, int H, int frames, int channels) {
    const uint32_t fe = frame_elems_for(W, H);
    int rc;
    if ((rc = e->d_tilted.ensure((size_t)fe * 4u * (size_t)frames))) return rc;
    // rows past H (the slack rows) must read as zero, like d_sum's
    HIP_TRY(hipMemsetAsync(e->d_tilted.p, 0, (size_t)fe * 4u * (size_t)frames, e->stream));
    TiltedArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.gray = d_gray;
    ta.gray_frame_bytes = frame_bytes;
    ta.gray_stride = (uint32_t)stride;
    ta.channels = (uint32_t)channels;
    ta.width = (uint32_t)W;
    ta.height = (uint32_t)H;
    ta.n_frames = (uint32_t)frames;
    ta.frame_elems = fe;
    ta.tilted = (uint32_t*)e->d_tilted.p;
    const size_t n_bands = ((size_t)H + 7u) / 8u;
    if ((rc = e->d_tilt_diag.ensure((size_t)frames * n_bands * 2u * (size_t)(W + H) * 4u))) return rc;
    if ((rc = e->d_tilt_col.ensure((size_t)frames * n_bands * (size_t)(W + 1) * 4u))) return rc;
    const int hrc = launch_tilted_bands(ta, (uint32_t*)e->d_tilt_diag.p, (uint32_t*)e->d_tilt_col.p, e->stream);
    if (hrc) {
        set_error("tilted integral launch failed (width %d): %s", W, hipGetErrorString((hipError_t)hrc));
        return hrc == (int)hipErrorInvalidValue ? VJ_ERR_LIMIT : VJ_ERR_HIP;
    }
    return VJ_OK;
}

// Upload host frames (or gather strided device frames) into d_gray with a 4-byte
// aligned pitch.  Returns the device pointer / pitch the integral kernels should use.
int image_channels(const vj_image& im) { return im.channels <= 1 ? 1 : im.channels; }

int stage_reserve(Lane* lane, size_t bytes) {
    if (lane->h_stage_bytes >= bytes) return VJ_OK;
    if (lane->h_stage) (void)hipHostFree(lane->h_stage);
    lane->h_stage = nullptr;
    lane->h_stage_bytes = 0;
    HIP_TRY(hipHostMalloc(&lane->h_stage, bytes, hipHostMallocDefault));
    lane->h_stage_bytes = bytes;
    return VJ_OK;
}

int stage_frames(vj_env* e, const vj_image* frames, int n, int W, int H, const uint8_t** d_ptr, size_t* frame_bytes,
                 int* stride, Lane* lane, hipStream_t copy_stream) {
    if (!lane) lane = &e->lane0;
    hipStream_t cs = copy_stream ? copy_stream : e->stream;
    const size_t row_bytes = (size_t)W * (size_t)image_channels(frames[0]);
    bool all_dev = true, contiguous = true;
    for (int i = 0; i < n; ++i) {
        if (!frames[i].on_device) all_dev = false;
        if (i > 0 && (frames[i].stride != frames[0].stride ||
                      frames[i].data != frames[0].data + (size_t)i * (size_t)frames[0].stride * (size_t)H))
            contiguous = false;
    }
    if (all_dev && contiguous) {  // use the caller's device batch in place
        *d_ptr = frames[0].data;
        *stride = frames[0].stride;
        *frame_bytes = (size_t)frames[0].stride * (size_t)H;
        return VJ_OK;
    }
    const size_t gstride = align4(row_bytes);
    bool all_host = true;
    for (int i = 0; i < n; ++i) all_host = all_host && !frames[i].on_device;
    if (all_host && contiguous && (size_t)frames[0].stride == gstride && n > 1) {
        // a batch that is one block on the host with the device's pitch (a numpy array of n frames): ONE copy instead of n
        // (2048 frames of 100 x 100: 24 ms of per-frame copy calls)
        const size_t bytes = gstride * (size_t)H * (size_t)n;
        const void* src = frames[0].data;
        if (copy_stream) {   // streams: a true DMA — page-locked memory as it is, pageable memory through the staging buffer
            hipPointerAttribute_t at;
            const bool pinned = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost;
            if (!pinned) {
                (void)hipGetLastError();
                if (const int err = stage_reserve(lane, bytes)) return err;
                memcpy(lane->h_stage, src, bytes);
                src = lane->h_stage;
            }
        }
        HIP_TRY(hipMemcpyAsync(lane->d_gray.p, src, bytes, hipMemcpyHostToDevice, cs));
        *d_ptr = (const uint8_t*)lane->d_gray.p;
        *stride = (int)gstride;
        *frame_bytes = gstride * (size_t)H;
        return VJ_OK;
    }
    if (all_host && n >= 4 && gstride * (size_t)H <= ((size_t)256 << 10)) {
        // many small frames in separate host buffers: gather them in the page-locked staging buffer (at the device's pitch)
        // and send one block — a copy call per frame costs more than copying a few KB twice
        const size_t fb = gstride * (size_t)H, bytes = fb * (size_t)n;
        if (const int err = stage_reserve(lane, bytes)) return err;
        for (int i = 0; i < n; ++i) {
            uint8_t* st = (uint8_t*)lane->h_stage + (size_t)i * fb;
            if ((size_t)frames[i].stride == gstride) memcpy(st, frames[i].data, fb);
            else
                for (int y = 0; y < H; ++y) memcpy(st + (size_t)y * gstride, frames[i].data + (size_t)y * (size_t)frames[i].stride, row_bytes);
        }
        HIP_TRY(hipMemcpyAsync(lane->d_gray.p, lane->h_stage, bytes, hipMemcpyHostToDevice, cs));
        *d_ptr = (const uint8_t*)lane->d_gray.p;
        *stride = (int)gstride;
        *frame_bytes = fb;
        return VJ_OK;
    }
    for (int i = 0; i < n; ++i) {
        uint8_t* dst = (uint8_t*)lane->d_gray.p + (size_t)i * gstride * (size_t)H;
        const uint8_t* src = frames[i].data;
        size_t src_stride = (size_t)frames[i].stride;
        if (!frames[i].on_device && (copy_stream || src_stride != gstride)) {
            // streams: the copy must be a true DMA to overlap the kernels — page-locked memory (vj_host_alloc) goes as
            // it is, pageable memory through this lane's pinned staging buffer.  Blocking calls: a pageable frame whose
            // row stride is not the device pitch (a width that is not a multiple of 4) would be a 2-D copy from pageable
            // memory, which the runtime does row by row (1921 x 1081: 7.5 ms instead of 0.2): re-pitch it in the
            // staging buffer and send it as one block
            hipPointerAttribute_t at;
            const bool pinned = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost;
            if (!pinned) {
                (void)hipGetLastError();
                const size_t need = gstride * (size_t)H * (size_t)n;
                if (const int err = stage_reserve(lane, need)) return err;
                uint8_t* st = (uint8_t*)lane->h_stage + (size_t)i * gstride * (size_t)H;
                for (int y = 0; y < H; ++y) memcpy(st + (size_t)y * gstride, src + (size_t)y * src_stride, row_bytes);
                src = st;
                src_stride = gstride;
            }
        }
        HIP_TRY(hipMemcpy2DAsync(dst, gstride, src, src_stride, row_bytes, (size_t)H,
                                 frames[i].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cs));
    }
    *d_ptr = (const uint8_t*)lane->d_gray.p;
    *stride = (int)gstride;
    *frame_bytes = gstride * (size_t)H;
    return VJ_OK;
}

int refuse_equalize(uint32_t flags, const char* entry_point) {
    if ((flags & VJ_FLAG_EQUALIZE_HIST) == 0u) return VJ_OK;
    set_error("%s does not take VJ_FLAG_EQUALIZE_HIST: equalize the frames with vj_equalize_hist first", entry_point);
    return VJ_ERR_UNSUPPORTED;
}

int enqueue_equalize_tables(vj_env* e, Lane* lane, const void* d_frame_recs, uint32_t n_frames, uint32_t n_hist_units, const uint8_t** lut) {
    int rc;
    if ((rc = lane->d_eq_hist.ensure((size_t)n_frames * 256u * sizeof(uint32_t)))) return rc;
    if ((rc = lane->d_eq_lut.ensure((size_t)n_frames * 256u))) return rc;
    HIP_TRY(hipMemsetAsync(lane->d_eq_hist.p, 0, (size_t)n_frames * 256u * sizeof(uint32_t), e->stream));
    EqualizeArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const AtlasFrameDev*)d_frame_recs;
    a.n_frames = n_frames;
    a.n_hist_units = n_hist_units;
    a.hist = (uint32_t*)lane->d_eq_hist.p;
    a.lut = (uint8_t*)lane->d_eq_lut.p;
    int hrc = launch_equalize_hist(a, e->stream);
    if (!hrc) hrc = launch_equalize_lut(a, e->stream);
    if (hrc) {
        set_error("equalization launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    *lut = (const uint8_t*)lane->d_eq_lut.p;
    return VJ_OK;
}

int enqueue_equalize(vj_env* e, Lane* lane, const uint8_t** d_gray, size_t* frame_bytes, int* stride, int* channels, int W, int H, int frames) {
    if (!lane) lane = &e->lane0;
    int rc;
    const uint32_t pitch = ((uint32_t)W + 3u) & ~3u;
    const uint64_t units_per_frame = (uint64_t)(((uint32_t)W + ATLAS_BLOCK_W - 1u) / ATLAS_BLOCK_W) * (((uint32_t)H + ATLAS_BLOCK_H - 1u) / ATLAS_BLOCK_H);
    if (units_per_frame * (uint64_t)frames > 0x7fffffffull) {
        set_error("VJ_FLAG_EQUALIZE_HIST: a sub-batch of %d frames holds more work units than a 32-bit index holds", frames);
        return VJ_ERR_LIMIT;
    }
    std::vector<AtlasFrameDev> recs((size_t)frames);
    for (int i = 0; i < frames; ++i)
        recs[(size_t)i] = AtlasFrameDev{*d_gray + (size_t)i * *frame_bytes, (uint32_t)*stride, (uint32_t)*channels, (uint32_t)W, (uint32_t)H, 0u, 0u,
                                        (uint32_t)(units_per_frame * (uint64_t)i), eq_hist_units((uint32_t)H) * (uint32_t)i};
    if ((rc = lane->d_eq_frames.ensure(recs.size() * sizeof(AtlasFrameDev)))) return rc;
    if ((rc = lane->d_eq_gray.ensure((size_t)pitch * (size_t)H * (size_t)frames))) return rc;
    // (pageable memory: the runtime has taken the records when the call returns)
    HIP_TRY(hipMemcpyAsync(lane->d_eq_frames.p, recs.data(), recs.size() * sizeof(AtlasFrameDev), hipMemcpyHostToDevice, e->stream));
    const uint8_t* lut;
    if ((rc = enqueue_equalize_tables(e, lane, lane->d_eq_frames.p, (uint32_t)frames, eq_hist_units((uint32_t)H) * (uint32_t)frames, &lut))) return rc;
    EqualizeArgs a;
    memset(&a, 0, sizeof(a));
    a.frames = (const AtlasFrameDev*)lane->d_eq_frames.p;
    a.n_frames = (uint32_t)frames;
    a.n_units = (uint32_t)(units_per_frame * (uint64_t)frames);
    a.lut = (uint8_t*)lane->d_eq_lut.p;
    a.dst = (uint8_t*)lane->d_eq_gray.p;
    a.dst_pitch = pitch;
    a.dst_h = (uint32_t)H;
    a.dst_frame_bytes = (uint64_t)pitch * (uint64_t)H;
    const int hrc = launch_equalize_apply(a, e->stream);
    if (hrc) {
        set_error("equalization launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    *d_gray = (const uint8_t*)lane->d_eq_gray.p;
    *frame_bytes = (size_t)pitch * (size_t)H;
    *stride = (int)pitch;
    *channels = 1;
    return VJ_OK;
}

struct RawDet {
    int frame;
    uint32_t slot, x, y;
};

// Where the counters of one batch live: [MAX_PASSES][MAX_SCALES][Q_PARTS] queue counts | det_count | pad | one
// stage_entered[VJ_MAX_STAGES] (u64) array per kernel launch (array 0 is spare) | the counters of a region-of-interest
// pass (vj_detect_chain): regions, units, invalid regions, unit ticket, detections, pad | its stage_entered array | the queue
// counts of the tiles' own queue set (stage trees, enqueue_cascade).
struct CountsLayout {
    static constexpr size_t q_counts = (size_t)MAX_SCALES * Q_PARTS;   // counters of one queue: [scale][part]
    static constexpr size_t stage_off_u32 = MAX_PASSES * q_counts + 2;
    static constexpr size_t roi_off_u32 = stage_off_u32 + (size_t)(1 + VJ_MAX_LAUNCHES) * VJ_MAX_STAGES * 2;
    static constexpr size_t q2_off_u32 = roi_off_u32 + 8 + (size_t)VJ_MAX_STAGES * 2;   // second set of queue counters (stage trees)
    static constexpr size_t bytes = (q2_off_u32 + MAX_PASSES * q_counts) * sizeof(uint32_t);
    // Queue 0 does not exist, so its q_counts counters serve as tickets, zeroed with the block once per enqueue_cascade.  From
    // the front: pass ps draws from [ps * Q_PARTS, (ps + 1) * Q_PARTS) — pass 0 is the grid pass, whose GRID_PARTS parts of the
    // (frame, unit) list take the first range (one grid launch per zeroing); from the back: tile class c at
    // q_counts - 8 (c + 1), the region pass's tiles at q_counts - 40.
    static constexpr size_t pass_tickets_end = (size_t)MAX_PASSES * Q_PARTS;
    static constexpr size_t tile_tickets_begin = q_counts - 8u * TILE_CLASSES;
    static constexpr size_t roi_tickets_begin = q_counts - 40u;
};
static_assert(GRID_PARTS == Q_PARTS, "the grid pass's tickets are pass 0's range of queue 0's counters");
static_assert(CountsLayout::pass_tickets_end <= CountsLayout::roi_tickets_begin, "pass tickets (the grid pass's among them) end before the region pass's");
static_assert(CountsLayout::roi_tickets_begin + 8u <= CountsLayout::tile_tickets_begin, "the region pass's tile tickets end before the tile classes'");

// Upload (or adopt) the frames of one batch and enqueue its integral images.  `copy_stream` != null: the upload runs
// on that stream and the integral waits for it (vj_stream); else everything is ordered on the environment's stream.
static int enqueue_prepare(vj_env* e, Lane* L, Plan* pl, const vj_image* frames, int nf, int W, int H, bool fixed_queue_layout,
                           hipStream_t copy_stream, bool equalize = false, bool sq_u32 = false) {
    int rc;
    int channels = image_channels(frames[0]);
    if ((rc = ensure_image_buffers(e, W, H, nf, true, channels, L))) return rc;
    uint64_t q_entries = 0;
    if (!fixed_queue_layout) {
        if ((rc = layout_queues(pl, nf, &q_entries))) return rc;
        const size_t n_pass = pl->pass_bounds.size() - 1;
        for (size_t ps = 1; ps < n_pass; ++ps)
            if ((rc = e->d_q[ps].ensure(std::max<uint64_t>(q_entries, 1) * sizeof(QEntry)))) return rc;
    }
    if ((rc = L->d_counts.ensure(CountsLayout::bytes))) return rc;
    if (L->det_cap == 0) {
        L->det_cap = e->det_cap_init;
        if ((rc = L->d_det.ensure((size_t)L->det_cap * sizeof(DetEntry)))) return rc;
    }
    const uint8_t* d_gray;
    size_t gray_frame_bytes;
    int gray_stride;
    if ((rc = stage_frames(e, frames, nf, W, H, &d_gray, &gray_frame_bytes, &gray_stride, L, copy_stream))) return rc;
    if (copy_stream) {
        HIP_TRY(hipEventRecord(L->upload_done, copy_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, L->upload_done, 0));
    }
    HIP_TRY(hipEventRecord(L->ev[0], e->stream));
    // VJ_FLAG_EQUALIZE_HIST: from here on the batch is the lane's equalized gray frames (a redo integrates those again)
    if (equalize && (rc = enqueue_equalize(e, L, &d_gray, &gray_frame_bytes, &gray_stride, &channels, W, H, nf))) return rc;
    L->src_gray = d_gray;
    L->src_frame_bytes = gray_frame_bytes;
    L->src_stride = gray_stride;
    L->src_channels = channels;
    // (a variance rectangle wider than SQ32_MAX_AREA pixels has no strip height: such frames keep the u64 layout)
    L->sq_u32 = sq_u32 && e->sq32 && e->sq_u32 && (uint32_t)W <= SQ32_MAX_AREA;
    if ((rc = enqueue_integral(e, d_gray, gray_frame_bytes, gray_stride, W, H, nf, channels, L->sq_u32))) return rc;
    HIP_TRY(hipEventRecord(L->ev[1], e->stream));
    HIP_TRY(hipEventRecord(L->integral_done, e->stream));   // the lane's frame buffer may be overwritten from here on
    L->nf = nf;
    return VJ_OK;
}

// Enqueue every cascade launch of the batch whose integral images are (being) computed, then the asynchronous
// read-back of its counters and first detections.  Nothing here waits for the device.
static int enqueue_cascade(vj_env* e, Lane* L, Plan* pl, int W, int /*H*/, const vj_params& p) {
    int rc;
    const int nf = L->nf;
    const size_t n_pass = pl->pass_bounds.size() - 1;
    const size_t counts_bytes = CountsLayout::bytes;
    constexpr size_t q_counts = CountsLayout::q_counts;
    uint32_t* d_qcount[MAX_PASSES];
    for (int ps = 0; ps < MAX_PASSES; ++ps) d_qcount[ps] = (uint32_t*)L->d_counts.p + ps * q_counts;
    uint32_t* d_qcount2[MAX_PASSES];   // the tiles' own queue set (stage trees: see split_sets below)
    for (int ps = 0; ps < MAX_PASSES; ++ps) d_qcount2[ps] = (uint32_t*)L->d_counts.p + CountsLayout::q2_off_u32 + ps * q_counts;
    uint32_t* d_det_count = (uint32_t*)L->d_counts.p + MAX_PASSES * q_counts;
    unsigned long long* d_stage_entered = (unsigned long long*)((uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32);
    const bool count = (p.flags & VJ_FLAG_COUNTERS) != 0;
    const int n_blocks = std::max(1, e->n_cu * e->blocks_per_cu);
    {
        HIP_TRY(hipMemsetAsync(L->d_counts.p, 0, counts_bytes, e->stream));
        HIP_TRY(hipEventRecord(L->ev[2], e->stream));
        CascadeArgs ca;
        memset(&ca, 0, sizeof(ca));
        ca.sum = (const uint32_t*)e->d_sum.p;
        ca.sqsum = (const uint64_t*)e->d_sqsum.p;
        ca.sq_u32 = L->sq_u32 ? 1u : 0u;
        ca.table = (const uint32_t*)pl->d_table.p;
        ca.scales = (const ScaleDev*)pl->d_scales.p;
        ca.stages = (const StageDev*)pl->d_stages.p;
        ca.units = (const UnitDev*)pl->d_units.p;
        ca.n_units = (uint32_t)pl->units.size();
        ca.tile_units = (const UnitDev*)pl->d_tile_units.p;
        ca.n_tile_units = (uint32_t)pl->tile_units.size();
        ca.n_frames = (uint32_t)nf;
        ca.n_scales = (uint32_t)pl->scales.size();
        ca.frame_elems = pl->frame_elems;
        ca.sum_bytes = (uint32_t)((uint64_t)pl->frame_elems * 4u * (uint64_t)nf);
        ca.stride = (uint32_t)W + 1u;
        // waves per workgroup of the gather chain: four for batches, three for single frames and for stage trees (their
        // workgroups carry a second LDS array); the launchers clamp, the kernels read blockDim.  The waves of a linear launch
        // divide one 16 KiB array (vj_gather_queue.hpp), and the plan's units must fit a wave's share: a plan cut for fewer
        // waves than this call would run (a stream's plan, a sub-batch) keeps the call at the waves it was cut for
        ca.gather_waves = gather_waves_fitting((uint32_t)e->gather_waves_for(nf, pl->general, pl->trees), pl->unit_cap);
        ca.q_cap = pl->general ? (uint32_t)UNIT_WINDOWS : gather_queue_cap(ca.gather_waves);
        ca.total_waves = (uint32_t)n_blocks * ca.gather_waves;
        ca.det = (DetEntry*)L->d_det.p;
        ca.det_count = d_det_count;
        ca.det_cap = L->det_cap;
        ca.signed_mean = (p.flags & VJ_FLAG_SIGNED_MEAN) ? 1u : 0u;
        ca.stage_entered = d_stage_entered;
        ca.tree_ctr = d_stage_entered;       // array 0 is spare: [0], [1] = the first cascade's visited child nodes / their rectangles
        ca.n_pass = (uint32_t)n_pass;
        for (size_t ps = 0; ps <= n_pass; ++ps) ca.pass_begin[ps] = pl->pass_bounds[ps];
        for (size_t ps = 1; ps < n_pass; ++ps) {
            ca.q_pass[ps] = (QEntry*)e->d_q[ps].p;
            ca.q_pass_count[ps] = d_qcount[ps];
        }
        // linear cascades: the kernel sees the configured tile_end, not the plan's clamped pl->tile_end; a tile leaves at the first pass boundary
        // at or beyond it, and `banded` / `handover` below compare it with pass_bounds[1]
        ca.tile_end = pl->general ? pl->general_prefix : (uint32_t)e->tile_end;   // stage trees: tiles run the linear prefix only
        ca.tile_min_lanes = (uint32_t)e->tile_min_lanes;
        ca.tile_repack_mask = e->tile_repack_mask;
        ca.tile_sp_begin = (!pl->general && (pl->wave_tail || pl->tree2)) ? (uint32_t)e->tile_sp_begin : 0xffffffffu;   // the finishes walk positions linearly: never on a stage tree
        ca.tree2 = pl->tree2 ? 1u : 0u;
        ca.identity_order = pl->general ? 0u : 1u;
        ca.n_seg = e->tile_segments ? pl->tile_n_seg : 0u;
        for (int k = 0; k < 4; ++k) ca.seg_end[k] = pl->tile_seg_end[k];
        ca.seg_chain = pl->tile_seg_chain;
        ca.sp_blocks = (const SpBlock*)pl->d_sp_blocks.p;
        ca.n_sp_blocks = pl->n_sp_blocks;
        ca.tile_ws_min = pl->wave_tail ? (uint32_t)e->tile_ws_min : 0u;   // no wave-independent tail: wave-split to the end
        ca.tile_ws_max = (uint32_t)std::min(e->tile_ws_max, (int)TILE_WS_MAX_WINDOWS);
        ca.pos_mode = pl->pos_mode;
        ca.pos_tab = (const uint32_t*)pl->d_pos_tab.p;
        ca.gather_pairs = e->pairs_for(nf);
        ca.sp_tail_max = (uint32_t)std::max(0, std::min(e->sp_tail_max, (int)gather_tail_max(ca.q_cap)));
        ca.max_stage_nodes = pl->max_stage_nodes;
        if (pl->skip_mode && pl->n_skip_units) {
            // the windows the reference's sequential CPU loop visits, as a bitmap: stage-0 verdict of every grid window,
            // then the parity recurrence; the passes below drop the unvisited windows while they enumerate the grid
            if ((rc = e->d_skip_bits.ensure((size_t)pl->skip_frame_words * 8u * (size_t)nf))) return rc;
            ca.skip_bits = (unsigned long long*)e->d_skip_bits.p;
            ca.skip_frame_words = pl->skip_frame_words;
            ca.skip_units = (const UnitDev*)pl->d_skip_units.p;
            ca.n_skip_units = pl->n_skip_units;
            ca.skip_segs = (const UnitDev*)pl->d_skip_segs.p;
            ca.n_skip_segs = pl->n_skip_segs;
            const int hrc = launch_skip_bitmap(ca, pl->trees, std::max(1, e->n_cu * 4), e->stream);
            if (hrc) {
                set_error("skip bitmap launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return VJ_ERR_HIP;
            }
        }
        int launches = 0;
        std::vector<vj_launch>& linfo = L->linfo;
        linfo.clear();
        // every launch is bracketed by its own pair of events on the stream it runs on
        auto begin_launch = [&](int kind, int cls, uint32_t sb, uint32_t se, uint32_t lds, hipStream_t st) -> int {
            if (linfo.size() < VJ_MAX_LAUNCHES) HIP_TRY(hipEventRecord(L->launch_ev[2 * linfo.size()], st));
            vj_launch li;
            memset(&li, 0, sizeof(li));
            li.kind = kind;
            li.lds_class = cls;
            li.stage_begin = (int32_t)sb;
            li.stage_end = (int32_t)se;
            li.lds_bytes = lds;
            for (uint32_t slot = 0; slot < pl->scales.size(); ++slot) {
                const ScaleDev& sd = pl->scales[slot];
                const bool in = kind == VJ_LAUNCH_QUEUE ||
                                (kind == VJ_LAUNCH_TILE && sd.tile_rw && sd.tile_row_end > 0 && (int)pl->scales[pl->tile_lead[slot]].tile_class == cls) ||
                                (kind == VJ_LAUNCH_GRID && sd.tile_row_end < sd.ny);
                if (in && sd.scale_idx < 128) li.scale_mask[sd.scale_idx >> 6] |= 1ull << (sd.scale_idx & 63);
            }
            linfo.push_back(li);
            return VJ_OK;
        };
        // the launch just begun counts into its own array
        auto launch_counters = [&]() -> unsigned long long* {
            return d_stage_entered + std::min<size_t>(linfo.size(), VJ_MAX_LAUNCHES) * VJ_MAX_STAGES;
        };
        auto end_launch = [&](hipStream_t st) -> int {
            if (linfo.size() <= VJ_MAX_LAUNCHES) HIP_TRY(hipEventRecord(L->launch_ev[2 * linfo.size() - 1], st));
            return VJ_OK;
        };
        auto pass_is_last = [&](size_t ps) { return pl->seg_last.empty() ? ps + 1 == n_pass : pl->seg_last[ps] != 0; };
        const bool general_kernel = pl->general && pl->seg_last.empty();   // run_stages_general finishes the tree
        // Band-major queue pass: a batch of a linear cascade whose gather chain is grid pass + ONE queue pass that only the grid
        // pass feeds.  It reads nothing but the runs the grid pass records in run_table, so the tiles must not feed that queue:
        // they run the whole cascade themselves only when tile_end lies BEYOND the boundary (at tile_end == pass_bounds[1] they
        // hand their survivors to q_pass[1], and the chunked pass, which sweeps the whole sub-queue, takes the batch)
        const bool banded = e->q_band_px > 0 && !pl->unit_groups.empty() && !pl->general && n_pass == 2 && nf >= e->q_band_min_frames &&
                            e->tile_min_lanes == 0 && (uint32_t)e->tile_end > pl->pass_bounds[1];
        if (banded) {
            if ((rc = e->d_run_table.ensure((size_t)nf * pl->units.size() * 8u))) return rc;
            ca.run_table = (uint32_t*)e->d_run_table.p;
        }
        auto queue_args = [&](size_t ps, int set = 0) {
            CascadeArgs qa = ca;
            DevBuf* dq = set ? e->d_q2 : e->d_q;
            uint32_t** qc = set ? d_qcount2 : d_qcount;
            qa.stage_begin = pl->pass_bounds[ps];
            qa.stage_end = pl->pass_bounds[ps + 1];
            const bool last = pass_is_last(ps);
            // pass ps reads queue ps (filled by pass ps-1 and by tiles that left at this boundary)
            // and appends its survivors to queue ps+1
            qa.q_in = (const QEntry*)dq[ps].p;
            qa.q_in_count = qc[ps];
            qa.q_ticket = qc[0] + ps * Q_PARTS;   // queue 0 does not exist: its counters serve as tickets
            // frame-major order inside a part: one slice per frame of the part's frame group (-1), or as configured
            qa.q_slices = e->q_slices >= 0 ? (uint32_t)std::max(1, e->q_slices)
                                           : (uint32_t)std::max(1, std::min(16, (nf + (int)Q_PARTS - 1) / (int)Q_PARTS));
            qa.min_chunk = (uint32_t)e->min_chunk;
            qa.wide_tail = (e->wide_tail < 0 ? nf <= 4 : e->wide_tail != 0) ? 1u : 0u;
            qa.q_out = last ? nullptr : (QEntry*)dq[ps + 1].p;
            qa.q_out_count = last ? nullptr : qc[ps + 1];
            if (banded && ps == 1) {
                qa.q_groups = (const UnitDev*)pl->d_unit_groups.p;
                qa.n_q_groups = (uint32_t)pl->unit_groups.size();
            }
            if (!pl->seg_fail.empty() && pl->seg_fail[ps] != 0) {   // stage tree: this segment's rejects continue
                qa.q_fail = (QEntry*)dq[pl->seg_fail[ps]].p;
                qa.q_fail_count = qc[pl->seg_fail[ps]];
            }
            return qa;
        };
        if (ca.n_units + ca.n_tile_units > 0) {
            int hrc = 0;
            // Two chains share the first part of the cascade and run CONCURRENTLY on two streams:
            //   A (e->stream) : the LDS-tile launches (LDS-bound)
            //   B (e->stream2): the global-gather first pass and the queue passes that only it feeds
            //                   (texture-address-bound) — every pass that begins before the stage at
            //                   which tiles hand over (tiles leave at one boundary when tile_min_lanes = 0)
            // then B joins A and the remaining queue passes run on A.
            const uint32_t handover = pl->general ? pl->general_prefix : std::max<uint32_t>(ca.tile_end, pl->pass_bounds[1]);
            size_t first_joint_pass = 1;
            if (e->tile_min_lanes == 0)
                while (first_joint_pass < n_pass && pl->pass_bounds[first_joint_pass] < handover) ++first_joint_pass;
            const bool two_streams = e->concurrent && ca.n_tile_units > 0 && ca.n_units > 0;
            // Stage tree in chains (seg_last): the chains' queue passes would have to wait for BOTH the grid pass and the
            // tiles, because a crowded tile hands its windows to the same queues — and the tiles take longer than the grid
            // pass (4096 x 4096: 7.8 vs 4.8 ms, then 7.8 ms of queue passes).  So the tiles get a queue set of their own:
            // the grid pass's survivors go down the tree on stream B while the tiles still run, and after the join the same
            // passes run once more on what the tiles left (usually little: thin passes).
            const bool split_sets = two_streams && pl->general && !pl->seg_last.empty() && e->tree_split_queues;
            if (split_sets) {
                for (size_t ps = 1; ps < n_pass; ++ps) {
                    if ((rc = e->d_q2[ps].ensure(e->d_q[ps].cap))) return rc;
                    ca.q_pass[ps] = (QEntry*)e->d_q2[ps].p;        // (the grid and queue passes take theirs from queue_args)
                    ca.q_pass_count[ps] = d_qcount2[ps];
                }
                first_joint_pass = n_pass;
            }
            hipStream_t sB = two_streams ? e->stream2 : e->stream;
            if (two_streams) {
                HIP_TRY(hipEventRecord(e->fork_ev, e->stream));
                HIP_TRY(hipStreamWaitEvent(e->stream2, e->fork_ev, 0));
            }
            HIP_TRY(hipEventRecord(L->pass_ev[0], e->stream));
            // chain A: tile launches
            auto chain_a = [&]() -> int {
            for (uint32_t ci = 0; ci < TILE_CLASSES && !hrc && ca.n_tile_units > 0; ++ci) {
                // largest LDS first: the one-workgroup-per-CU class suffers most from the gather chain, whose first pass is
                // the heavier one (measured: 48.3 -> 47.2 ms)
                const uint32_t cls = TILE_CLASSES - 1u - ci;
                const uint32_t n_cls = pl->class_first[cls + 1] - pl->class_first[cls];
                if (!n_cls) continue;
                CascadeArgs ta = ca;
                ta.tile_units = (const UnitDev*)pl->d_tile_units.p + pl->class_first[cls];
                ta.n_tile_units = n_cls;
                ta.tile_lds_bytes = pl->class_lds[cls];
                ta.tile_ticket = d_qcount[0] + (q_counts - 8u * (cls + 1u));   // queue 0 does not exist: its counters are free
                // workgroups per CU: what the LDS allows (160 KiB per CU), at most 4 x 8 waves
                const int per_cu = std::max(1, std::min(32 / TILE_WAVES, (int)(160u * 1024u / ta.tile_lds_bytes)));
                const int tb = (int)std::min<uint64_t>((uint64_t)n_cls * (uint64_t)nf, (uint64_t)e->n_cu * (uint64_t)per_cu);
                const uint32_t deepest = std::min<uint32_t>((uint32_t)pl->stages.size(), handover);
                if ((rc = begin_launch(VJ_LAUNCH_TILE, (int)cls, 0, deepest, ta.tile_lds_bytes, e->stream))) return rc;
                ta.stage_entered = launch_counters();
                hrc = launch_cascade_tile_pass(ta, pl->trees, count, std::max(1, tb), e->stream);
                if ((rc = end_launch(e->stream))) return rc;
            }
                return VJ_OK;
            };
            // chain B: grid pass, then the queue passes fed by it alone.  When the chains overlap it goes
            // first, with one small workgroup per CU (the texture-address unit it is bound by saturates at
            // one wave per SIMD), so that the tile workgroups find their LDS share next to it.
            const int b_blocks = two_streams ? std::max(1, e->n_cu * e->concurrent_blocks_per_cu) : n_blocks;
            auto chain_b = [&]() -> int {
            if (!hrc && ca.n_units > 0) {
                CascadeArgs ga = queue_args(0);   // (q_ticket: pass 0's range — the tickets of the unit list's parts)
                if ((rc = begin_launch(VJ_LAUNCH_GRID, 0, ga.stage_begin, ga.stage_end, 0, sB))) return rc;
                ga.stage_entered = launch_counters();
                hrc = launch_cascade_pass(ga, true, pl->trees, n_pass == 1, count, general_kernel && n_pass == 1, b_blocks, sB);
                if ((rc = end_launch(sB))) return rc;
                for (size_t ps = 1; ps < first_joint_pass && !hrc; ++ps) {
                    CascadeArgs qa = queue_args(ps);
                    // (next to the tiles one workgroup per CU; a stage tree's chains are latency-bound: all of them)
                    const int qb = split_sets ? n_blocks : b_blocks;
                    qa.total_waves = (uint32_t)qb * qa.gather_waves;
                    if ((rc = begin_launch(VJ_LAUNCH_QUEUE, 0, qa.stage_begin, qa.stage_end, 0, sB))) return rc;
                    qa.stage_entered = launch_counters();
                    hrc = launch_cascade_pass(qa, false, pl->trees, pass_is_last(ps), count, false, qb, sB);
                    if ((rc = end_launch(sB))) return rc;
                }
            } else {
                first_joint_pass = 1;
            }
                return VJ_OK;
            };
            if (two_streams) {
                if ((rc = chain_b())) return rc;
                if ((rc = chain_a())) return rc;
            } else {
                if ((rc = chain_a())) return rc;
                if ((rc = chain_b())) return rc;
            }
            if (two_streams) {
                HIP_TRY(hipEventRecord(e->join_ev, e->stream2));
                HIP_TRY(hipStreamWaitEvent(e->stream, e->join_ev, 0));
            }
            for (size_t ps = 1; ps < n_pass && ps < VJ_MAX_PASSES && ps <= first_joint_pass; ++ps)
                HIP_TRY(hipEventRecord(L->pass_ev[ps], e->stream));
            // joint passes (split_sets: all of them once more, on the tiles' queue set)
            for (size_t ps = split_sets ? 1 : first_joint_pass; ps < n_pass && !hrc; ++ps) {
                if (ps > first_joint_pass && ps < VJ_MAX_PASSES) HIP_TRY(hipEventRecord(L->pass_ev[ps], e->stream));
                CascadeArgs qa = queue_args(ps, split_sets ? 1 : 0);
                if ((rc = begin_launch(VJ_LAUNCH_QUEUE, 0, qa.stage_begin, qa.stage_end, 0, e->stream))) return rc;
                qa.stage_entered = launch_counters();
                hrc = launch_cascade_pass(qa, false, pl->trees, pass_is_last(ps), count, general_kernel, n_blocks, e->stream);
                if ((rc = end_launch(e->stream))) return rc;
            }
            if (hrc) {
                set_error("cascade launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return VJ_ERR_HIP;
            }
            launches = (int)n_pass;
        }
        if (n_pass <= VJ_MAX_PASSES && launches) HIP_TRY(hipEventRecord(L->pass_ev[n_pass], e->stream));
        HIP_TRY(hipEventRecord(L->ev[3], e->stream));
        L->launches = launches;
    }
    L->n_pass = n_pass;
    L->count = count;
    // read back the counters block and the first detections (nearly always all of them)
    HIP_TRY(hipMemcpyAsync(L->h_pinned, L->d_counts.p, counts_bytes, hipMemcpyDeviceToHost, e->stream));
    const size_t room = (L->h_pinned_bytes - ((counts_bytes + 255) & ~(size_t)255)) / sizeof(DetEntry);
    L->det_copied = (uint32_t)std::min<size_t>(room, L->det_cap);
    HIP_TRY(hipMemcpyAsync((char*)L->h_pinned + ((counts_bytes + 255) & ~(size_t)255), L->d_det.p, (size_t)L->det_copied * sizeof(DetEntry),
                           hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipEventRecord(L->done, e->stream));
    L->pending = true;
    return VJ_OK;
}

// Wait for the batch on lane L and decode it: detections appended to `dets` with frame numbers offset by f0.  When the
// detection buffer overflowed it is grown and the cascade passes run again — on the integral images still in place for a
// blocking call, after recomputing them from the lane's frames for a stream lane (the two lanes of a vj_stream share
// the environment's integral images, and the next batch's have replaced this one's by now).  The redo is ordered on the
// environment's stream behind everything already queued, and finished synchronously here.
static int finish_batch(vj_env* e, Lane* L, Plan* pl, int f0, int W, int H, const vj_params& p, std::vector<RawDet>* dets,
                        vj_counters* ctr, vj_timing* tm, std::vector<DetEntry>* raw_out = nullptr) {
    int rc;
    constexpr size_t q_counts = CountsLayout::q_counts;
    const size_t counts_bytes = CountsLayout::bytes;
    for (int attempt = 0; attempt < 3; ++attempt) {
        HIP_TRY(hipEventSynchronize(L->done));
        L->pending = false;
        const size_t n_pass = L->n_pass;
        const int launches = L->launches;
        const bool count = L->count;
        const std::vector<vj_launch>& linfo = L->linfo;
        const uint32_t n_det = ((const uint32_t*)L->h_pinned)[MAX_PASSES * q_counts];
        float ms_i = 0, ms_c = 0, ms_t = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, L->ev[0], L->ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_c, L->ev[2], L->ev[3]));
        HIP_TRY(hipEventElapsedTime(&ms_t, L->ev[0], L->ev[3]));
        if (n_det > L->det_cap) {  // detections overflowed: grow and redo the cascade passes
            const uint32_t want = grown_cap(L->det_cap, n_det);
            if ((rc = L->d_det.ensure((size_t)want * sizeof(DetEntry)))) return rc;
            L->det_cap = want;
            if (L->shared_integrals) {
                HIP_TRY(hipEventRecord(L->ev[0], e->stream));
                if ((rc = enqueue_integral(e, L->src_gray, L->src_frame_bytes, L->src_stride, W, H, L->nf, L->src_channels, L->sq_u32))) return rc;
                HIP_TRY(hipEventRecord(L->ev[1], e->stream));
            }
            if ((rc = enqueue_cascade(e, L, pl, W, H, p))) return rc;
            continue;
        }
        if (attempt == 0) tm->integral_ms += ms_i;
        tm->cascade_ms += ms_c;
        tm->total_ms += ms_t;
        if (launches && n_pass <= VJ_MAX_PASSES)
            for (size_t ps = 0; ps < n_pass; ++ps) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, L->pass_ev[ps], L->pass_ev[ps + 1]));
                tm->pass_ms[ps] += ms;
                tm->pass_stage_begin[ps] = (int32_t)pl->pass_bounds[ps];
                tm->pass_stage_end[ps] = (int32_t)pl->pass_bounds[ps + 1];
            }
        tm->n_cascade_launches = std::max(tm->n_cascade_launches, launches);
        const unsigned long long* se_all = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::stage_off_u32);
        if (linfo.size() <= VJ_MAX_LAUNCHES) {
            for (size_t i = 0; i < linfo.size(); ++i) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, L->launch_ev[2 * i], L->launch_ev[2 * i + 1]));
                vj_launch acc = tm->launch[i];   // sums over sub-batches: time and counters
                tm->launch[i] = linfo[i];
                tm->launch[i].ms = acc.ms + ms;
                const unsigned long long* se = se_all + (1 + i) * VJ_MAX_STAGES;
                for (size_t s = 0; s < (size_t)VJ_MAX_STAGES; ++s)
                    tm->launch[i].stage_entered[s] = acc.stage_entered[s] + (count ? se[s] : 0ull);
            }
            tm->n_launches = (int32_t)linfo.size();
        }
#ifdef VJ_STAMPS
        if (getenv("VJ_DEBUG_STAMPS")) {  // diagnostic build (-DVJ_STAMPS=1): phase cycle sums of the tile kernel
            const unsigned long long* se = se_all;
            for (size_t l = 0; l < linfo.size(); ++l)
                fprintf(stderr, "vj launch %zu kind %d class %d: max resident workgroups %llu\n", l, linfo[l].kind, linfo[l].lds_class,
                        se[(1 + l) * VJ_MAX_STAGES + 39]);
            for (size_t l = 0; l < linfo.size(); ++l)   // queue passes: chunk time sum / max / chunks; stump-parallel tail: A, B, pairs, stages
                if (linfo[l].kind == 1)
                    fprintf(stderr, "vj queue launch %zu [%d,%d): chunks %llu sum %llu max %llu | tail A %llu B %llu pairs %llu stages %llu\n", l,
                            linfo[l].stage_begin, linfo[l].stage_end, se[(1 + l) * VJ_MAX_STAGES + 50], se[(1 + l) * VJ_MAX_STAGES + 48],
                            se[(1 + l) * VJ_MAX_STAGES + 49], se[(1 + l) * VJ_MAX_STAGES + 51], se[(1 + l) * VJ_MAX_STAGES + 52],
                            se[(1 + l) * VJ_MAX_STAGES + 53], se[(1 + l) * VJ_MAX_STAGES + 54]);
            for (size_t l = 0; l < linfo.size(); ++l)   // grid pass: when the waves leave the unit loop (vj_kernels.hip, slots 40..45)
                if (linfo[l].kind == VJ_LAUNCH_GRID) {
                    const unsigned long long* g = se + (1 + l) * VJ_MAX_STAGES + 40;
                    const double wgs = (double)std::max(1ull, g[5]), span = (double)(g[3] - ~g[4]);
                    fprintf(stderr, "vj grid launch %zu: workgroups %llu span %.0f ticks | per workgroup last - mean wave end: mean %.0f (%.2f %%) max %llu (%.2f %%) | "
                            "launch end - mean last wave end %.0f (%.2f %%)\n", l, g[5], span, (double)g[0] / wgs, 100.0 * (double)g[0] / wgs / span, g[1],
                            100.0 * (double)g[1] / span, (double)g[3] - (double)g[2] / wgs, 100.0 * ((double)g[3] - (double)g[2] / wgs) / span);
                }
            fprintf(stderr, "vj stamps:");
            for (int i = 40; i < 63; ++i) {   // (60 .. 62: the dense sweep's groups, its lone chunks, how many lone chunks)
                unsigned long long v = 0;
                for (int l = 1; l <= VJ_MAX_LAUNCHES; ++l) v += se[l * VJ_MAX_STAGES + i];
                fprintf(stderr, " %llu", v);
            }
            fprintf(stderr, "\n");
        }
#endif
        if (count) {
            for (size_t s = 0; s < pl->stages.size(); ++s)
                for (int l = 1; l <= VJ_MAX_LAUNCHES; ++l) ctr->stage_entered[s] += se_all[(size_t)l * VJ_MAX_STAGES + s];
            // multi-node trees: nodes below the roots that the walks visited, and their rectangles — parked in the two derived
            // fields until fill_counters prices the roots (every entering window evaluates those) and adds these
            ctr->stump_evals += se_all[0];
            ctr->gather_bytes += se_all[1];
        }
        std::vector<DetEntry> raw(n_det);
        const uint32_t have = std::min(n_det, L->det_copied);
        if (have) memcpy(raw.data(), (const char*)L->h_pinned + ((counts_bytes + 255) & ~(size_t)255), (size_t)have * sizeof(DetEntry));
        if (n_det > have)
            HIP_TRY(hipMemcpy(raw.data() + have, (const DetEntry*)L->d_det.p + have, (size_t)(n_det - have) * sizeof(DetEntry),
                              hipMemcpyDeviceToHost));
        const uint32_t stride = (uint32_t)W + 1u;
        const uint64_t fbytes = (uint64_t)pl->frame_elems * 4u;
        for (const DetEntry& d : raw) {
            const uint32_t f = (uint32_t)(d.off / fbytes);
            const uint32_t el = (uint32_t)((d.off - (uint64_t)f * fbytes) / 4u);
            dets->push_back(RawDet{f0 + (int)f, d.scale, el % stride, el / stride});
        }
        if (raw_out) *raw_out = std::move(raw);
        return VJ_OK;
    }
    set_error("detection buffer overflow persisted");
    return VJ_ERR_LIMIT;
}

// One sub-batch: frames [f0, f0+nf).  Appends decoded detections to `dets`.
static int detect_subbatch(vj_env* e, Plan* pl, const vj_image* frames, int f0, int nf, int W, int H,
                           const vj_params& p, bool equalize, std::vector<RawDet>* dets, vj_counters* ctr, vj_timing* tm) {
    int rc;
    Lane* L = &e->lane0;
    if ((rc = enqueue_prepare(e, L, pl, frames + f0, nf, W, H, false, nullptr, equalize, true))) return rc;
    if ((rc = enqueue_cascade(e, L, pl, W, H, p))) return rc;
    return finish_batch(e, L, pl, f0, W, H, p, dets, ctr, tm);
}

// Sort, widen and (optionally) group the decoded detections of a whole call; fill the counters.
static void fill_counters(Plan* pl, int n_frames, const vj_params& p, vj_result* out) {
    if (!(p.flags & VJ_FLAG_COUNTERS)) return;
    vj_counters& k = out->counters;
    k.windows = pl->windows_per_frame * (uint64_t)n_frames;
    // node evaluations as the oracle counts them: every node a window's walk visits.  Stumps: every node of an
    // entered stage.  Multi-node trees: the root of every tree of an entered stage + the nodes below the roots that the
    // counted kernels saw visited (finish_batch parked those in the two derived fields).
    const uint64_t child_nodes = k.stump_evals, child_rects = k.gather_bytes;
    uint64_t rect_evals = pl->trees ? child_rects : 0;
    k.stump_evals = pl->trees ? child_nodes : 0;
    for (size_t s = 0; s < pl->stages.size(); ++s) {
        k.stump_evals += k.stage_entered[s] * (pl->trees ? pl->prog.n_roots[s] : pl->prog.n_nodes[s]);
        rect_evals += k.stage_entered[s] * (pl->trees ? pl->prog.n_root_rects[s] : pl->prog.n_rects[s]);
    }
    k.gather_bytes = 48ull * k.windows + 16ull * rect_evals;
}

static int build_result(Plan* pl, std::vector<RawDet>& dets, int n_frames, const vj_params& p, vj_result* out) {
    // deterministic order: (frame, scale_idx, y, x)
    std::sort(dets.begin(), dets.end(), [](const RawDet& a, const RawDet& b) {
        return std::tie(a.frame, a.slot, a.y, a.x) < std::tie(b.frame, b.slot, b.y, b.x);
    });
    out->count = (uint32_t)dets.size();
    if (!dets.empty()) {
        out->rects = (vj_rect*)malloc(dets.size() * sizeof(vj_rect));
        if (!out->rects) return VJ_ERR_NOMEM;
        for (size_t i = 0; i < dets.size(); ++i) {
            const vj_scale_info& si = pl->scales_info[dets[i].slot];
            out->rects[i] = vj_rect{(int32_t)dets[i].x, (int32_t)dets[i].y, si.win_w, si.win_h, 0.0f, dets[i].frame,
                                    si.scale_idx};
        }
    }
    if (p.min_neighbors != 0 && out->count) {  // clod.cpp:1325-1326: filterResult(matches, n, MAX(min_neighbors, 1), EPS)
        const int rc = vj_group_rectangles(out->rects, &out->count, (int)std::max<uint32_t>(p.min_neighbors, 1u), 0.2);
        if (rc) return rc;
    }
    fill_counters(pl, n_frames, p, out);
    return VJ_OK;
}

// Frames per sub-batch so that 32-bit byte offsets into the batch sum image never wrap and the worst-case survivor
// queues stay within a fixed budget.
static uint64_t max_frames_per_subbatch(const vj_env* e, const Plan* pl) {
    const uint64_t frame_bytes = (uint64_t)pl->frame_elems * 4u;
    uint64_t max_frames = (0xffffffffull - (uint64_t)pl->max_reach_elems * 4u - 16u) / frame_bytes;
    const uint64_t q_budget = 6ull << 30;  // bytes per queue
    // a queue holds Q_PARTS parts of ceil(frames / Q_PARTS) frames' worth of windows each (layout_queues)
    auto fit_parts = [](uint64_t frames_worth) {
        return frames_worth >= Q_PARTS ? frames_worth / Q_PARTS * Q_PARTS : std::max<uint64_t>(1, frames_worth);
    };
    if (pl->windows_per_frame) {
        max_frames = std::min<uint64_t>(max_frames, fit_parts(q_budget / (pl->windows_per_frame * sizeof(QEntry))));
        max_frames = std::min<uint64_t>(max_frames, fit_parts(0xffffffffull / pl->windows_per_frame));
    }
    if (e->max_subbatch > 0) max_frames = std::min<uint64_t>(max_frames, (uint64_t)e->max_subbatch);
    return max_frames;
}

static int check_frames(const vj_image* frames, int n_frames, int* W_, int* H_, int* CH_) {
    const int W = frames[0].width, H = frames[0].height;
    if (W <= 0 || H <= 0) return VJ_ERR_ARG;
    const int CH = image_channels(frames[0]);
    if (CH != 1 && CH != 3 && CH != 4) {
        set_error("frames must have 1 (gray), 3 (BGR) or 4 (BGRA) channels");
        return VJ_ERR_ARG;
    }
    for (int i = 0; i < n_frames; ++i) {
        if (!frames[i].data || frames[i].width != W || frames[i].height != H || image_channels(frames[i]) != CH ||
            frames[i].stride < W * CH) {
            set_error("frame %d: all frames of a batch must be non-null and of equal size and channel count", i);
            return VJ_ERR_ARG;
        }
    }
    if ((uint64_t)(W + 1) * (uint64_t)(H + 3) >= (1ull << 30)) {
        set_error("image too large");
        return VJ_ERR_LIMIT;
    }
    *W_ = W;
    *H_ = H;
    *CH_ = CH;
    return VJ_OK;
}

}  // namespace vj

extern "C" {
static void drop_plans(vj_env* e);   // (defined inside the extern "C" block below: the same language linkage here)
}

// Arguments of the region pass (roi_plan_units + cascade_roi_pass): `second` inside regions of the nf frames whose integral
// images sit in e->d_sum / e->d_sqsum.  The region list is e->d_rois (max_rois entries), its length on the device at
// roi_counts[0]; the counters live in the lane's counts block.
static void fill_region_args(vj_env* e, Lane* L, Plan* pl2, const vj_cascade* second, const vj_params& p_second, int W, int H, int nf,
                             uint32_t max_rois, RoiArgs* ra_, CascadeArgs* ca_) {
    uint32_t* roi_counts = (uint32_t*)L->d_counts.p + CountsLayout::roi_off_u32;
    const uint32_t stride = (uint32_t)W + 1u;
    RoiArgs& ra = *ra_;
    memset(&ra, 0, sizeof(ra));
    ra.frame_bytes = pl2->frame_elems * 4u;
    ra.stride = stride;
    ra.rois = (RoiDev*)e->d_rois.p;
    ra.n_rois = roi_counts + 0;
    ra.max_rois = max_rois;
    ra.n_frames = (uint32_t)nf;
    ra.frame_w = W;
    ra.frame_h = H;
    ra.win_w0 = second->win_w;
    ra.win_h0 = second->win_h;
    ra.units = (RoiUnit*)e->d_roi_units.p;
    ra.n_units = roi_counts + 1;   // (+2: invalid regions)
    ra.max_units = e->roi_unit_cap;
    ra.ticket = roi_counts + 3;
    ra.det = (RoiDet*)e->d_roi_det.p;
    ra.det_count = roi_counts + 4;
    ra.det_cap = e->roi_det_cap;
    CascadeArgs& ca = *ca_;
    memset(&ca, 0, sizeof(ca));
    ca.sum = (const uint32_t*)e->d_sum.p;
    ca.sqsum = (const uint64_t*)e->d_sqsum.p;
    ca.table = (const uint32_t*)pl2->d_table.p;
    ca.scales = (const ScaleDev*)pl2->d_scales.p;
    ca.stages = (const StageDev*)pl2->d_stages.p;
    ca.n_frames = (uint32_t)nf;
    ca.n_scales = (uint32_t)pl2->scales.size();
    ca.frame_elems = pl2->frame_elems;
    ca.sum_bytes = (uint32_t)((uint64_t)pl2->frame_elems * 4u * (uint64_t)nf);
    ca.stride = stride;
    ca.gather_waves = (uint32_t)std::min(e->gather_waves_for(nf, pl2->general, pl2->trees), (int)GATHER_WAVES_FULL);   // the region pass keeps full queues
    ca.q_cap = (uint32_t)UNIT_WINDOWS;
    ca.stage_begin = 0;
    ca.stage_end = pl2->general ? pl2->pass_bounds.back() : (uint32_t)pl2->stages.size();   // stage trees: positions in the sweep order
    ca.identity_order = pl2->general ? 0u : 1u;
    ca.tree2 = 0u;
    ca.signed_mean = (p_second.flags & VJ_FLAG_SIGNED_MEAN) ? 1u : 0u;
    ca.pos_mode = pl2->pos_mode;   // (0 on this path: check_params sends the f64 grids through the per-size plans; bound all the same)
    ca.pos_tab = (const uint32_t*)pl2->d_pos_tab.p;
    ca.gather_pairs = 2u;   // regions are small: thin waves, latency-bound
    ca.sp_tail_max = (uint32_t)std::max(0, std::min(e->sp_tail_max, (int)gather_tail_max(ca.q_cap)));
    ca.max_stage_nodes = pl2->max_stage_nodes;
    ca.stage_entered = (unsigned long long*)(roi_counts + 8);
    ca.tree_ctr = (unsigned long long*)((uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32) + 2;   // the spare array's [2], [3]: the region pass's
    // Regions with large grids at the small scales (many raw candidates, big faces) run those grids on the tile kernel
    // (cascade_tile_roi_pass: tiles of the second cascade's two-per-CU tile scales, laid inside the region): stump cascades
    // whose plan has such tiles.  The caller sizes e->d_roi_tiles and zeroes the eight ticket counters.
    if (e->roi_tile_min_windows > 0 && !pl2->general && !pl2->trees && pl2->wave_tail && pl2->class_first[1] > pl2->class_first[0] &&
        e->roi_tile_cap != 0u) {
        ra.tiles = (RoiTile*)e->d_roi_tiles.p;
        ra.n_tiles = roi_counts + 6;
        ra.max_tiles = e->roi_tile_cap;
        ra.tile_min_windows = (uint32_t)e->roi_tile_min_windows;
        ca.tile_lds_bytes = pl2->class_lds[0];
        const int per_cu = std::max(1, std::min(32 / TILE_WAVES, (int)(160u * 1024u / ca.tile_lds_bytes)));
        ra.tile_blocks = (uint32_t)std::max(1, e->n_cu * per_cu);
        ca.tile_ticket = (uint32_t*)L->d_counts.p + (CountsLayout::q_counts - 40u);
        ca.n_pass = 1;                       // the whole cascade inside the tile: survivors are detections
        ca.pass_begin[0] = 0;
        ca.pass_begin[1] = (uint32_t)pl2->stages.size();
        ca.tile_end = (uint32_t)pl2->stages.size();
        ca.tile_min_lanes = 0;
        ca.tile_repack_mask = e->tile_repack_mask;
        ca.tile_sp_begin = (uint32_t)e->tile_sp_begin;
        ca.sp_blocks = (const SpBlock*)pl2->d_sp_blocks.p;
        ca.n_sp_blocks = pl2->n_sp_blocks;
        ca.tile_ws_min = (uint32_t)e->tile_ws_min;
        ca.tile_ws_max = (uint32_t)std::min(e->tile_ws_max, (int)TILE_WS_MAX_WINDOWS);
    }
}

// vj_detect_rois on frames of one size with a linear cascade: one integral per frame and ONE region pass for regions of
// any sizes (the machinery of vj_detect_chain's second half, the region list uploaded instead of built on the device) —
// not one plan and one vj_detect call per distinct region size.
static int detect_rois_on_device(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                                 const vj_params* p, int W, int H, vj_result* out) {
    int rc;
    Plan* pl2;
    if ((rc = get_plan(e, c, W, H, *p, &pl2))) return rc;
    const uint64_t max_frames = max_frames_per_subbatch(e, pl2);
    if (max_frames == 0) {
        set_error("a single frame exceeds the 32-bit offset range");
        return VJ_ERR_LIMIT;
    }
    {
        uint64_t dummy = 0;
        if (pl2->frames_q == 0 && (rc = layout_queues(pl2, 1, &dummy))) return rc;
    }
    Lane* L = &e->lane0;
    const bool count2 = (p->flags & VJ_FLAG_COUNTERS) != 0;
    const uint32_t stride = (uint32_t)W + 1u;
    const uint64_t fbytes = (uint64_t)pl2->frame_elems * 4u;
    struct Det2 { int roi; uint32_t slot, x, y; };
    std::vector<Det2> dets2;
    uint64_t child2_nodes = 0, child2_rects = 0;   // counted calls, multi-node trees: visited nodes below the roots (second cascade)
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        std::vector<RoiDev> regions;
        std::vector<int> index;   // position in `regions` -> the caller's region
        for (int i = 0; i < n_rois; ++i)
            if (rois[i].frame >= f0 && rois[i].frame < f0 + nf) {
                regions.push_back(RoiDev{rois[i].frame - f0, rois[i].x, rois[i].y, rois[i].w, rois[i].h});
                index.push_back(i);
            }
        if (regions.empty()) continue;
        if ((rc = enqueue_prepare(e, L, pl2, frames + f0, nf, W, H, false, nullptr))) return rc;
        if (e->roi_unit_cap == 0) e->roi_unit_cap = 1u << 18;
        if (e->roi_det_cap == 0) e->roi_det_cap = 1u << 16;
        const uint32_t n_reg = (uint32_t)regions.size();
        if ((rc = e->d_rois.ensure((size_t)n_reg * sizeof(RoiDev)))) return rc;
        HIP_TRY(hipMemcpyAsync(e->d_rois.p, regions.data(), (size_t)n_reg * sizeof(RoiDev), hipMemcpyHostToDevice, e->stream));
        uint32_t n_units = 0, n_det2 = 0;
        float ms_roi = 0;
        bool ok = false;
        for (int attempt = 0; attempt < 6 && !ok; ++attempt) {
            if ((rc = e->d_roi_units.ensure((size_t)e->roi_unit_cap * sizeof(RoiUnit)))) return rc;
            if ((rc = e->d_roi_det.ensure((size_t)e->roi_det_cap * sizeof(RoiDet)))) return rc;
            if (e->roi_tile_cap == 0) e->roi_tile_cap = 1u << 16;
            if ((rc = e->d_roi_tiles.ensure((size_t)e->roi_tile_cap * sizeof(RoiTile)))) return rc;
            HIP_TRY(hipMemsetAsync((uint32_t*)L->d_counts.p + (CountsLayout::q_counts - 40u), 0, 8 * 4, e->stream));   // tile tickets of the region pass
            uint32_t* roi_counts = (uint32_t*)L->d_counts.p + CountsLayout::roi_off_u32;
            HIP_TRY(hipMemsetAsync(roi_counts, 0, (8 + (size_t)VJ_MAX_STAGES * 2) * 4, e->stream));
            HIP_TRY(hipMemsetAsync((uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32 + 4, 0, 16, e->stream));   // the region pass's tree counters
            HIP_TRY(hipMemcpyAsync(roi_counts, &n_reg, 4, hipMemcpyHostToDevice, e->stream));
            RoiArgs ra;
            CascadeArgs ca;
            fill_region_args(e, L, pl2, c, *p, W, H, nf, n_reg, &ra, &ca);
            HIP_TRY(hipEventRecord(L->launch_ev[2 * VJ_MAX_LAUNCHES - 2], e->stream));
            const int hrc = launch_roi_chain(ra, ca, false, pl2->trees, count2, pl2->general, std::max(1, e->n_cu * e->blocks_per_cu), e->stream,
                                             e->concurrent ? e->stream2 : nullptr, e->fork_ev, e->join_ev);
            if (hrc) {
                set_error("region pass launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return VJ_ERR_HIP;
            }
            HIP_TRY(hipEventRecord(L->launch_ev[2 * VJ_MAX_LAUNCHES - 1], e->stream));
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::roi_off_u32, roi_counts, (8 + (size_t)VJ_MAX_STAGES * 2) * 4,
                                   hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::stage_off_u32 + 4, (uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32 + 4, 16,
                                   hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipEventRecord(L->done, e->stream));
            HIP_TRY(hipEventSynchronize(L->done));
            const uint32_t* hc = (const uint32_t*)L->h_pinned;
            n_units = hc[CountsLayout::roi_off_u32 + 1];
            n_det2 = hc[CountsLayout::roi_off_u32 + 4];
            if (hc[CountsLayout::roi_off_u32 + 2] != 0) {
                set_error("internal error: %u regions outside their frames", hc[CountsLayout::roi_off_u32 + 2]);
                return VJ_ERR_HIP;
            }
            const uint32_t n_tiles2 = hc[CountsLayout::roi_off_u32 + 6];
            if (n_units > e->roi_unit_cap || n_det2 > e->roi_det_cap || n_tiles2 > e->roi_tile_cap) {
                e->roi_unit_cap = grown_cap(e->roi_unit_cap, n_units);
                e->roi_det_cap = grown_cap(e->roi_det_cap, n_det2);
                e->roi_tile_cap = grown_cap(e->roi_tile_cap, n_tiles2);
                continue;
            }
            HIP_TRY(hipEventElapsedTime(&ms_roi, L->launch_ev[2 * VJ_MAX_LAUNCHES - 2], L->launch_ev[2 * VJ_MAX_LAUNCHES - 1]));
            ok = true;
        }
        if (!ok) {
            set_error("region buffers kept overflowing");
            return VJ_ERR_LIMIT;
        }
        float ms_i = 0;
        HIP_TRY(hipEventElapsedTime(&ms_i, L->ev[0], L->ev[1]));
        out->timing.integral_ms += ms_i;
        out->timing.cascade_ms += ms_roi;
        out->timing.total_ms += ms_i + ms_roi;
        out->timing.n_cascade_launches = 1;
        std::vector<RoiDet> raw2(n_det2);
        if (n_det2) HIP_TRY(hipMemcpy(raw2.data(), e->d_roi_det.p, (size_t)n_det2 * sizeof(RoiDet), hipMemcpyDeviceToHost));
        for (const RoiDet& d : raw2) {
            const uint32_t f = (uint32_t)(d.off / fbytes);
            const uint32_t el = (uint32_t)((d.off - (uint64_t)f * fbytes) / 4u);
            const RoiDev& r1 = regions[d.roi];
            dets2.push_back(Det2{index[d.roi], d.slot, el % stride - (uint32_t)r1.x, el / stride - (uint32_t)r1.y});
        }
        if (count2) {
            const unsigned long long* se = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::roi_off_u32 + 8);
            const unsigned long long* tc = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::stage_off_u32) + 2;
            child2_nodes += tc[0];
            child2_rects += tc[1];
            for (size_t s2 = 0; s2 < pl2->stages.size(); ++s2) out->counters.stage_entered[s2] += se[s2];
        }
    }
    std::sort(dets2.begin(), dets2.end(), [](const Det2& a, const Det2& b) {
        return std::make_tuple(a.roi, a.slot, a.y, a.x) < std::make_tuple(b.roi, b.slot, b.y, b.x);
    });
    out->count = (uint32_t)dets2.size();
    if (!dets2.empty()) {
        out->rects = (vj_rect*)malloc(dets2.size() * sizeof(vj_rect));
        if (!out->rects) return VJ_ERR_NOMEM;
        for (size_t i = 0; i < dets2.size(); ++i) {
            const vj_scale_info& si = pl2->scales_info[dets2[i].slot];
            out->rects[i] = vj_rect{(int32_t)dets2[i].x, (int32_t)dets2[i].y, si.win_w, si.win_h, 0.0f, dets2[i].roi, si.scale_idx};
        }
    }
    if (p->min_neighbors != 0 && out->count) {
        rc = vj_group_rectangles(out->rects, &out->count, (int)std::max<uint32_t>(p->min_neighbors, 1u), 0.2);
        if (rc) return rc;
    }
    if (count2) {
        vj_counters& k = out->counters;
        k.windows = k.stage_entered[0];
        uint64_t rect_evals = 0;
        for (size_t s2 = 0; s2 < pl2->stages.size(); ++s2) {   // (as fill_counters: roots on the host, visited child nodes from the device)
            k.stump_evals += k.stage_entered[s2] * (pl2->trees ? pl2->prog.n_roots[s2] : pl2->prog.n_nodes[s2]);
            rect_evals += k.stage_entered[s2] * (pl2->trees ? pl2->prog.n_root_rects[s2] : pl2->prog.n_rects[s2]);
        }
        if (pl2->trees) {
            k.stump_evals += child2_nodes;
            rect_evals += child2_rects;
        }
        k.gather_bytes = 48ull * k.windows + 16ull * rect_evals;
    }
    return VJ_OK;
}


extern "C" {

int vj_env_create(int device_index, vj_env** out) {
    if (!out) return VJ_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t he = hipGetDeviceCount(&n);
    if (he != hipSuccess || n <= 0) {
        set_error("no HIP device (hipGetDeviceCount: %s); this library has no CPU fallback",
                  he == hipSuccess ? "0 devices" : hipGetErrorString(he));
        return VJ_ERR_NO_DEVICE;
    }
    if (device_index < 0 || device_index >= n) {
        set_error("device_index %d out of range [0,%d)", device_index, n);
        return VJ_ERR_ARG;
    }
    auto e = std::make_unique<vj_env>();
    e->device = device_index;
    HIP_TRY(hipSetDevice(device_index));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_index));
    snprintf(e->name, sizeof(e->name), "%s (%s)", prop.name, prop.gcnArchName);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; the kernels are built for gfx950 only", device_index, prop.gcnArchName);
        return VJ_ERR_NO_DEVICE;
    }
    e->n_cu = prop.multiProcessorCount;
    e->tile_group = tile_group_from_env();
    if (const char* g = getenv("VJ_SQ32")) e->sq32 = atoi(g) != 0;
    if (const char* g = getenv("VJ_SQ_U32")) e->sq_u32 = atoi(g) != 0;
    if (const int hrc = prepare_tile_kernels()) {
        set_error("raising the dynamic LDS limit on device %d failed: %s", device_index, hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (const int hrc = prepare_cv_tile_kernels()) {
        set_error("raising the dynamic LDS limit on device %d failed: %s", device_index, hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (const int hrc = prepare_group_kernels()) {
        set_error("raising the dynamic LDS limit on device %d failed: %s", device_index, hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (const int hrc = prepare_cv_chain_kernels()) {
        set_error("raising the dynamic LDS limit on device %d failed: %s", device_index, hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if (const int hrc = prepare_cv_biggest_kernels()) {
        set_error("raising the dynamic LDS limit on device %d failed: %s", device_index, hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    { const int lrc = e->lane0.create(); if (lrc) return lrc; }
    HIP_TRY(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->join_ev, hipEventDisableTiming));
    for (hipEvent_t& ev : e->cv_chain_ev) HIP_TRY(hipEventCreate(&ev));
    for (hipEvent_t& ev : e->cv_rois_ev) HIP_TRY(hipEventCreate(&ev));
    for (hipEvent_t& ev : e->atlas_ev) HIP_TRY(hipEventCreate(&ev));
    for (hipEvent_t& ev : e->call_ev) HIP_TRY(hipEventCreate(&ev));
    for (hipEvent_t& ev : e->track_ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
    *out = e.release();
    return VJ_OK;
}

void vj_env_destroy(vj_env* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    drop_plans(e);
    for (DevBuf* b : {&e->d_sum, &e->d_sqsum, &e->d_band_sum, &e->d_band_sq, &e->d_band_sqp, &e->d_tilted, &e->d_tilt_diag, &e->d_tilt_col, &e->d_out,
                      &e->d_skip_bits, &e->d_rois, &e->d_roi_units, &e->d_roi_det, &e->d_roi_tiles, &e->d_group, &e->d_cv_det, &e->d_cv_counts,
                      &e->d_cv_accept, &e->d_cv_tq, &e->d_cv_fail_rows, &e->d_cv_fail_walk, &e->d_run_table,
                      &e->d_canny_cls, &e->d_canny_label, &e->d_canny_flag, &e->d_edges, &e->d_edge_sum,
                      &e->d_cv_prune_bits, &e->d_pyr, &e->d_pyr_tab, &e->d_cv_big, &e->d_cv_rois, &e->d_cv_roi_units,
                      &e->d_cv_chain, &e->d_cv_chain_keys, &e->d_cv_chain_staged, &e->d_cv_roi_first, &e->d_cv_det2, &e->d_cv_counts2,
                      &e->d_cv_rl_levels, &e->d_cv_rl_taps, &e->d_cv_rl_scales, &e->d_cv_rl_rows, &e->d_cv_rl_table, &e->d_cv_rl_stages,
                      &e->d_points, &e->d_point_units, &e->d_point_scales, &e->d_point_out, &e->d_atlas, &e->d_atlas_src, &e->d_prep, &e->d_extract, &e->d_yuv, &e->d_track})
        b->release();
    e->lane0.destroy();
    for (DevBuf& b : e->d_q) b.release();
    for (DevBuf& b : e->d_q2) b.release();
    for (hipEvent_t& ev : e->cv_chain_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t& ev : e->cv_rois_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t& ev : e->atlas_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t& ev : e->call_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t& ev : e->track_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (e->fork_ev) (void)hipEventDestroy(e->fork_ev);
    if (e->join_ev) (void)hipEventDestroy(e->join_ev);
    if (e->stream2) (void)hipStreamDestroy(e->stream2);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int vj_env_device_name(const vj_env* e, char* buf, size_t cap) {
    if (!e || !buf || cap == 0) return VJ_ERR_ARG;
    snprintf(buf, cap, "%s, %d CUs", e->name, e->n_cu);
    return VJ_OK;
}

static void drop_cv_point_plans(vj_env* e) {
    for (auto& kv : e->cv_point_cascades) kv.second->release_device();
    e->cv_point_cascades.clear();
    for (auto& kv : e->cv_point_plans) kv.second->release_device();
    e->cv_point_plans.clear();
    for (auto& kv : e->clod_point_cascades) kv.second->release_device();
    e->clod_point_cascades.clear();
    for (auto& kv : e->clod_point_plans) kv.second->release_device();
    e->clod_point_plans.clear();
}

static void drop_plans(vj_env* e) {
    for (auto& kv : e->plans) kv.second->release_device();
    e->plans.clear();
    for (auto& kv : e->cv_plans) kv.second->release_device();
    e->cv_plans.clear();
    for (auto& kv : e->cv_roi_plans) kv.second->release_device();
    e->cv_roi_plans.clear();
    drop_cv_point_plans(e);
}

// ----------------------------------------------------------------------------------------- tunables
// One row per vj_env_configure key: how its value is parsed, the field it lands in and what a new value invalidates.
// vj_env_query formats the same field back in the syntax configure accepts.
namespace {

enum class Kind { Bool, Clamp, Range, Auto, List, Custom };
//   Bool   atoi(value) != 0                       Range  atoi(value), VJ_ERR_ARG outside [lo, hi]
//   Clamp  atoi(value) clamped to [lo, hi]        Auto   -1 for negative values ("auto"), else clamped to [lo, hi]
//   List   comma-separated integers               Custom the row's own set / get (get == nullptr: an action, not a value)
enum : unsigned {
    DROP_PLANS = 1,       // the value is baked into plans: sync, then drop every cached plan
    DROP_CV_PLANS = 2,    // ... into OpenCV-profile plans only
    SET_THRESHOLDS = 4,   // the tile thresholds were chosen by the caller: no per-frame-size defaults (get_plan)
    SET_SPLIT = 8,        // the chain balance was chosen by the caller: no feedback
    CLEAR_BALANCE = 16,   // forget the chain balances found so far
};

struct Key {
    const char* name;
    Kind kind;
    unsigned effects;
    int Tunables::*i;                // Bool (an int field), Clamp, Range, Auto
    bool Tunables::*b;               // Bool
    std::vector<int> Tunables::*v;   // List
    int lo, hi;
    int (*set)(vj_env*, const char*);                  // Custom
    void (*get)(const vj_env*, std::string&);          // Custom
};

constexpr int MAX = INT_MAX;
Key flag(const char* n, bool Tunables::*f, unsigned fx = 0) { return {n, Kind::Bool, fx, nullptr, f}; }
Key int_flag(const char* n, int Tunables::*f, unsigned fx = 0) { return {n, Kind::Bool, fx, f}; }   // an int field holding 0 / 1
Key clamped(const char* n, int Tunables::*f, int lo, int hi, unsigned fx = 0) { return {n, Kind::Clamp, fx, f, nullptr, nullptr, lo, hi}; }
Key bounded(const char* n, int Tunables::*f, int lo, int hi, unsigned fx = 0) { return {n, Kind::Range, fx, f, nullptr, nullptr, lo, hi}; }
Key with_auto(const char* n, int Tunables::*f, int lo, int hi, unsigned fx = 0) { return {n, Kind::Auto, fx, f, nullptr, nullptr, lo, hi}; }
Key int_list(const char* n, std::vector<int> Tunables::*f, unsigned fx = 0) { return {n, Kind::List, fx, nullptr, nullptr, f}; }
Key special(const char* n, int (*set)(vj_env*, const char*), void (*get)(const vj_env*, std::string&), unsigned fx = 0) {
    return {n, Kind::Custom, fx, nullptr, nullptr, nullptr, 0, 0, set, get};
}

// "a,b,c" -> integers; at most max_n of them are read (the rest of the string is ignored)
bool parse_list(const char* s, std::vector<long>& out, size_t max_n = SIZE_MAX) {
    for (const char* q = s; *q && out.size() < max_n;) {
        char* end;
        const long x = strtol(q, &end, 10);
        if (end == q) return false;
        out.push_back(x);
        q = *end == ',' ? end + 1 : end;
    }
    return true;
}

void append_list(std::string& s, const int* v, size_t n) {
    for (size_t k = 0; k < n; ++k) s += (k ? "," : "") + std::to_string(v[k]);
}

int set_tile_classes(vj_env* e, const char* value) {   // "36,64,140"; "0,0,0" disables the LDS-tile path
    std::vector<long> v;
    bool ok = parse_list(value, v, TILE_CLASSES);
    for (long x : v) ok = ok && (int)x >= -4 && (int)x <= 140;
    if (!ok) {
        set_error("tile_classes_kb: expected up to %d comma-separated values in [-4,140]", TILE_CLASSES);
        return VJ_ERR_ARG;
    }
    for (int k = 0; k < TILE_CLASSES; ++k) e->tile_class_kb[k] = k < (int)v.size() ? (int)v[k] : 0;
    return VJ_OK;
}

int set_tile_repack(vj_env* e, const char* value) {   // "3,5": stages before which tiles re-pack ("" = never)
    std::vector<long> v;
    bool ok = parse_list(value, v);
    unsigned long long m = 0;
    for (long x : v) {
        ok = ok && x >= 1 && x <= 63;
        if (ok) m |= 1ull << x;
    }
    if (!ok) {
        set_error("tile_repack: expected comma-separated stage indices in [1,63]");
        return VJ_ERR_ARG;
    }
    e->tile_repack_mask = m;
    return VJ_OK;
}

void get_tile_repack(const vj_env* e, std::string& s) {
    std::vector<int> v;
    for (int x = 0; x < 64; ++x)
        if (e->tile_repack_mask >> x & 1) v.push_back(x);
    append_list(s, v.data(), v.size());
}

int set_tile_split(vj_env* e, const char* value) {   // one value for every batch size, or "small,mid,large" (<= 4, < 32, >= 32 frames)
    float a = 0, b = 0, c = 0;
    if (sscanf(value, "%f,%f,%f", &a, &b, &c) != 3) a = b = c = (float)atof(value);
    e->tile_split_small = std::max(0.0f, a);
    e->tile_split_mid = std::max(0.0f, b);
    e->tile_split = std::max(0.0f, c);
    return VJ_OK;
}

int set_det_cap(vj_env* e, const char* value) {   // (re)sets the detection buffer capacity; it still grows on overflow
    const int v = atoi(value);
    if (v < 1) {
        set_error("det_cap must be >= 1");
        return VJ_ERR_ARG;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->det_cap_init = (uint32_t)v;
    e->lane0.det_cap = 0;
    return VJ_OK;
}

int set_auto_balance(vj_env* e, const char* value) {   // 1: find the chain balance of a batch workload from its first calls' times; "reset": start over
    if (strcmp(value, "reset") == 0) e->tile_split_set = false;
    else e->auto_balance = atoi(value) != 0;
    return VJ_OK;
}

int set_defaults(vj_env* e, const char*) {   // every tunable as vj_env_create left it
    static_cast<Tunables&>(*e) = Tunables{};
    e->lane0.det_cap = 0;   // det_cap_init applies again
    return VJ_OK;
}

const Key KEYS[] = {
    // launch structure
    int_list("pass_split", &Tunables::split_override, DROP_PLANS),
    int_list("pass_cut_nodes", &Tunables::pass_cut_nodes, DROP_PLANS),
    bounded("blocks_per_cu", &Tunables::blocks_per_cu, 1, 16),
    int_flag("concurrent", &Tunables::concurrent),
    clamped("concurrent_blocks_per_cu", &Tunables::concurrent_blocks_per_cu, 1, MAX),
    clamped("max_subbatch", &Tunables::max_subbatch, 0, MAX),
    special("det_cap", set_det_cap, [](const vj_env* e, std::string& s) { s = std::to_string(e->det_cap_init); }),
    // LDS tiles
    special("tile_classes_kb", set_tile_classes, [](const vj_env* e, std::string& s) { append_list(s, e->tile_class_kb, TILE_CLASSES); },
            DROP_PLANS),
    clamped("tile_lds_reserve_kb", &Tunables::tile_lds_reserve_kb, 0, 96, DROP_PLANS),
    bounded("tile_min_windows", &Tunables::tile_min_windows, 0, 65536, DROP_PLANS | SET_THRESHOLDS),
    bounded("tile_accept_windows", &Tunables::tile_accept_windows, 0, 65536, DROP_PLANS | SET_THRESHOLDS),
    bounded("tile_max_dwords_per_window", &Tunables::tile_max_dwords_per_window, 0, 65536, DROP_PLANS | SET_THRESHOLDS),
    bounded("tile_end", &Tunables::tile_end, 0, 65536, DROP_PLANS),
    bounded("tile_min_lanes", &Tunables::tile_min_lanes, 0, 65536, DROP_PLANS),
    special("tile_repack", set_tile_repack, get_tile_repack),
    // tile finish
    clamped("tile_sp_begin", &Tunables::tile_sp_begin, 0, MAX, DROP_PLANS),   // the LDS layout of the tile launches depends on it
    clamped("tile_ws_min", &Tunables::tile_ws_min, 0, TILE_SP_MAX_WINDOWS),
    clamped("tile_ws_max", &Tunables::tile_ws_max, 0, TILE_WS_MAX_WINDOWS),
    // chain balance
    special("tile_split", set_tile_split,
            [](const vj_env* e, std::string& s) {
                char b[64];
                snprintf(b, sizeof(b), "%.9g,%.9g,%.9g", e->tile_split_small, e->tile_split_mid, e->tile_split);
                s = b;
            },
            DROP_PLANS | SET_SPLIT | CLEAR_BALANCE),
    special("auto_balance", set_auto_balance, [](const vj_env* e, std::string& s) { s = std::to_string((int)e->auto_balance); },
            CLEAR_BALANCE),
    special("balance_export", [](vj_env* e, const char* path) { return balance_export(e, path); }, nullptr),
    special("balance_import", [](vj_env* e, const char* path) { return balance_import(e, path); }, nullptr),
    // global-gather chain
    clamped("grid_block_w", &Tunables::grid_block_w, 0, UNIT_WINDOWS, DROP_PLANS),
    clamped("gather_waves", &Tunables::gather_waves, INT_MIN, MAX, DROP_PLANS),   // 1 ... 8, or -1 = 4 for calls of >= 8 frames; the first-pass units follow it
    with_auto("gather_pairs", &Tunables::gather_pairs, 0, 2),
    clamped("sp_tail_max", &Tunables::sp_tail_max, 0, 48),
    with_auto("wide_tail", &Tunables::wide_tail, 0, 1),
    clamped("min_chunk", &Tunables::min_chunk, 1, 64),
    with_auto("q_slices", &Tunables::q_slices, 0, 64),
    clamped("q_band_px", &Tunables::q_band_px, 0, MAX, DROP_PLANS),
    clamped("q_group_units", &Tunables::q_group_units, 0, MAX, DROP_PLANS),
    clamped("q_band_min_frames", &Tunables::q_band_min_frames, 1, MAX),
    // stage trees
    int_flag("general_prefix", &Tunables::general_prefix, DROP_PLANS),
    int_flag("tile_segments", &Tunables::tile_segments),
    clamped("seg_cut2", &Tunables::seg_cut2, 0, MAX, DROP_PLANS),
    flag("tree_split_queues", &Tunables::tree_split_queues),
    // regions / chain
    flag("rois_on_device", &Tunables::rois_on_device),
    clamped("roi_tiles", &Tunables::roi_tile_min_windows, 0, MAX),
    clamped("group_max", &Tunables::group_max, 1, GROUP_MAX),
    // OpenCV profile
    flag("cv_tiles", &Tunables::cv_tiles, DROP_CV_PLANS),
    with_auto("cv_row_blocks", &Tunables::cv_row_blocks, 1, 4, DROP_CV_PLANS),
    with_auto("cv_tile_min_windows", &Tunables::cv_tile_min_windows, 64, MAX, DROP_CV_PLANS),
    clamped("cv_tile_min_windows0", &Tunables::cv_tile_min_windows0, 64, MAX, DROP_CV_PLANS),
    clamped("cv_tile_ws_max", &Tunables::cv_tile_ws_max, 0, CVT_WS_MAX, DROP_CV_PLANS),
    clamped("cv_row_blocks_tree", &Tunables::cv_row_blocks_tree, 1, 4, DROP_CV_PLANS),
    clamped("cv_tile_min_windows_tree", &Tunables::cv_tile_min_windows_tree, 64, MAX, DROP_CV_PLANS),
    flag("cv_tree_chains", &Tunables::cv_tree_chains),
    clamped("cv_tree_chunk", &Tunables::cv_tree_chunk, 1, MAX),
    clamped("cv_tree_chain_blocks", &Tunables::cv_tree_chain_blocks, 1, MAX),
    clamped("cv_tail_max", &Tunables::cv_tail_max, 0, CV_TAIL_MAX, DROP_PLANS),
    clamped("cv_row_band_px", &Tunables::cv_row_band_px, 0, MAX, DROP_PLANS),
    flag("cv_tree2", &Tunables::cv_tree2, DROP_PLANS),   // (the default balance depends on it)
    flag("cv_tiles_tilted", &Tunables::cv_tiles_tilted, DROP_PLANS),
    clamped("cv_tree_queue_cap", &Tunables::cv_tree_queue_cap, 0, MAX),
    // single frames, integral, housekeeping
    clamped("one_pass_max_frames", &Tunables::one_pass_max_frames, 0, MAX),   // (part of the plan key: nothing to drop)
    clamped("integral_rows", &Tunables::integral_rows_mode, 0, 2),
    clamped("plan_cache_max", &Tunables::plan_cache_max, 2, MAX),   // vj_detect_chain holds two plans at once
    special("defaults", set_defaults, nullptr, DROP_PLANS | CLEAR_BALANCE),
};

const Key* find_key(const char* name) {
    for (const Key& k : KEYS)
        if (strcmp(k.name, name) == 0) return &k;
    set_error("unknown option '%s'", name);
    return nullptr;
}

}  // namespace

int vj_env_query(const vj_env* e, const char* key, char* buf, size_t cap) {
    if (!e || !key || !buf || cap == 0) return VJ_ERR_ARG;
    const Key* k = find_key(key);
    if (!k) return VJ_ERR_ARG;
    std::string s;
    switch (k->kind) {
        case Kind::Bool: s = std::to_string(k->b ? (int)(e->*k->b) : e->*k->i); break;
        case Kind::List: append_list(s, (e->*k->v).data(), (e->*k->v).size()); break;
        case Kind::Custom:
            if (!k->get) {
                set_error("'%s' is an action, not a value", key);
                return VJ_ERR_ARG;
            }
            k->get(e, s);
            break;
        default: s = std::to_string(e->*k->i);
    }
    if (s.size() >= cap) {
        set_error("vj_env_query(%s): the value needs %zu bytes", key, s.size() + 1);
        return VJ_ERR_ARG;
    }
    memcpy(buf, s.c_str(), s.size() + 1);
    return VJ_OK;
}

int vj_env_configure(vj_env* e, const char* key, const char* value) {
    if (!e || !key || !value) return VJ_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    const Key* k = find_key(key);
    if (!k) return VJ_ERR_ARG;
    const int v = atoi(value);
    switch (k->kind) {
        case Kind::Bool:
            if (k->b) e->*k->b = v != 0;
            else e->*k->i = v != 0;
            break;
        case Kind::Clamp: e->*k->i = std::max(k->lo, std::min(v, k->hi)); break;
        case Kind::Auto: e->*k->i = v < 0 ? -1 : std::max(k->lo, std::min(v, k->hi)); break;
        case Kind::Range:
            if (v < k->lo || v > k->hi) {
                set_error("%s must be in [%d,%d]", key, k->lo, k->hi);
                return VJ_ERR_ARG;
            }
            e->*k->i = v;
            break;
        case Kind::List: {
            std::vector<long> x;
            if (!parse_list(value, x)) {
                set_error("%s: expected comma-separated integers, got '%s'", key, value);
                return VJ_ERR_ARG;
            }
            e->*k->v = std::vector<int>(x.begin(), x.end());
            break;
        }
        case Kind::Custom:
            if (const int rc = k->set(e, value)) return rc;
    }
    if (k->effects & SET_THRESHOLDS) e->tile_thresholds_set = true;
    if (k->effects & SET_SPLIT) e->tile_split_set = true;
    if (k->effects & CLEAR_BALANCE) e->balance.clear();
    if (k->effects & (DROP_PLANS | DROP_CV_PLANS)) HIP_TRY(hipStreamSynchronize(e->stream));
    if (k->effects & DROP_PLANS) drop_plans(e);
    if (k->effects & DROP_CV_PLANS) {
        for (auto& kv : e->cv_plans) kv.second->release_device();
        e->cv_plans.clear();
        for (auto& kv : e->cv_roi_plans) kv.second->release_device();
        e->cv_roi_plans.clear();
        drop_cv_point_plans(e);
    }
    return VJ_OK;
}

int vj_env_reserve(vj_env* e, int max_w, int max_h, int max_batch) {
    if (!e || max_w <= 0 || max_h <= 0 || max_batch <= 0) return VJ_ERR_ARG;
    HIP_TRY(hipSetDevice(e->device));
    return ensure_image_buffers(e, max_w, max_h, max_batch, true);
}

int vj_integral_image(vj_env* e, const vj_image* image, uint32_t* sum, uint64_t* sqsum) {
    if (!e || !image || !image->data || !sum || !sqsum) return VJ_ERR_ARG;
    const int w = image->width, h = image->height, ch = image_channels(*image);
    if (w <= 0 || h <= 0 || (ch != 1 && ch != 3 && ch != 4) || image->stride < w * ch) return VJ_ERR_ARG;
    if ((uint64_t)(w + 1) * (uint64_t)(h + 3) >= (1ull << 30)) {
        set_error("image too large");
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = ensure_image_buffers(e, w, h, 1, true, ch))) return rc;
    const uint8_t* d_gray;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_gray, &fb, &gs))) return rc;
    if ((rc = enqueue_integral(e, d_gray, fb, gs, w, h, 1, ch))) return rc;
    const size_t n = (size_t)(w + 1) * (size_t)(h + 1);
    HIP_TRY(hipMemcpyAsync(sum, e->d_sum.p, n * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(sqsum, e->d_sqsum.p, n * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return VJ_OK;
}

int vj_integral_batch_sq32(vj_env* e, const vj_image* frames, int n_frames, uint32_t* sum, uint32_t* sqsum32) {
    if (!e || !frames || n_frames <= 0 || !sum || !sqsum32) return VJ_ERR_ARG;
    int W, H, CH, rc;
    if ((rc = check_frames(frames, n_frames, &W, &H, &CH))) return rc;
    const size_t fe = frame_elems_for(W, H);
    if (fe * 8u * (size_t)n_frames > 0xfffffff0ull) {
        set_error("vj_integral_batch_sq32: %d frames of %d x %d exceed one batch", n_frames, W, H);
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_image_buffers(e, W, H, n_frames, true, CH))) return rc;
    const uint8_t* d_gray;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, frames, n_frames, W, H, &d_gray, &fb, &gs))) return rc;
    if ((rc = enqueue_integral(e, d_gray, fb, gs, W, H, n_frames, CH, true))) return rc;
    // frame f of either image starts at element f * frame_elems on the device; the caller's arrays are dense
    const size_t row = (size_t)(W + 1) * (size_t)(H + 1) * 4;
    HIP_TRY(hipMemcpy2DAsync(sum, row, e->d_sum.p, fe * 4, row, (size_t)n_frames, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpy2DAsync(sqsum32, row, e->d_sqsum.p, fe * 4, row, (size_t)n_frames, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return VJ_OK;
}

}  // extern "C"

namespace vj {
// one image of vj_integral_image / vj_integral_tilted / vj_grayscale / vj_canny: channels, row stride, addressing limit
int check_single_image(const vj_image* image, int* ch_out) {
    const int w = image->width, h = image->height, ch = image_channels(*image);
    if (w <= 0 || h <= 0 || (ch != 1 && ch != 3 && ch != 4) || image->stride < w * ch) return VJ_ERR_ARG;
    if ((uint64_t)(w + 1) * (uint64_t)(h + 3) >= (1ull << 30)) {
        set_error("image too large");
        return VJ_ERR_LIMIT;
    }
    *ch_out = ch;
    return VJ_OK;
}
}  // namespace vj

extern "C" {

int vj_integral_tilted(vj_env* e, const vj_image* image, uint32_t* tilted) {
    if (!e || !image || !image->data || !tilted) return VJ_ERR_ARG;
    int ch, rc;
    if ((rc = check_single_image(image, &ch))) return rc;
    const int w = image->width, h = image->height;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_image_buffers(e, w, h, 1, true, ch))) return rc;
    const uint8_t* d_gray;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_gray, &fb, &gs))) return rc;
    if ((rc = enqueue_tilted(e, d_gray, fb, gs, w, h, 1, ch))) return rc;
    HIP_TRY(hipMemcpyAsync(tilted, e->d_tilted.p, (size_t)(w + 1) * (size_t)(h + 1) * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return VJ_OK;
}

int vj_grayscale(vj_env* e, const vj_image* image, uint8_t* gray, int gray_stride) {
    if (!e || !image || !image->data || !gray || gray_stride < image->width) return VJ_ERR_ARG;
    int ch, rc;
    if ((rc = check_single_image(image, &ch))) return rc;
    const int w = image->width, h = image->height;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_image_buffers(e, w, h, 1, true, ch))) return rc;
    const uint8_t* d_src;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_src, &fb, &gs))) return rc;
    const size_t pitch = align4((size_t)w);
    if ((rc = e->d_out.ensure(pitch * (size_t)h))) return rc;
    TiltedArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.gray = d_src;
    ta.gray_frame_bytes = fb;
    ta.gray_stride = (uint32_t)gs;
    ta.channels = (uint32_t)ch;
    ta.width = (uint32_t)w;
    ta.height = (uint32_t)h;
    ta.n_frames = 1;
    const int hrc = launch_grayscale(ta, (uint8_t*)e->d_out.p, (uint32_t)pitch, e->stream);
    if (hrc) {
        set_error("grayscale launch failed: %s", hipGetErrorString((hipError_t)hrc));
        return VJ_ERR_HIP;
    }
    if ((size_t)gray_stride == pitch && pitch == (size_t)w) {
        // one block only when the device rows carry no padding: with w % 4 != 0 a block copy would write the pad bytes
        // over the caller's row padding (caller data if `gray` is a view into a larger image) and past a tight last row
        HIP_TRY(hipMemcpyAsync(gray, e->d_out.p, pitch * (size_t)h, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return VJ_OK;
    }
    // another row stride on the host: one block into page-locked memory, the rows from there (a 2-D copy into pageable
    // memory goes row by row in the runtime)
    Lane* L = &e->lane0;
    const size_t need = pitch * (size_t)h;
    if (const int err = stage_reserve(L, need)) return err;
    HIP_TRY(hipMemcpyAsync(L->h_stage, e->d_out.p, need, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int y = 0; y < h; ++y) memcpy(gray + (size_t)y * (size_t)gray_stride, (const uint8_t*)L->h_stage + (size_t)y * pitch, (size_t)w);
    return VJ_OK;
}

int vj_equalize_hist(vj_env* e, const vj_image* image, uint8_t* dst, int dst_stride) {
    if (!e || !image || !image->data || !dst || dst_stride < image->width) return VJ_ERR_ARG;
    int ch, rc;
    if ((rc = check_single_image(image, &ch))) return rc;
    const int w = image->width, h = image->height;
    HIP_TRY(hipSetDevice(e->device));
    if ((rc = ensure_image_buffers(e, w, h, 1, true, ch))) return rc;
    const uint8_t* d_src;
    size_t fb;
    int gs;
    if ((rc = stage_frames(e, image, 1, w, h, &d_src, &fb, &gs))) return rc;
    Lane* L = &e->lane0;
    if ((rc = enqueue_equalize(e, L, &d_src, &fb, &gs, &ch, w, h, 1))) return rc;
    // one block into page-locked memory, the rows from there (as vj_grayscale returns a strided image)
    const size_t pitch = (size_t)gs, need = pitch * (size_t)h;
    if (const int err = stage_reserve(L, need)) return err;
    HIP_TRY(hipMemcpyAsync(L->h_stage, d_src, need, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (int y = 0; y < h; ++y) memcpy(dst + (size_t)y * (size_t)dst_stride, (const uint8_t*)L->h_stage + (size_t)y * pitch, (size_t)w);
    return VJ_OK;
}

int vj_host_alloc(vj_env* e, size_t bytes, void** out) {
    if (!e || !out || bytes == 0) return VJ_ERR_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(e->device));
    const hipError_t he = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (he != hipSuccess) {
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(he));
        *out = nullptr;
        return he == hipErrorOutOfMemory ? VJ_ERR_NOMEM : VJ_ERR_HIP;
    }
    return VJ_OK;
}

void vj_host_free(vj_env* e, void* p) {
    if (!e || !p) return;
    (void)hipSetDevice(e->device);
    (void)hipHostFree(p);
}

int vj_integral(vj_env* e, const uint8_t* gray, int w, int h, int stride, uint32_t* sum, uint64_t* sqsum) {
    if (!e || !gray || !sum || !sqsum || w <= 0 || h <= 0 || stride < w) return VJ_ERR_ARG;
    vj_image im{gray, w, h, stride, 0, 1};
    return vj_integral_image(e, &im, sum, sqsum);
}

int vj_detect(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_params* p,
              vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || (n_frames > 0 && !frames)) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (n_frames == 0) return VJ_OK;
    // VJ_FLAG_EQUALIZE_HIST is read here and nowhere else: plans, balance entries and kernels see the parameters without it
    const bool equalize = (p->flags & VJ_FLAG_EQUALIZE_HIST) != 0u;
    vj_params q = *p;
    q.flags &= ~(uint32_t)VJ_FLAG_EQUALIZE_HIST;
    p = &q;
    int rc = check_params(*p);
    if (rc) return rc;
    int W, H, CH;
    rc = check_frames(frames, n_frames, &W, &H, &CH);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    Plan* pl;
    vj_env::Balance* bal = balance_of(e, c, W, H, *p, n_frames, true);   // (created before the plan is looked up: it names the split)
    if (bal) balance_touch(bal, n_frames);
    rc = get_plan(e, c, W, H, *p, &pl, n_frames);
    if (rc) return rc;
    const uint64_t max_frames = max_frames_per_subbatch(e, pl);
    if (max_frames == 0) {
        set_error("a single frame exceeds the 32-bit offset range");
        return VJ_ERR_LIMIT;
    }
    std::vector<RawDet> dets;
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        rc = detect_subbatch(e, pl, frames, f0, nf, W, H, *p, equalize, &dets, &out->counters, &out->timing);
        if (rc) return rc;
    }
    // feedback for the chain balance: only the timed (uncounted) kernel variants.  A plan none of whose scales can run on tiles
    // has nothing to balance; a CANDIDATE split that leaves one chain only (every tile moved to the gathers, or a share of
    // the scales without large ones) is measured like any other — the search must be able to step back from it
    if (bal && bal->phase != 3) {
        bool any_tile_scale = false;
        for (const ScaleDev& sd : pl->scales) any_tile_scale |= sd.tile_rw != 0;
        if (!any_tile_scale) {
            bal->cur = bal->best;
            bal->phase = 3;
        } else if (!(p->flags & VJ_FLAG_COUNTERS) && (uint64_t)n_frames <= max_frames && n_frames == bal->n_ref) {
            balance_report(bal, out->timing.cascade_ms / (float)n_frames, !e->tile_thresholds_set);
        }
    }
    out->timing.tile_split = pl->tile_split;
    out->timing.balance_state = !bal ? 0 : bal->phase == 3 ? 2 : 1;
    out->timing.balance_calls = bal ? bal->calls : 0;
    return build_result(pl, dets, n_frames, *p, out);
}

// Second cascade on regions of interest (config 5: eyes inside faces).  A ROI is a view —
// pointer + stride — into its frame, as the reference's callers would pass a sub-image header; detection windows
// come in few distinct sizes, so the ROIs are grouped by size and every group is ONE batched vj_detect pass.
int vj_detect_rois(vj_env* e, const vj_cascade* c, const vj_image* frames, int n_frames, const vj_roi* rois, int n_rois,
                   const vj_params* p, vj_result* out) {
    if (!e || !c || !p || !out || n_frames < 0 || n_rois < 0 || (n_rois > 0 && (!frames || !rois))) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (refuse_equalize(p->flags, "vj_detect_rois")) return VJ_ERR_UNSUPPORTED;
    {
        const int prc = check_params(*p);
        if (prc) return prc;
    }
    std::map<std::pair<int, int>, std::vector<int>> by_size;   // (w, h) -> ROI indices
    for (int i = 0; i < n_rois; ++i) {
        const vj_roi& r = rois[i];
        if (r.frame < 0 || r.frame >= n_frames || !frames[r.frame].data || r.w <= 0 || r.h <= 0 || r.x < 0 || r.y < 0 ||
            r.x + r.w > frames[r.frame].width || r.y + r.h > frames[r.frame].height) {
            set_error("roi %d lies outside its frame", i);
            return VJ_ERR_ARG;
        }
        by_size[{r.w, r.h}].push_back(i);
    }
    // frames of one size, a linear cascade, the exhaustive grid: every region in one pass on the frames' own integral images
    // (a scale mask selects among the plan's scales; every region still enumerates its own prefix of them)
    if (n_rois > 0 && n_frames > 0 && !(p->flags & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW)) && p->scale_factor > 1.0f && e->rois_on_device) {
        bool same = true;
        for (int i = 0; i < n_frames && same; ++i)
            same = frames[i].data && frames[i].width == frames[0].width && frames[i].height == frames[0].height &&
                   image_channels(frames[i]) == image_channels(frames[0]) && frames[i].stride >= frames[i].width * image_channels(frames[i]);
        int W = 0, H = 0, CH = 0;
        if (same && check_frames(frames, n_frames, &W, &H, &CH) == VJ_OK) {
            HIP_TRY(hipSetDevice(e->device));
            return detect_rois_on_device(e, c, frames, n_frames, rois, n_rois, p, W, H, out);
        }
    }
    std::vector<vj_rect> all;
    for (const auto& kv : by_size) {
        std::vector<vj_image> views;
        int ch0 = -1;
        for (int i : kv.second) {
            const vj_roi& r = rois[i];
            const vj_image& f = frames[r.frame];
            const int ch = image_channels(f);
            if (ch0 < 0) ch0 = ch;
            if (ch != ch0) {
                set_error("ROIs of one size must come from frames with the same channel count");
                return VJ_ERR_ARG;
            }
            views.push_back(vj_image{f.data + (size_t)r.y * (size_t)f.stride + (size_t)r.x * (size_t)ch, r.w, r.h, f.stride,
                                     f.on_device, f.channels});
        }
        vj_result part;
        int rc = vj_detect(e, c, views.data(), (int)views.size(), p, &part);
        if (rc) {
            vj_result_free(&part);
            return rc;
        }
        for (uint32_t k = 0; k < part.count; ++k) {
            vj_rect rr = part.rects[k];
            rr.frame = kv.second[(size_t)rr.frame];   // index in the batch -> ROI index
            all.push_back(rr);
        }
        // counters and times add up over the groups
        out->counters.windows += part.counters.windows;
        out->counters.stump_evals += part.counters.stump_evals;
        out->counters.gather_bytes += part.counters.gather_bytes;
        for (int s2 = 0; s2 < VJ_MAX_STAGES; ++s2) out->counters.stage_entered[s2] += part.counters.stage_entered[s2];
        out->timing.integral_ms += part.timing.integral_ms;
        out->timing.cascade_ms += part.timing.cascade_ms;
        out->timing.total_ms += part.timing.total_ms;
        vj_result_free(&part);
    }
    std::stable_sort(all.begin(), all.end(), [](const vj_rect& a, const vj_rect& b) { return a.frame < b.frame; });
    out->count = (uint32_t)all.size();
    if (!all.empty()) {
        out->rects = (vj_rect*)malloc(all.size() * sizeof(vj_rect));
        if (!out->rects) return VJ_ERR_NOMEM;
        memcpy(out->rects, all.data(), all.size() * sizeof(vj_rect));
    }
    return VJ_OK;
}


// ------------------------------------------------------------------ two cascades, hand-off on the device
int vj_detect_chain(vj_env* e, const vj_cascade* first, const vj_cascade* second, const vj_image* frames, int n_frames,
                    const vj_params* p_first, const vj_params* p_second, vj_result* out_first, vj_result* out_second) {
    if (!e || !first || !second || !p_first || !p_second || !out_first || !out_second || n_frames < 0 || (n_frames > 0 && !frames))
        return VJ_ERR_ARG;
    memset(out_first, 0, sizeof(*out_first));
    memset(out_second, 0, sizeof(*out_second));
    if (refuse_equalize(p_first->flags | p_second->flags, "vj_detect_chain")) return VJ_ERR_UNSUPPORTED;
    if (n_frames == 0) return VJ_OK;
    for (const vj_params* pp : {p_first, p_second}) {
        const int prc = check_params(*pp);
        if (prc) return prc;
    }
    if ((p_first->flags | p_second->flags) & (VJ_FLAG_SKIP_LIST | VJ_FLAG_SKIP_ROW)) {
        // the CPU variants' skip rules make a window's fate depend on its row's history inside ITS image: the first cascade runs
        // as vj_detect does, the second one per region size on the sub-images (vj_detect_rois' path for these modes) — the
        // hand-off goes through the host, the results are the ones the definition above gives
        int rc = vj_detect(e, first, frames, n_frames, p_first, out_first);
        if (rc) return rc;
        std::vector<vj_roi> regions(out_first->count);
        for (uint32_t i = 0; i < out_first->count; ++i) {
            const vj_rect& q = out_first->rects[i];
            regions[i] = vj_roi{(int32_t)q.frame, q.x, q.y, q.w, q.h};
        }
        if (regions.empty()) return VJ_OK;
        return vj_detect_rois(e, second, frames, n_frames, regions.data(), (int)regions.size(), p_second, out_second);
    }
    const bool grouped = p_first->min_neighbors != 0;   // the regions are the GROUPED candidates (grouped on the device)
    int W, H, CH;
    int rc = check_frames(frames, n_frames, &W, &H, &CH);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(e->device));
    Plan *pl1, *pl2;
    // (the first cascade's chain balance is found by feedback as in vj_detect: its kernels run before the region pass starts)
    vj_env::Balance* bal = balance_of(e, first, W, H, *p_first, n_frames, true);
    if (bal) balance_touch(bal, n_frames);
    if ((rc = get_plan(e, first, W, H, *p_first, &pl1, n_frames))) return rc;
    // the second cascade is planned for the frame's stride and every scale a region as large as the frame could use;
    // each region picks its own scales and grid on the device
    if ((rc = get_plan(e, second, W, H, *p_second, &pl2))) return rc;
    if ((rc = get_plan(e, first, W, H, *p_first, &pl1, n_frames))) return rc;   // (the cache may have evicted it for pl2: look it up again)
    const uint64_t max_frames = std::min(max_frames_per_subbatch(e, pl1), max_frames_per_subbatch(e, pl2));
    if (max_frames == 0) {
        set_error("a single frame exceeds the 32-bit offset range");
        return VJ_ERR_LIMIT;
    }
    {   // the second plan's scale records go to the device with a queue layout (none is used by the region pass)
        uint64_t dummy = 0;
        if (pl2->frames_q == 0 && (rc = layout_queues(pl2, 1, &dummy))) return rc;
    }
    Lane* L = &e->lane0;
    std::vector<RawDet> dets1;
    std::vector<vj_rect> grouped1;       // grouped mode: the first result, as the device grouped it
    struct Det2 { int roi; uint32_t slot, x, y; };
    std::vector<Det2> dets2;
    uint64_t child2_nodes = 0, child2_rects = 0;   // counted calls, multi-node trees: visited nodes below the roots (second cascade)
    const bool count2 = (p_second->flags & VJ_FLAG_COUNTERS) != 0;
    const uint32_t stride = (uint32_t)W + 1u;
    const uint64_t fbytes = (uint64_t)pl1->frame_elems * 4u;
    for (int f0 = 0; f0 < n_frames; f0 += (int)max_frames) {
        const int nf = (int)std::min<uint64_t>(max_frames, (uint64_t)(n_frames - f0));
        if ((rc = enqueue_prepare(e, L, pl1, frames + f0, nf, W, H, false, nullptr))) return rc;
        if (e->roi_unit_cap == 0) e->roi_unit_cap = 1u << 18;
        if (e->roi_det_cap == 0) e->roi_det_cap = 1u << 16;
        uint32_t n_det1 = 0, n_units = 0, n_det2 = 0;
        size_t roi_weight_off = 0;   // grouped mode: where the groups' member counts sit in d_group
        float ms_roi = 0;
        bool ok = false;
        for (int attempt = 0; attempt < 6 && !ok; ++attempt) {
            if ((rc = enqueue_cascade(e, L, pl1, W, H, *p_first))) return rc;
            if ((rc = e->d_rois.ensure((size_t)L->det_cap * sizeof(RoiDev)))) return rc;
            GroupArgs ga;
            memset(&ga, 0, sizeof(ga));
            if (grouped) {
                // one buffer: keys (u64) | grouped | the zeroed counter block | frame_first | weights
                const size_t cap = L->det_cap, nfz = (size_t)nf;
                const size_t o_keys = 0, o_grouped = o_keys + cap * 8u, o_zero = o_grouped + cap * sizeof(RoiDev),
                             o_first = o_zero + (3u * nfz + 1u) * 4u, o_gw = o_first + (nfz + 1u) * 4u, o_rw = o_gw + cap * 4u,
                             total = o_rw + cap * 4u;
                if ((rc = e->d_group.ensure(total))) return rc;
                char* gb = (char*)e->d_group.p;
                ga.det = (const DetEntry*)L->d_det.p;
                ga.det_count = (const uint32_t*)L->d_counts.p + MAX_PASSES * CountsLayout::q_counts;
                ga.det_cap = L->det_cap;
                ga.scales = (const ScaleDev*)pl1->d_scales.p;
                ga.frame_bytes = pl1->frame_elems * 4u;
                ga.stride = stride;
                ga.n_frames = (uint32_t)nf;
                ga.threshold = (int32_t)std::max<uint32_t>(p_first->min_neighbors, 1u);   // clod.cpp:1326
                ga.eps = 0.2;                                                               // clod.cpp:11
                ga.keys = (uint64_t*)(gb + o_keys);
                ga.grouped = (RoiDev*)(gb + o_grouped);
                ga.frame_count = (uint32_t*)(gb + o_zero);
                ga.frame_cursor = ga.frame_count + nfz;
                ga.grouped_count = ga.frame_cursor + nfz;
                ga.overflow = ga.grouped_count + nfz;
                ga.frame_first = (uint32_t*)(gb + o_first);
                ga.grouped_weight = (uint32_t*)(gb + o_gw);
                ga.roi_weight = (uint32_t*)(gb + o_rw);
                roi_weight_off = o_rw;
                ga.rois = (RoiDev*)e->d_rois.p;
                ga.max_rois = L->det_cap;
                ga.group_max = (uint32_t)e->group_max;
            }
            if ((rc = e->d_roi_units.ensure((size_t)e->roi_unit_cap * sizeof(RoiUnit)))) return rc;
            if ((rc = e->d_roi_det.ensure((size_t)e->roi_det_cap * sizeof(RoiDet)))) return rc;
            if (e->roi_tile_cap == 0) e->roi_tile_cap = 1u << 16;
            if ((rc = e->d_roi_tiles.ensure((size_t)e->roi_tile_cap * sizeof(RoiTile)))) return rc;
            uint32_t* roi_counts = (uint32_t*)L->d_counts.p + CountsLayout::roi_off_u32;   // zeroed with the block by enqueue_cascade (the tile tickets too)
            RoiArgs ra;
            CascadeArgs ca;
            fill_region_args(e, L, pl2, second, *p_second, W, H, nf, L->det_cap, &ra, &ca);
            ra.det_in = (const DetEntry*)L->d_det.p;
            ra.det_in_count = (const uint32_t*)L->d_counts.p + MAX_PASSES * CountsLayout::q_counts;
            ra.det_in_cap = L->det_cap;
            ra.scales_in = (const ScaleDev*)pl1->d_scales.p;
            HIP_TRY(hipEventRecord(L->launch_ev[2 * VJ_MAX_LAUNCHES - 2], e->stream));
            if (grouped) {
                ga.n_rois = ra.n_rois;
                const int grc = launch_group_rois(ga, e->stream);
                if (grc) {
                    set_error("grouping launch failed: %s", hipGetErrorString((hipError_t)grc));
                    return VJ_ERR_HIP;
                }
                HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::roi_off_u32 + 5, ga.overflow, 4, hipMemcpyDeviceToHost, e->stream));
            }
            const int hrc = launch_roi_chain(ra, ca, !grouped, pl2->trees, count2, pl2->general, std::max(1, e->n_cu * e->blocks_per_cu), e->stream,
                                             e->concurrent ? e->stream2 : nullptr, e->fork_ev, e->join_ev);
            if (hrc) {
                set_error("region pass launch failed: %s", hipGetErrorString((hipError_t)hrc));
                return VJ_ERR_HIP;
            }
            HIP_TRY(hipEventRecord(L->launch_ev[2 * VJ_MAX_LAUNCHES - 1], e->stream));
            // the region counters join the block enqueue_cascade already copies; copy them again now that they are final
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::roi_off_u32, roi_counts, 5 * 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::roi_off_u32 + 6, roi_counts + 6, 4, hipMemcpyDeviceToHost, e->stream));   // region tiles
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::roi_off_u32 + 8, roi_counts + 8, (size_t)VJ_MAX_STAGES * 2 * 4,
                                   hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync((uint32_t*)L->h_pinned + CountsLayout::stage_off_u32 + 4, (uint32_t*)L->d_counts.p + CountsLayout::stage_off_u32 + 4, 16,
                                   hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipEventRecord(L->done, e->stream));
            HIP_TRY(hipEventSynchronize(L->done));
            const uint32_t* hc = (const uint32_t*)L->h_pinned;
            n_det1 = hc[MAX_PASSES * CountsLayout::q_counts];
            n_units = hc[CountsLayout::roi_off_u32 + 1];
            n_det2 = hc[CountsLayout::roi_off_u32 + 4];
            if (hc[CountsLayout::roi_off_u32 + 2] != 0) {
                set_error("internal error: %u regions outside their frames", hc[CountsLayout::roi_off_u32 + 2]);
                return VJ_ERR_HIP;
            }
            if (n_det1 > L->det_cap) {   // as finish_batch would: grow, and run both cascades again
                const uint32_t want = grown_cap(L->det_cap, n_det1);
                if ((rc = L->d_det.ensure((size_t)want * sizeof(DetEntry)))) return rc;
                L->det_cap = want;
                continue;
            }
            if (grouped && hc[CountsLayout::roi_off_u32 + 5] != 0) {
                // a frame with more raw candidates than the device kernel groups: the same result the long way round
                // (group on the host, hand the regions back as a list)
                vj_result_free(out_first);
                vj_result_free(out_second);
                if ((rc = vj_detect(e, first, frames, n_frames, p_first, out_first))) return rc;
                std::vector<vj_roi> rois(out_first->count);
                for (uint32_t i = 0; i < out_first->count; ++i) {
                    const vj_rect& r = out_first->rects[i];
                    rois[i] = vj_roi{r.frame, r.x, r.y, r.w, r.h};
                }
                return vj_detect_rois(e, second, frames, n_frames, rois.data(), (int)rois.size(), p_second, out_second);
            }
            const uint32_t n_tiles2 = hc[CountsLayout::roi_off_u32 + 6];
            if (n_units > e->roi_unit_cap || n_det2 > e->roi_det_cap || n_tiles2 > e->roi_tile_cap) {
                e->roi_unit_cap = grown_cap(e->roi_unit_cap, n_units);
                e->roi_det_cap = grown_cap(e->roi_det_cap, n_det2);
                e->roi_tile_cap = grown_cap(e->roi_tile_cap, n_tiles2);
                continue;
            }
            HIP_TRY(hipEventElapsedTime(&ms_roi, L->launch_ev[2 * VJ_MAX_LAUNCHES - 2], L->launch_ev[2 * VJ_MAX_LAUNCHES - 1]));
            ok = true;
        }
        if (!ok) {
            set_error("region buffers kept overflowing");
            return VJ_ERR_LIMIT;
        }
        // first cascade: decode (device order kept in raw1 for the region numbers)
        const size_t base1 = dets1.size();
        std::vector<DetEntry> raw1;
        if ((rc = finish_batch(e, L, pl1, f0, W, H, *p_first, &dets1, &out_first->counters, &out_first->timing, &raw1))) return rc;
        // second cascade
        std::vector<RoiDet> raw2(n_det2);
        if (n_det2) HIP_TRY(hipMemcpy(raw2.data(), e->d_roi_det.p, (size_t)n_det2 * sizeof(RoiDet), hipMemcpyDeviceToHost));
        std::vector<RoiDev> regions;
        size_t base_g = grouped1.size();
        if (grouped) {   // the first result is the region list itself
            const uint32_t n_rois = ((const uint32_t*)L->h_pinned)[CountsLayout::roi_off_u32 + 0];
            regions.resize(n_rois);
            std::vector<uint32_t> weights(n_rois);
            if (n_rois) {
                HIP_TRY(hipMemcpy(regions.data(), e->d_rois.p, (size_t)n_rois * sizeof(RoiDev), hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(weights.data(), (const char*)e->d_group.p + roi_weight_off, (size_t)n_rois * 4u, hipMemcpyDeviceToHost));
            }
            for (uint32_t i = 0; i < n_rois; ++i)
                grouped1.push_back(vj_rect{regions[i].x, regions[i].y, regions[i].w, regions[i].h, (float)weights[i], regions[i].frame + f0, -1});
        }
        for (const RoiDet& d : raw2) {
            const uint32_t f = (uint32_t)(d.off / fbytes);
            const uint32_t el = (uint32_t)((d.off - (uint64_t)f * fbytes) / 4u);
            if (grouped) {
                const RoiDev& r1 = regions[d.roi];
                dets2.push_back(Det2{(int)(base_g + d.roi), d.slot, el % stride - (uint32_t)r1.x, el / stride - (uint32_t)r1.y});
            } else {
                const RawDet& r1 = dets1[base1 + d.roi];
                dets2.push_back(Det2{(int)(base1 + d.roi), d.slot, el % stride - r1.x, el / stride - r1.y});
            }
        }
        out_second->timing.cascade_ms += ms_roi;
        out_second->timing.total_ms += ms_roi;
        out_second->timing.n_cascade_launches = 1;
        if (count2) {
            const unsigned long long* se = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::roi_off_u32 + 8);
            const unsigned long long* tc = (const unsigned long long*)((const uint32_t*)L->h_pinned + CountsLayout::stage_off_u32) + 2;
            child2_nodes += tc[0];
            child2_rects += tc[1];
            for (size_t s2 = 0; s2 < pl2->stages.size(); ++s2) out_second->counters.stage_entered[s2] += se[s2];
        }
    }
    if (bal && bal->phase != 3) {   // (as vj_detect: one sub-batch, timed kernel variants only)
        bool any_tile_scale = false;
        for (const ScaleDev& sd : pl1->scales) any_tile_scale |= sd.tile_rw != 0;
        if (!any_tile_scale) {
            bal->cur = bal->best;
            bal->phase = 3;
        } else if (!(p_first->flags & VJ_FLAG_COUNTERS) && (uint64_t)n_frames <= max_frames && n_frames == bal->n_ref) {
            balance_report(bal, out_first->timing.cascade_ms / (float)n_frames, !e->tile_thresholds_set);
        }
    }
    out_first->timing.tile_split = pl1->tile_split;
    out_first->timing.balance_state = !bal ? 0 : bal->phase == 3 ? 2 : 1;
    out_first->timing.balance_calls = bal ? bal->calls : 0;
    // the first result in its sorted order; regions are numbered by their position in it
    std::vector<uint32_t> rank;
    if (grouped) {   // frames in order, groups in cv::partition's class order: already the result's order
        rank.resize(grouped1.size());
        for (size_t i = 0; i < rank.size(); ++i) rank[i] = (uint32_t)i;
        out_first->count = (uint32_t)grouped1.size();
        if (!grouped1.empty()) {
            out_first->rects = (vj_rect*)malloc(grouped1.size() * sizeof(vj_rect));
            if (!out_first->rects) return VJ_ERR_NOMEM;
            memcpy(out_first->rects, grouped1.data(), grouped1.size() * sizeof(vj_rect));
        }
        fill_counters(pl1, n_frames, *p_first, out_first);
    } else {
        std::vector<uint32_t> order(dets1.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return std::tie(dets1[a].frame, dets1[a].slot, dets1[a].y, dets1[a].x) < std::tie(dets1[b].frame, dets1[b].slot, dets1[b].y, dets1[b].x);
        });
        rank.resize(dets1.size());
        for (size_t i = 0; i < order.size(); ++i) rank[order[i]] = (uint32_t)i;
        if ((rc = build_result(pl1, dets1, n_frames, *p_first, out_first))) return rc;
    }
    std::sort(dets2.begin(), dets2.end(), [&](const Det2& a, const Det2& b) {
        return std::make_tuple(rank[a.roi], a.slot, a.y, a.x) < std::make_tuple(rank[b.roi], b.slot, b.y, b.x);
    });
    out_second->count = (uint32_t)dets2.size();
    if (!dets2.empty()) {
        out_second->rects = (vj_rect*)malloc(dets2.size() * sizeof(vj_rect));
        if (!out_second->rects) return VJ_ERR_NOMEM;
        for (size_t i = 0; i < dets2.size(); ++i) {
            const vj_scale_info& si = pl2->scales_info[dets2[i].slot];
            out_second->rects[i] = vj_rect{(int32_t)dets2[i].x, (int32_t)dets2[i].y, si.win_w, si.win_h, 0.0f, (int32_t)rank[dets2[i].roi],
                                           si.scale_idx};
        }
    }
    if (p_second->min_neighbors != 0 && out_second->count) {
        rc = vj_group_rectangles(out_second->rects, &out_second->count, (int)std::max<uint32_t>(p_second->min_neighbors, 1u), 0.2);
        if (rc) return rc;
    }
    if (count2) {
        vj_counters& k = out_second->counters;
        k.windows = k.stage_entered[0];
        uint64_t rect_evals = 0;
        for (size_t s2 = 0; s2 < pl2->stages.size(); ++s2) {   // (as fill_counters: roots on the host, visited child nodes from the device)
            k.stump_evals += k.stage_entered[s2] * (pl2->trees ? pl2->prog.n_roots[s2] : pl2->prog.n_nodes[s2]);
            rect_evals += k.stage_entered[s2] * (pl2->trees ? pl2->prog.n_root_rects[s2] : pl2->prog.n_rects[s2]);
        }
        if (pl2->trees) {
            k.stump_evals += child2_nodes;
            rect_evals += child2_rects;
        }
        k.gather_bytes = 48ull * k.windows + 16ull * rect_evals;
    }
    return VJ_OK;
}

// ------------------------------------------------------------------ frame streams
struct vj_stream {
    vj_env* e = nullptr;
    vj_params p;
    int W = 0, H = 0, CH = 1, max_batch = 0;
    std::unique_ptr<Plan> plan;     // private: its queue layout must not change while a batch is in flight
    Lane lanes[2];
    hipStream_t copy = nullptr;
    int fifo[2] = {0, 0};           // lanes holding submitted batches, oldest first
    int n_pending = 0;
    int n_frames_of[2] = {0, 0};
};

int vj_stream_create(vj_env* e, const vj_cascade* c, int width, int height, int channels, int max_batch, const vj_params* p,
                     vj_stream** out) {
    if (!out) return VJ_ERR_ARG;
    *out = nullptr;
    if (!e || !c || !p || width <= 0 || height <= 0 || max_batch <= 0) return VJ_ERR_ARG;
    const int CH = channels <= 1 ? 1 : channels;
    if (CH != 1 && CH != 3 && CH != 4) return VJ_ERR_ARG;
    if (refuse_equalize(p->flags, "vj_stream_create")) return VJ_ERR_UNSUPPORTED;
    if (check_params(*p)) return VJ_ERR_ARG;
    if ((uint64_t)(width + 1) * (uint64_t)(height + 3) >= (1ull << 30)) {
        set_error("image too large");
        return VJ_ERR_LIMIT;
    }
    HIP_TRY(hipSetDevice(e->device));
    auto s = std::make_unique<vj_stream>();
    s->e = e;
    s->p = *p;
    s->W = width;
    s->H = height;
    s->CH = CH;
    s->max_batch = max_batch;
    s->plan = std::make_unique<Plan>();
    struct Guard {   // releases what was created when a later step fails
        vj_stream* s;
        ~Guard() { if (s) vj_stream_destroy(s); }
    } guard{nullptr};
    // (a chain balance already found for this workload by vj_detect's feedback is taken over; a stream does not search itself)
    const vj_env::Balance* bal = balance_of(e, c, width, height, *p, max_batch, false);
    const bool lower_thresholds = bal && balance_choice(bal, -1).thr == 1 && !e->tile_thresholds_set;
    int rc = plan_and_upload(e, *c, width, height, *p, s->plan.get(), bal ? bal->best : e->split_for(max_batch, *p, linear_stumps(*c)),
                             thresholds_for(*e, lower_thresholds ? 3 : 0), max_batch, false);
    if (rc) {
        s->plan->release_device();
        return rc;
    }
    vj_stream* raw = s.release();
    guard.s = raw;
    if ((uint64_t)max_batch > max_frames_per_subbatch(e, raw->plan.get())) {
        set_error("max_batch %d exceeds what one launch sequence can address at this frame size (%llu frames)", max_batch,
                  (unsigned long long)max_frames_per_subbatch(e, raw->plan.get()));
        return VJ_ERR_LIMIT;
    }
    for (Lane& L : raw->lanes) {
        if ((rc = L.create())) return rc;
        L.shared_integrals = true;
    }
    HIP_TRY(hipStreamCreateWithFlags(&raw->copy, hipStreamNonBlocking));
    // every buffer at its final size now: nothing is (re)allocated while batches are in flight
    for (Lane& L : raw->lanes)
        if ((rc = ensure_image_buffers(e, width, height, max_batch, true, CH, &L))) return rc;
    uint64_t q_entries = 0;
    if ((rc = layout_queues(raw->plan.get(), max_batch, &q_entries))) return rc;
    const size_t n_pass = raw->plan->pass_bounds.size() - 1;
    for (size_t ps = 1; ps < n_pass; ++ps)
        if ((rc = e->d_q[ps].ensure(std::max<uint64_t>(q_entries, 1) * sizeof(QEntry)))) return rc;
    guard.s = nullptr;
    *out = raw;
    return VJ_OK;
}

int vj_stream_submit(vj_stream* s, const vj_image* frames, int n_frames) {
    if (!s || !frames || n_frames <= 0 || n_frames > s->max_batch) return VJ_ERR_ARG;
    if (s->n_pending >= 2) {
        set_error("two batches are pending: collect one before submitting the next");
        return VJ_ERR_LIMIT;
    }
    int W, H, CH;
    int rc = check_frames(frames, n_frames, &W, &H, &CH);
    if (rc) return rc;
    if (W != s->W || H != s->H || CH != s->CH) {
        set_error("frames do not have the stream's size / channel count");
        return VJ_ERR_ARG;
    }
    vj_env* e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    const int lane = s->n_pending == 0 ? 0 : 1 - s->fifo[0];
    Lane* L = &s->lanes[lane];
    // the lane's frame buffer is free once the integral kernels of its previous batch have read it
    HIP_TRY(hipEventSynchronize(L->integral_done));
    if ((rc = enqueue_prepare(e, L, s->plan.get(), frames, n_frames, W, H, true, s->copy, false, true))) return rc;
    if ((rc = enqueue_cascade(e, L, s->plan.get(), W, H, s->p))) return rc;
    s->fifo[s->n_pending] = lane;
    s->n_frames_of[lane] = n_frames;
    s->n_pending++;
    return VJ_OK;
}

int vj_stream_collect(vj_stream* s, vj_result* out) {
    if (!s || !out) return VJ_ERR_ARG;
    memset(out, 0, sizeof(*out));
    if (s->n_pending == 0) {
        set_error("no batch is pending");
        return VJ_ERR_ARG;
    }
    vj_env* e = s->e;
    HIP_TRY(hipSetDevice(e->device));
    const int lane = s->fifo[0];
    s->fifo[0] = s->fifo[1];
    s->n_pending--;
    Lane* L = &s->lanes[lane];
    std::vector<RawDet> dets;
    int rc = finish_batch(e, L, s->plan.get(), 0, s->W, s->H, s->p, &dets, &out->counters, &out->timing);
    if (rc) return rc;
    return build_result(s->plan.get(), dets, s->n_frames_of[lane], s->p, out);
}

void vj_stream_destroy(vj_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->e->device);
    if (s->e->stream) (void)hipStreamSynchronize(s->e->stream);
    if (s->e->stream2) (void)hipStreamSynchronize(s->e->stream2);
    if (s->copy) {
        (void)hipStreamSynchronize(s->copy);
        (void)hipStreamDestroy(s->copy);
    }
    for (Lane& L : s->lanes) L.destroy();
    if (s->plan) s->plan->release_device();
    delete s;
}

void vj_result_free(vj_result* r) {
    if (!r) return;
    free(r->rects);
    r->rects = nullptr;
    r->count = 0;
}

}  // extern "C"
