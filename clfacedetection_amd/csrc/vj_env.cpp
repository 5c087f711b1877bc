// The environment of the HIP path: its life cycle, device buffers and frame staging, the per-(cascade, size, params) plan cache
// with the chain-balance search, the configure table and the image entry points.  It replaces clodInitEnvironment /
// clodInitBuffers (clod.cpp:72-163); the detect drivers that launch on it are vj_detect.cpp and vj_detect_regions.cpp.
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
int plan_and_upload(const vj_env* e, const vj_cascade& c, int W, int H, const vj_params& p, Plan* pl, float tile_split,
                           const TileThresholds& thresholds, int n_frames, bool one_pass) {
    PlanTables tab;
    const int rc = plan_clod(*e, e->tile_group, e->sq32, c, W, H, p, tile_split, thresholds, n_frames, one_pass, false, pl, &tab);
    return rc ? rc : upload_plan(pl, tab);
}

// (Re)lay out the per-scale queue segments for `frames` frames in flight.
int layout_queues(Plan* pl, int frames, uint64_t* total_entries) {
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

vj_env::Balance* balance_of(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, int n_frames, bool create) {
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
BalanceChoice balance_choice(const vj_env::Balance* b, int n_frames) {
    if (b->phase != 3 && n_frames == b->n_ref) return BalanceChoice{b->cur, b->thr, b->cur != b->best || b->phase == 4};
    return BalanceChoice{b->best, b->phase == 4 ? 0 : b->thr, false};
}

// Called once per vj_detect / vj_detect_chain call of a balanced workload, before its plan is looked up: bookkeeping, and the
// reference size follows the traffic (a class whose reference size stopped coming — 32 calls of other sizes — restarts the
// measurement of its current best at the size that does come; what was found so far stays the starting point).
void balance_touch(vj_env::Balance* b, int n_frames) {
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
void balance_report(vj_env::Balance* b, float ms, bool try_thresholds) {
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

int get_plan(vj_env* e, const vj_cascade* c, int W, int H, const vj_params& p, Plan** out, int n_frames) {
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

int check_frames(const vj_image* frames, int n_frames, int* W_, int* H_, int* CH_) {
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
static void drop_plans(vj_env* e);   // (defined below)

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

}  // extern "C"
