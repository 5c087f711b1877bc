"""Cascade shapes no shipped file has, on every entry point that takes a cascade, against the oracle frame by frame.

cases.TOPOLOGY_CELLS stand on each side of the planners' and kernels' fixed-size assumptions ("Fixed-size
assumptions"): 1, 2, 3, 64 and 65 stages around VJ_MAX_STAGES, the 64-bit entered masks and tile_sp_begin; stages of 256 / 257
and 512 / 513 stumps around the two stump-parallel tails; node trees beyond {root, child}; stage trees with a prefix of 0, 1 and
3 stages, 3, 4 and 5 chains around CvChainDev::begin[4] and CascadeArgs::seg_end[4], chains of one stage, chains that overflow
VJ_MAX_PASSES, a nested sibling list, an unreachable stage and a cycle.  tests/test_topology_cases_cpu.py proves on the oracle
alone that every stage of every case is entered and every chain decides something.  Which route a call took is asserted from
public fields (DetectResult.passes / launches, cv_plan_info, vj_plan_tiles) in test_both_sides_of_each_limit_ran: a change that
moves a limit updates that test and the CPU straddle test."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import clod_window_oracle as cw
import find_biggest_oracle as fo
import roc_oracle as ro
import run_window_oracle as rw
import scale_image_oracle as so
from cases import (ARITH_FRAMES, TOPOLOGY_RUNNABLE, cascade_to_product, rows_of, topology_cascade, topology_cell, topology_chains,
                   topology_frames, tunables)
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_SCALE_IMAGE, VjError, default_params,
                                 run_windows, run_windows_opencv)
from clfacedetection_amd.api import (CLOD_WINDOW_RESULT_DTYPE, VJ_PLAN_TILES_FORMER_SHAPES, WINDOW_DTYPE, WINDOW_RESULT_DTYPE, CvParams,
                                     CvRocParams, _Result, _RocResult)

pytestmark = pytest.mark.gpu
VJ_ERR_UNSUPPORTED, VJ_ERR_LIMIT = 4, 8
IDS = [c[0] for c in TOPOLOGY_RUNNABLE]
FAMILY = {c[0]: c[1] for c in TOPOLOGY_RUNNABLE}
STAGE_TREES = [cid for cid in IDS if FAMILY[cid] == "stage_tree"]
BATCHES = (ARITH_FRAMES, 1)
_CASC, _FRAMES, _ORACLE = {}, {}, {}
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module", autouse=True)
def report_oracle_share():
    t = time.perf_counter()
    yield
    print(f"\ntest_gpu_topologies: {time.perf_counter() - t:.1f} s, of which {ORACLE_SECONDS[0]:.1f} s in the oracles")


def cascade(cid):
    """(oracle CascadeArrays, product Cascade)."""
    if cid not in _CASC:
        a = topology_cascade(cid)
        _CASC[cid] = (a, cascade_to_product(a))
    return _CASC[cid]


def frames_of(cid):
    if cid not in _FRAMES:
        _FRAMES[cid] = topology_frames(topology_cell(cid))
    return _FRAMES[cid]


def timed(fn, *args, **kw):
    t = time.perf_counter()
    out = fn(*args, **kw)
    ORACLE_SECONDS[0] += time.perf_counter() - t
    return out


def oracle_of(oracle, cid, profile):
    """[(rects, stats)] of the oracle per frame of the cell, computed once per module.  profile: "clod" (stage trees: the walk of
    mode 1), "cv", "si" (CV_HAAR_SCALE_IMAGE) or "fb" (CV_HAAR_FIND_BIGGEST_OBJECT, min_neighbors 1)."""
    if (cid, profile) not in _ORACLE:
        a, _ = cascade(cid)
        fn = {"clod": lambda f: oracle.detect(a, f), "cv": lambda f: oracle.detect_opencvlike(a, f),
              "si": lambda f: so.detect_scale_image(a, f), "fb": lambda f: fo.detect_biggest(a, f, min_neighbors=1)}[profile]
        if profile in ("si", "fb"):
            fn(frames_of(cid)[0][:40, :40])             # (compiles the restatement before the threads start)
        with ThreadPoolExecutor(8) as ex:
            _ORACLE[cid, profile] = timed(lambda: list(ex.map(fn, frames_of(cid))))
    return _ORACLE[cid, profile]


def srows(rects):
    return sorted(rows_of(rects))


def totals(want, n_stages):
    entered = np.zeros(n_stages, np.int64)
    for _, st in want:
        entered += np.array(st["stage_entered"], np.int64)
    return entered.tolist(), sum(st["windows"] for _, st in want)


def check_call(call, n_stages, want, label):
    """call(flags) -> DetectResult: a counted and an uncounted call against the oracle's per-frame (or per-region) results."""
    r = call(VJ_FLAG_COUNTERS)
    for i, (ro_, _) in enumerate(want):
        mine = srows(r.rects[r.rects["frame"] == i])
        assert mine == srows(ro_), f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(ro_)}"
    entered, windows = totals(want, n_stages)
    assert r.stage_entered == entered, f"{label}: stages entered {r.stage_entered}, the oracle {entered}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"
    r0 = call(0)
    assert np.array_equal(r0.rects, r.rects), f"{label}: the uncounted call's rectangles differ from the counted ones"
    return r


def entered_by(r, kind, stage):
    return sum(l["stage_entered"][stage] for l in r.launches if l["kind"] == kind)


def kinds_of(r):
    return sorted({l["kind"] for l in r.launches})


def route_of(r):
    return (f"passes {[(b, e) for b, e, _ in r.passes]} launches {[(l['kind'], l['stage_begin'], l['stage_end']) for l in r.launches]} "
            f"stages the tiles entered {[s for s in range(len(r.stage_entered)) if entered_by(r, 'tile', s)]}")


# ------------------------------------------------------------------------------------------------ the two detectors
@pytest.mark.parametrize("cid", IDS)
def test_detect_matches_the_oracle(env, oracle, cid):
    a, c = cascade(cid)
    want = oracle_of(oracle, cid, "clod")
    for n in BATCHES:
        r = check_call(lambda fl: env.detect(c, frames_of(cid)[:n], default_params(flags=fl)), a.n_stages, want[:n], f"{cid} n={n}")
        per_launch = [sum(l["stage_entered"][s] for l in r.launches) for s in range(a.n_stages)]
        assert per_launch == r.stage_entered, f"{cid} n={n}: the per-launch counters do not add up: {per_launch} / {r.stage_entered}"
        print(f"ROUTE clod {cid} n={n}: {route_of(r)}")
        # the tile kernel takes part wherever the plan allows tiles: linear cascades, and stage trees with a linear prefix of at
        # least two stages
        if FAMILY[cid] != "stage_tree" or topology_chains(cid)[0][0] >= 2:
            assert "tile" in kinds_of(r), f"{cid} n={n}: {kinds_of(r)}"


@pytest.mark.parametrize("cid", IDS)
def test_detect_opencv_matches_the_oracle(env, oracle, cid):
    """The counted call and the uncounted one (the row kernel's chain sweep for stage trees: another kernel path)."""
    a, c = cascade(cid)
    want = oracle_of(oracle, cid, "cv")
    h, w = topology_cell(cid)[2]
    for n in BATCHES:
        check_call(lambda fl: env.detect_opencv(c, frames_of(cid)[:n], flags=fl), a.n_stages, want[:n], f"cv {cid} n={n}")
        info = env.cv_plan_info(c, w, h, n)
        print(f"ROUTE cv {cid} n={n}: tile scales {info.n_tile_scales} tree_prefix {info.tree_prefix} tree_queue {info.tree_queue}")


# ------------------------------------------------------------------------------------------------ regions
def regions_of(cid):
    h, w = topology_cell(cid)[2]
    return [(0, w - 97, h - 83, 97, 83), (0, 40, 30, 61, 61), (0, 0, 0, w, h)]    # right and bottom edges; 61 x 61; the whole frame


@pytest.mark.parametrize("cid", IDS)
def test_regions_match_the_oracle(env, oracle, cid):
    """The case as the only cascade of vj_detect_rois and vj_detect_opencv_rois on three regions of one frame, each against the
    oracle on the crop; the frame as a batch of eight and alone."""
    a, c = cascade(cid)
    rois = regions_of(cid)
    crops = [np.ascontiguousarray(frames_of(cid)[f][y:y + rh, x:x + rw]) for f, x, y, rw, rh in rois]
    full = {"clod": oracle_of(oracle, cid, "clod")[0], "cv": oracle_of(oracle, cid, "cv")[0]}
    want = {"clod": [timed(oracle.detect, a, g) for g in crops[:2]] + [full["clod"]],
            "cv": [timed(oracle.detect_opencvlike, a, g) for g in crops[:2]] + [full["cv"]]}
    assert sum(len(r) for r, _ in want["clod"][:2]) > 0 and sum(len(r) for r, _ in want["cv"][:2]) > 0
    for n in BATCHES:
        fr = frames_of(cid)[:n]
        check_call(lambda fl: env.detect_rois(c, fr, rois, default_params(flags=fl)), a.n_stages, want["clod"], f"rois {cid} n={n}")
        check_call(lambda fl: env.detect_opencv_rois(c, fr, rois, flags=fl), a.n_stages, want["cv"], f"cv rois {cid} n={n}")


# ------------------------------------------------------------------------------------------------ window lists
def bits32(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def grid_rows(grid, frame, k):
    return np.column_stack([np.full(len(grid), frame), grid, np.full(len(grid), k)]).astype(np.int64).reshape(-1, 4)


@pytest.mark.parametrize("cid", IDS)
def test_window_lists_match_the_restatements(env, cid):
    """vj_run_windows and vj_run_windows_opencv on the full grids of two chain scales (1 and 1.1^3): both grids on the single
    frame, and one grid on the first and one on the last frame of the batch.  `result` exactly, the sums as bit patterns."""
    a, c = cascade(cid)
    h, w = topology_cell(cid)[2]
    frames = frames_of(cid)
    s_clod = [cw.chain_scale(0), cw.chain_scale(3)]
    s_cv = [rw.chain_factor(0), rw.chain_factor(3)]
    g_clod = [cw.grid_of(a, s, w, h) for s in s_clod]
    g_cv = [rw.grid_of(a, s, w, h) for s in s_cv]
    for n, placing in ((1, (0, 0)), (ARITH_FRAMES, (0, ARITH_FRAMES - 1))):
        fr = list(frames[:n])
        wl = np.concatenate([grid_rows(g_clod[k], placing[k], k) for k in range(2)])
        res, sums, var = run_windows(fr, c, env, wl, s_clod)
        want = timed(cw.run_windows, a, fr, wl, s_clod)
        bad = np.flatnonzero((res != want[0]) | (bits32(sums) != bits32(want[1])) | (bits32(var) != bits32(want[2])))
        assert len(bad) == 0, (cid, n, len(bad), [(wl[i].tolist(), int(res[i]), int(want[0][i]), float(sums[i]), float(want[1][i])) for i in bad[:5]])
        assert (res == 1).any() and (res <= 0).any()
        wl = np.concatenate([grid_rows(g_cv[k], placing[k], k) for k in range(2)])
        res, sums = run_windows_opencv(fr, c, env, wl, s_cv)
        want = timed(rw.run_windows, a, fr, wl, s_cv)
        bad = np.flatnonzero((res != want[0]) | (sums.view(np.uint64) != want[1].view(np.uint64)))
        assert len(bad) == 0, (cid, n, len(bad), [(wl[i].tolist(), int(res[i]), int(want[0][i]), float(sums[i]), float(want[1][i])) for i in bad[:5]])
        assert (res == 1).any() and (res <= 0).any()


# ------------------------------------------------------------------------------------------------ the other OpenCV-profile modes
@pytest.mark.parametrize("cid", ["st_c4", "st_c5", "st_root", "st_64"])
def test_scale_image_and_find_biggest_on_stage_trees(env, oracle, cid):
    """Both modes read a stage tree with a route of their own (find-biggest: no chain sweep)."""
    a, c = cascade(cid)
    want_si, want_fb = oracle_of(oracle, cid, "si"), oracle_of(oracle, cid, "fb")
    for n in BATCHES:
        fr = frames_of(cid)[:n]
        check_call(lambda fl: env.detect_opencv(c, fr, flags=fl | VJ_FLAG_CV_SCALE_IMAGE), a.n_stages, want_si[:n], f"scale image {cid} n={n}")
        r = env.detect_opencv(c, fr, min_neighbors=1, flags=VJ_FLAG_CV_FIND_BIGGEST | VJ_FLAG_COUNTERS)
        got = [tuple(int(x[k]) for k in ("frame", "x", "y", "w", "h")) + (int(x["weight"]),) for x in r.rects]
        assert got == [(f,) + tuple(res) for f, (res, _) in enumerate(want_fb[:n]) if res is not None], f"find biggest {cid} n={n}"
        entered, windows = totals(want_fb[:n], a.n_stages)
        assert r.stage_entered == entered and r.windows == windows, f"find biggest {cid} n={n}"
        r0 = env.detect_opencv(c, fr, min_neighbors=1, flags=VJ_FLAG_CV_FIND_BIGGEST)
        assert np.array_equal(r0.rects, r.rects)
    assert sum(res is not None for res, _ in want_fb) >= 1 and sum(len(r_) for r_, _ in want_si) >= 10


# ------------------------------------------------------------------------------------------------ route switches
CLOD_TREE_SWITCHES = [("tile_segments", 0), ("general_prefix", 0), ("tree_split_queues", 0), ("seg_cut2", 4)]
CV_TREE_SWITCHES = [("cv_tree_chains", 0), ("cv_tiles", 0), ("cv_tree_queue_cap", 4096)]
LINEAR_SWITCHES = [("tile_sp_begin", 99), ("tile_ws_max", 0), ("cv_tree2", 0), ("one_pass_max_frames", 8)]


@pytest.mark.parametrize("cid", IDS)
def test_route_switches_give_the_default_result(env, cid):
    """Every switch between two routes gives the default call's result bit for bit, with equal counters (the default call itself
    is compared with the oracle above)."""
    a, c = cascade(cid)
    switches = CLOD_TREE_SWITCHES + CV_TREE_SWITCHES if FAMILY[cid] == "stage_tree" else LINEAR_SWITCHES
    for n in BATCHES:
        fr = frames_of(cid)[:n]
        calls = {"clod": lambda: env.detect(c, fr, default_params(flags=VJ_FLAG_COUNTERS)),
                 "cv": lambda: env.detect_opencv(c, fr, flags=VJ_FLAG_COUNTERS)}
        base = {k: f() for k, f in calls.items()}
        for key, value in switches:
            profile = "cv" if key.startswith("cv_") else "clod"
            with tunables(env, (key, value)):
                r = calls[profile]()
            b = base[profile]
            assert np.array_equal(r.rects, b.rects), f"{cid} n={n} {key} {value}: {len(r.rects)} rectangles, the default {len(b.rects)}"
            assert r.stage_entered == b.stage_entered and r.windows == b.windows, f"{cid} n={n} {key} {value}: {r.stage_entered} / {b.stage_entered}"


# ------------------------------------------------------------------------------------------------ both sides of each limit
def test_both_sides_of_each_limit_ran(env):
    def passes(cid, n):
        _, c = cascade(cid)
        return [(b, e) for b, e, _ in env.detect(c, frames_of(cid)[:n]).passes]
    for n in BATCHES:
        # the clod segment plan: one pass for the prefix and one per chain (two per chain of more than 4 stages) up to
        # VJ_MAX_PASSES; beyond it {prefix, rest}; without a prefix of two stages one pass over the whole sweep order
        assert passes("st_c3", n) == [(0, 3), (3, 5), (5, 7), (7, 9)]
        assert passes("st_c4", n) == [(0, 3), (3, 5), (5, 7), (7, 9), (9, 11)]
        assert passes("st_c3long", n) == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 15), (15, 18), (18, 21)]
        assert passes("st_c4long", n) == [(0, 3), (3, 27)]
        assert passes("st_root", n) == [(0, 6)] and passes("st_p1", n) == [(0, 7)]
        assert passes("st_64", n) == [(0, 3), (3, 6), (6, 33), (33, 36), (36, 64)]
        assert len(passes("st_c5", n)) == 6 and passes("st_nested", n) == [(0, 3), (3, 10)]
        assert passes("st_dead", n) == [(0, 3), (3, 5), (5, 7), (7, 9)]          # the sweep order drops the unreachable stage
    # CascadeArgs::seg_end[4]: the tiles run up to four chains themselves (tile_segments), with five they leave after the prefix
    def tile_stages(cid, *settings):
        with tunables(env, *settings):
            r = env.detect(cascade(cid)[1], frames_of(cid), default_params(flags=VJ_FLAG_COUNTERS))
        return [s for s in range(len(r.stage_entered)) if entered_by(r, "tile", s)]
    assert tile_stages("st_c3") == list(range(9)) and tile_stages("st_c4") == list(range(11))
    assert tile_stages("st_c5") == [0, 1, 2] and tile_stages("st_c4", ("tile_segments", 0)) == [0, 1, 2]
    # the OpenCV profile: the tiles run the prefix; up to CvChainDev::begin[4] chains take the chain pass over the tree queue
    # (tree_queue 1), more take the flat queue (2)
    for cid, prefix in (("st_root", 0), ("st_p1", 1), ("st_c3", 3), ("st_c4", 3), ("st_c5", 3), ("st_c4long", 3)):
        h, w = topology_cell(cid)[2]
        assert env.cv_plan_info(cascade(cid)[1], w, h, ARITH_FRAMES).tree_prefix == prefix, cid
    h, w = topology_cell("st_c4")[2]
    assert env.cv_plan_info(cascade("st_c4")[1], w, h, ARITH_FRAMES).tree_queue == 1
    assert env.cv_plan_info(cascade("st_c5")[1], w, h, ARITH_FRAMES).tree_queue == 2
    # the tile plan's wave-independent tail (stages of at most TILE_SP_MAX_BLOCKS * TILE_SP_BLOCK nodes): the public plan of a
    # call does not show it — w256 and w257 get the same shapes and header, and both run above — but the plan dump's former
    # shape search (VJ_PLAN_TILES_FORMER_SHAPES) budgets the tail's tables only where the tail is on
    shapes = {}
    for cid in ("w256", "w257"):
        for flags in (0, VJ_PLAN_TILES_FORMER_SHAPES):
            info, tiles = cascade(cid)[1].plan_tiles(w, h, ARITH_FRAMES, flags=flags)
            shapes[cid, flags] = (list(info.class_lds), [(t.scale_idx, t.lds_class, t.tile_w, t.tile_h) for t in tiles])
    assert shapes["w256", 0] == shapes["w257", 0]
    assert shapes["w256", VJ_PLAN_TILES_FORMER_SHAPES] != shapes["w257", VJ_PLAN_TILES_FORMER_SHAPES]


# ------------------------------------------------------------------------------------------------ refusals
def refused_calls(env, lib, c, good, frames):
    """[(name, call() -> (return code, the result came back empty))] of every entry point that plans `c`."""
    imgs, n, keep = env._images(frames, False)
    h, w = frames[0].shape
    p, cp = default_params(), CvParams(0, 0, 1.1, 0, 0)
    roi = np.array([[0, 0, 0, w, h]], np.int32)
    wl = np.zeros(1, WINDOW_DTYPE)

    def result_call(fn, *args):
        def call():
            res = _Result()
            res.count = 7
            rc = fn(*args, C.byref(res))
            return rc, res.count == 0 and not res.rects
        return call

    def roc_call():
        res = _RocResult()
        res.r.count = 7
        rc = lib.vj_detect_opencv_roc(env._h, c._h, imgs, n, C.byref(CvRocParams(0, 0, 0, 0, 1.1, 0, VJ_FLAG_CV_SCALE_IMAGE)), C.byref(res))
        return rc, res.r.count == 0 and not res.r.rects and not res.reject_levels and not res.level_weights

    def chain_call(first, second):
        def call():
            r1, r2 = _Result(), _Result()
            r1.count = r2.count = 7
            rc = lib.vj_detect_chain(env._h, first._h, second._h, imgs, n, C.byref(p), C.byref(p), C.byref(r1), C.byref(r2))
            empty = r1.count == 0 and not r1.rects and r2.count == 0 and not r2.rects
            lib.vj_result_free(C.byref(r1))
            lib.vj_result_free(C.byref(r2))
            return rc, empty
        return call

    def windows_call(name, dtype, scale_dtype, flags):
        def call():
            out = np.frombuffer(b"\xf9" * dtype.itemsize, dtype).copy()
            before = out.tobytes()
            sc = np.ones(1, scale_dtype)
            rc = getattr(lib, name)(env._h, c._h, imgs, n, sc.ctypes.data, 1, wl.ctypes.data, 1, 0, *flags, out.ctypes.data)
            return rc, out.tobytes() == before
        return call

    def stream_call():
        h_ = C.c_void_p(7)
        rc = lib.vj_stream_create(env._h, c._h, w, h, 1, 2, C.byref(p), C.byref(h_))
        return rc, not h_.value

    return [("vj_detect", result_call(lib.vj_detect, env._h, c._h, imgs, n, C.byref(p))),
            ("vj_detect_opencv", result_call(lib.vj_detect_opencv, env._h, c._h, imgs, n, C.byref(cp))),
            ("vj_detect_opencv_roc", roc_call),
            ("vj_run_windows", windows_call("vj_run_windows", CLOD_WINDOW_RESULT_DTYPE, np.float32, (0,))),
            ("vj_run_windows_opencv", windows_call("vj_run_windows_opencv", WINDOW_RESULT_DTYPE, np.float64, ())),
            ("vj_detect_rois", result_call(lib.vj_detect_rois, env._h, c._h, imgs, n, roi.ctypes.data, 1, C.byref(p))),
            ("vj_detect_opencv_rois", result_call(lib.vj_detect_opencv_rois, env._h, c._h, imgs, n, roi.ctypes.data, 1, C.byref(cp))),
            ("vj_detect_chain first", chain_call(c, good)),
            ("vj_detect_chain second", chain_call(good, c)),
            ("vj_stream_create", stream_call)]


@pytest.mark.parametrize("cid,code", [("lin65", VJ_ERR_LIMIT), ("st_cycle", VJ_ERR_UNSUPPORTED)])
def test_refusals_leave_the_result_empty_and_the_environment_usable(env, lib, oracle, cid, code):
    """More than VJ_MAX_STAGES stages: VJ_ERR_LIMIT from plan_clod, plan_cv, get_cv_roi_plan and run_points; a cycle of the
    pass / fail graph: VJ_ERR_UNSUPPORTED wherever stage_sweep_order is asked.  After every refusal a valid call on the same
    environment gives the oracle's result."""
    c = cascade_to_product(topology_cascade(cid))
    good_a, good = cascade("st_c3" if cid == "st_cycle" else "lin64")
    good_id = "st_c3" if cid == "st_cycle" else "lin64"
    frames = frames_of(good_id)[:2]
    want = oracle_of(oracle, good_id, "clod")[:2]
    want_cv = oracle_of(oracle, good_id, "cv")[:2]
    for name, call in refused_calls(env, lib, c, good, frames):
        rc, empty = call()
        assert rc == code, f"{cid}: {name} returned {rc}"
        assert empty, f"{cid}: {name} left something in its result"
        if name.endswith("opencv") or "opencv_" in name:
            r = env.detect_opencv(good, frames)
            assert [srows(r.rects[r.rects["frame"] == i]) for i in range(2)] == [srows(w_) for w_, _ in want_cv], f"{cid}: after {name}"
        else:
            r = env.detect(good, frames)
            assert [srows(r.rects[r.rects["frame"] == i]) for i in range(2)] == [srows(w_) for w_, _ in want], f"{cid}: after {name}"


def test_reject_levels_at_both_ends_of_the_stage_count(env):
    """vj_detect_opencv_roc refuses lin3 (fewer than 4 stages: VJ_ERR_UNSUPPORTED, vj_detect_opencv_roc's own check) and takes
    lin64, whose levels lie in 61 .. 64: a pass is 64, rejects come from stages 62 and 63 (stage 61 accepts every window)."""
    _, c3 = cascade("lin3")
    with pytest.raises(VjError) as ei:
        env.detect_opencv_roc(c3, frames_of("lin3")[:1])
    assert ei.value.code == VJ_ERR_UNSUPPORTED
    a, c = cascade("lin64")
    for n in BATCHES:
        fr = frames_of("lin64")[:n]
        r = env.detect_opencv_roc(c, fr)
        for f in range(n):
            ro_r, ro_lv, ro_lw, _ = timed(ro.detect_roc, a, fr[f])
            sel = r.rects["frame"] == f
            got = [(int(x["scale_idx"]), int(x["y"]), int(x["x"]), int(x["w"]), int(x["h"]), int(l), int(b))
                   for x, l, b in zip(r.rects[sel], r.reject_levels[sel], r.level_weights[sel].view(np.uint64))]
            assert got == [(int(x["scale_idx"]), int(x["y"]), int(x["x"]), int(x["w"]), int(x["h"]), int(l), int(b))
                           for x, l, b in zip(ro_r, ro_lv, ro_lw.view(np.uint64))], f"frame {f}"
        assert {62, 63, 64} <= set(r.reject_levels.tolist()) <= {61, 62, 63, 64}
