"""The OpenCV-profile modes on survivor- and candidate-heavy content, against their restatements frame by frame: find-biggest
(cv_biggest_pass, cv_biggest_update's device grouping on lists of up to GROUP_MAX candidates, the segment's regrow inside the
scanROI, the VJ_ERR_LIMIT return), scale image (cv_tile_pass<3> and the rows with every grid position alive past the prefix, the
detection buffer's growth), canny pruning on frames where the prune bites, and the plain path's linear forms they are all
compared with.  The cells and their premises: tests/heavy_cases.py, checked on the CPU in tests/test_cv_modes_heavy_cpu.py.
Every comparison is exact."""
import numpy as np
import pytest

import canny_oracle as co
import heavy_cases as hc
import scale_image_oracle as so
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH,
                                 VJ_FLAG_CV_SCALE_IMAGE, Environment, VjError)
from test_gpu_find_biggest import _check as fb_check
from test_gpu_find_biggest import got_rows

pytestmark = pytest.mark.gpu
FB, SI, PRUNE = VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_CV_CANNY_PRUNING
ORACLE_CAP = 1 << 21
_CANON = {}


def same(r, base):
    return np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered


# ----------------------------------------------------------------------------- 1. find-biggest
def fb_flags(kw):
    return FB | (VJ_FLAG_CV_ROUGH_SEARCH if kw.get("rough") else 0)


def fb_args(mn, kw):
    return {"min_neighbors": mn, **{k: v for k, v in kw.items() if k != "rough"}}


@pytest.mark.parametrize("cid", list(hc.FB_CELLS))
def test_find_biggest_heavy_lists(env, cid):
    """One frame per cell: 94 to 2032 candidates grouped on the device at the hit (the bitonic sort up to P = 2048, two rounds of
    block_rank, many classes), every form, rough search and scale_factor 1.25."""
    form, spec, mn, kw, _ = hc.FB_CELLS[cid]
    c, a = hc.product(form)
    frames = hc.frame_of(spec)[None]
    r, want = fb_check(env, c, a, frames, flags=fb_flags(kw), **fb_args(mn, kw))
    assert want == [(0,) + tuple(hc.biggest(form, spec, mn, **kw)[0])]
    r0 = env.detect_opencv(c, frames, flags=fb_flags(kw), **fb_args(mn, kw))      # uncounted: other kernel instantiations
    assert np.array_equal(r0.rects, r.rects)
    if cid in hc.ROI_OVERFLOW_CELLS:
        assert want[0][5] > hc.FB_SEGMENT


@pytest.mark.parametrize("cid", list(hc.TIE_CELLS))
def test_find_biggest_tie_takes_the_first_class(env, cid):
    form, spec, mn = hc.TIE_CELLS[cid]
    c, a = hc.product(form)
    _, want = fb_check(env, c, a, hc.frame_of(spec)[None], min_neighbors=mn)
    assert len(want) == 1
    batch = np.stack([hc.frame_of(spec), hc.frame_of(spec)[::-1].copy(), hc.frame_of(spec)])
    _, want3 = fb_check(env, c, a, batch, min_neighbors=mn)
    assert want3[0][1:] == want[0][1:] and want3[-1] == (2,) + want[0][1:]


@pytest.mark.parametrize("cid", hc.ROI_OVERFLOW_CELLS)
def test_find_biggest_scan_roi_overflows_the_segment(cid):
    """More than 4096 candidates inside the scanROI at the default det_cap: the segment overflows in phase 1, the sub-batch repeats
    with a grown buffer, and the neighbors count of several thousand is the restatement's.  A fresh environment, so that every
    buffer starts at its initial size."""
    form, spec, mn, kw, _ = hc.FB_CELLS[cid]
    env = Environment(0)
    try:
        assert int(env.query("det_cap")) == hc.DET_CAP_INIT
        c, a = hc.product(form)
        f = hc.frame_of(spec)
        _, want = fb_check(env, c, a, f[None], min_neighbors=mn)
        assert len(want) == 1 and want[0][5] > hc.FB_SEGMENT
        r, want2 = fb_check(env, c, a, np.stack([f, hc.frame_of(("synth", "noise", 41) + f.shape), f]), min_neighbors=mn)
        assert want2[0][1:] == want[0][1:] and len(want2) >= 2
        assert got_rows(env.detect_opencv(c, f[None], flags=FB, min_neighbors=mn)) == want == got_rows(r)[:1]
    finally:
        env.close()


def test_find_biggest_mixed_batch(env):
    """Frames of every regime in one call: the batch's result is the frames' own results concatenated, whatever the sub-batching
    and the segment's first size (det_cap 64 regrows several times, 5000 — a segment of 4096 — once)."""
    c, a = hc.product(hc.MIXED_FORM)
    frames = np.stack([hc.frame_of(s) for s in hc.MIXED_FRAMES])
    mn = hc.MIXED_NEIGHBORS
    base, want = fb_check(env, c, a, frames, min_neighbors=mn)
    assert want == [(i,) + tuple(res) for i, s in enumerate(hc.MIXED_FRAMES) for res in [hc.biggest(hc.MIXED_FORM, s, mn)[0]] if res is not None]
    single = []
    for f in range(len(frames)):
        r1, _ = fb_check(env, c, a, frames[f:f + 1], min_neighbors=mn)
        single += [(f,) + row[1:] for row in got_rows(r1)]
    assert single == got_rows(base)
    assert np.array_equal(env.detect_opencv(c, frames, flags=FB, min_neighbors=mn).rects, base.rects)
    for settings in hc.MIXED_SETTINGS:
        with tunables(env, *settings):
            r, _ = fb_check(env, c, a, frames, min_neighbors=mn)
        assert same(r, base), settings
    back = frames[::-1].copy()
    _, want_back = fb_check(env, c, a, back, min_neighbors=mn)
    assert sorted(w[1:] for w in want_back) == sorted(w[1:] for w in want)


@pytest.mark.parametrize("cid", list(hc.LIMIT_CELLS))
def test_find_biggest_limit(env, cid):
    """a frame with more than GROUP_MAX candidates after a whole scale and no group yet returns VJ_ERR_LIMIT, naming
    the frame; the environment serves the next call as before."""
    form, spec, mn, other = hc.LIMIT_CELLS[cid]
    c, a = hc.product(form)
    bad, ok = hc.frame_of(spec), hc.frame_of(other)
    cells = [([bad], 0, ()), ([ok, ok, bad, ok], 2, ()), ([ok, ok, ok, ok, bad], 4, (("max_subbatch", "3"),))]
    for frames, k, settings in cells:
        for flags in (FB | VJ_FLAG_COUNTERS, FB):
            with tunables(env, *settings):
                with pytest.raises(VjError) as ei:
                    env.detect_opencv(c, np.stack(frames), flags=flags, min_neighbors=mn)
            print(f"{cid}: frame {k} of {len(frames)}: {ei.value}")
            assert ei.value.code == hc.VJ_ERR_LIMIT
            assert f"frame {k} holds" in str(ei.value)
        _, want = fb_check(env, c, a, np.stack([ok, ok[::-1].copy()]), min_neighbors=mn)
        assert len(want) >= 1 and want[0][0] == 0


# ----------------------------------------------------------------------------- 2-4. rectangles per frame, counters
def canon(rects):
    """The rectangles' (scale_idx, x, y, w, h) packed into one sorted int64 each."""
    v = [rects[k].astype(np.int64) for k in ("scale_idx", "x", "y", "w", "h")]
    assert len(rects) == 0 or (min(int(x.min()) for x in v) >= 0 and max(int(x.max()) for x in v) < 8192)
    return np.sort((v[0] << 52) | (v[1] << 39) | (v[2] << 26) | (v[3] << 13) | v[4])


def canon_of(ro):
    if id(ro) not in _CANON:
        _CANON[id(ro)] = (ro, canon(ro))      # (keeps ro alive: the id stays its own)
    return _CANON[id(ro)][1]


def check(r, want, label, counted, evals=None):
    """r: the result of a batch; want: [(rects, stats)] of the restatement, one per frame of the batch."""
    n = len(want)
    frame = r.rects["frame"]
    order = np.argsort(frame, kind="stable")
    bounds = np.searchsorted(frame[order], np.arange(n + 1))
    assert bounds[n] == len(frame), f"{label}: rectangles of frames past the batch"
    for i, (ro, _) in enumerate(want):
        mine = canon(r.rects[order[bounds[i]:bounds[i + 1]]])
        assert np.array_equal(mine, canon_of(ro)), f"{label}: frame {i}: {len(mine)} rectangles, the restatement {len(ro)}"
    if counted:
        n_st = len(r.stage_entered)
        entered = [sum(st["stage_entered"][s] for _, st in want) for s in range(n_st)]
        windows = sum(st["windows"] for _, st in want)
        assert r.stage_entered == entered, f"{label}: stage_entered {r.stage_entered}, the restatement {entered}"
        assert r.windows == windows, f"{label}: {r.windows} windows, the restatement {windows}"
        if evals is not None:
            a, every_node = evals
            visited = sum(st["stump_evals"] for _, st in want)
            if all(int(k) == 1 for k in a.tree_n_nodes):
                assert r.stump_evals == visited, label
            elif every_node:     # multi-node trees: the library counts every node of an entered stage, the restatement the visited ones
                assert r.stump_evals == sum(e * k for e, k in zip(entered, hc.nodes_per_stage(a))) >= visited, label


def run_cells(env, c, a, frames, want, flags, label, routes, evals_rule, **kw):
    """Defaults counted and uncounted against the restatement; every other route equal to them, counted and uncounted."""
    counted = env.detect_opencv(c, frames, flags=flags | VJ_FLAG_COUNTERS, **kw)
    check(counted, want, label + " counted", True, None if evals_rule is None else (a, evals_rule))
    timed = env.detect_opencv(c, frames, flags=flags, **kw)
    check(timed, want, label + " uncounted", False)
    for settings in routes:
        with tunables(env, *settings):
            r = env.detect_opencv(c, frames, flags=flags | VJ_FLAG_COUNTERS, **kw)
            assert same(r, counted) and r.stump_evals == counted.stump_evals, f"{label} {settings} counted"
            r = env.detect_opencv(c, frames, flags=flags, **kw)
            assert np.array_equal(r.rects, timed.rects), f"{label} {settings} uncounted"
    return counted, timed


# ----------------------------------------------------------------------------- 2. scale image
SI_ROUTES = ((("cv_tiles", "0"),), (("cv_tile_ws_max", "64"),))


def si_want(form, h, w, n):
    specs = hc.repeat(hc.survivor_specs(h, w), n)
    return [hc.frame_of(s) for s in specs], hc.cached_many(so.detect_scale_image, form, specs, cap=1 << 23)


def si_route(env, c, form, h, w, n):
    info = env.cv_plan_info(c, w, h, n, flags=SI)
    if form in hc.LINEAR_FORMS:
        assert info.n_tile_scales >= 1, f"{form} {h}x{w} n={n}: no scale on LDS tiles"
        with tunables(env, ("cv_tiles", "0")):
            assert env.cv_plan_info(c, w, h, n, flags=SI).n_tile_scales == 0
    else:
        assert info.n_tile_scales == 0, f"{form} {h}x{w} n={n}: a stage tree off the row kernel"


@pytest.mark.parametrize("form", hc.SURVIVOR_FORMS)
def test_scale_image_survivors(env, form):
    """Every grid position of every level alive past the prefix: cv_tile_pass<3>'s finish stages and detection store for the
    linear forms (the plan says so), the row kernel for the stage trees; batches of 1, 7 and 11 of four distinct frames."""
    c, a = hc.product(form)
    for h, w in hc.SIZES:
        if form == "accept_all" and (h, w) != hc.SIZES[0]:
            continue                                   # (every position a rectangle: the larger sizes run below, in a fresh environment)
        for n in hc.BATCHES:
            frames, want = si_want(form, h, w, n)
            si_route(env, c, form, h, w, n)
            routes = SI_ROUTES if form in hc.LINEAR_FORMS else ((("cv_tree_chains", "0"),),)
            run_cells(env, c, a, frames, want, SI, f"scale image {form} {h}x{w} n={n}", routes, True)


@pytest.mark.parametrize("form", hc.SI_BIG[3])
def test_scale_image_survivors_1080p(env, form):
    h, w, n, _ = hc.SI_BIG
    c, a = hc.product(form)
    frames, want = si_want(form, h, w, n)
    si_route(env, c, form, h, w, n)
    run_cells(env, c, a, frames, want, SI, f"scale image {form} {h}x{w} n={n}", (), True)


def test_scale_image_accept_all_grows_the_detection_buffer():
    """602 348 rectangles per 480 x 640 frame, far above det_cap's initial 65 536: the buffer grows, nothing is lost, and the
    result is sorted by (frame, scale_idx, y, x)."""
    env = Environment(0)
    try:
        assert int(env.query("det_cap")) == hc.DET_CAP_INIT
        c, a = hc.product("accept_all")
        for (h, w), batches in (((480, 640), hc.SI_ACCEPT_ALL_BATCHES), ((479, 641), (1,))):
            for n in batches:
                frames, want = si_want("accept_all", h, w, n)
                assert all(len(ro) > hc.DET_CAP_INIT for ro, _ in want)
                si_route(env, c, "accept_all", h, w, n)
                _, timed = run_cells(env, c, a, frames, want, SI, f"scale image accept_all {h}x{w} n={n}", SI_ROUTES[:1], True)
                rr = timed.rects
                key = (rr["frame"].astype(np.int64) << 40) | (rr["scale_idx"].astype(np.int64) << 32) | (rr["y"].astype(np.int64) << 16) | rr["x"]
                assert np.all(np.diff(key) > 0), "not sorted by (frame, scale_idx, y, x)"
    finally:
        env.close()


@pytest.mark.parametrize("form", ("stumps", "chain_tree"))
def test_scale_image_survivors_sub_batches(env, form):
    c, a = hc.product(form)
    h, w, n = 480, 640, 7
    frames, want = si_want(form, h, w, n)
    base = env.detect_opencv(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    with tunables(env, ("max_subbatch", "2")):
        r, _ = run_cells(env, c, a, frames, want, SI, f"scale image {form} max_subbatch 2", (), True)
    assert same(r, base)


# ----------------------------------------------------------------------------- 3. canny pruning
@pytest.mark.parametrize("form", hc.SURVIVOR_FORMS)
def test_canny_pruning_survivors(env, form):
    """Frames on which the prune drops a quarter and more of the windows while every window it keeps passes the prefix:
    cv_profile_pass / cv_tile_pass under the prune bitmap, the tiles and the rows, the stage trees' flat queue too."""
    c, a = hc.product(form)
    routes = ((("cv_tiles", "0"),),) + (((("cv_tree_chains", "0"),),) if form in hc.TREE_FORMS else ())
    for h, w in hc.CANNY_SIZES:
        for n in hc.CANNY_BATCHES:
            specs = hc.repeat(hc.canny_specs(h, w), n)
            want = hc.cached_many(co.detect_opencvlike, form, specs)
            frames = [hc.frame_of(s) for s in specs]
            run_cells(env, c, a, frames, want, PRUNE, f"canny {form} {h}x{w} n={n}", routes, False)


# ----------------------------------------------------------------------------- 4. the plain path, linear forms
_PLAIN = {}


def plain_want(oracle, form, h, w, n):
    specs = hc.repeat(hc.survivor_specs(h, w), n)
    for s in specs:
        if (form, s) not in _PLAIN:
            _PLAIN[(form, s)] = oracle.detect_opencvlike(hc.arrays(form), hc.frame_of(s), cap=ORACLE_CAP)
    return [hc.frame_of(s) for s in specs], [_PLAIN[(form, s)] for s in specs]


@pytest.mark.parametrize("form", hc.LINEAR_FORMS)
def test_plain_opencv_linear_survivors(env, oracle, form):
    """What the three modes share (vj_cv_window.hpp's arithmetic, the tiles, the rows) with no mode on: the linear forms through
    vj_detect_opencv against oracle.detect_opencvlike, next to the stage trees of tests/test_gpu_survivors.py."""
    c, a = hc.product(form)
    for h, w in hc.PLAIN_SIZES:
        for n in hc.PLAIN_BATCHES:
            frames, want = plain_want(oracle, form, h, w, n)
            run_cells(env, c, a, frames, want, 0, f"plain {form} {h}x{w} n={n}", ((("cv_tiles", "0"),),), None)
