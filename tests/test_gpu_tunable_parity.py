"""Every vj_env_configure key at values other than its default, against the C oracle on batches of DISTINCT frames.

include/vj.h promises of the tunables: "speed only: results never depend on them".  cases.TUNABLE_SWEEPS has one row per key
of the table in vj_env.cpp (the guard below fails when a key has none); every (key, value, workload, batch prefix) is a cell:

  1. inside `with tunables(env, ..., (key, value))` the key's query differs from a fresh environment's;
  2. a counted call: rectangles per frame equal the oracle's for THAT frame, summed stage_entered and windows equal the
     oracle's sums, the per-launch stage_entered add up to the totals (clod profile);
  3. the timed (uncounted) call returns the same rectangles;
  4. the key's effect on the plan, wherever the ABI reports the plan (EFFECTS below; TUNABLE_SWEEPS says where it cannot);
  5. after the `with`, every key reads its default again and a default call still equals the oracle (plans dropped or
     re-keyed correctly).

Agreement is exact; every frame, stage and scale is compared."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cases import (CONFIGURE_ACTIONS, TUNABLE_KINDS, TUNABLE_SWEEPS, TUNABLE_WORKLOADS, check_against_oracle, configure_keys,
                   first_difference, rows_of, tunables)
from clfacedetection_amd import VJ_FLAG_COUNTERS, default_params, synth

gpu = pytest.mark.gpu


# ----------------------------------------------------------------------------- the guard (no GPU)
def test_every_configure_key_has_a_sweep_row():
    keys = set(configure_keys()) - set(CONFIGURE_ACTIONS)
    assert set(TUNABLE_SWEEPS) == keys, (sorted(keys - set(TUNABLE_SWEEPS)), sorted(set(TUNABLE_SWEEPS) - keys))
    for key, sweeps in TUNABLE_SWEEPS.items():
        assert len(sweeps) >= 1, key
        for sw in sweeps:
            assert len(sw.values) >= 1 and len(sw.workloads) >= 1, key
            assert all(isinstance(v, str) for v in sw.values), key
            assert set(sw.workloads) <= set(TUNABLE_WORKLOADS), (key, sw.workloads)
            assert all(k in keys and k != key for k, _ in sw.also), (key, sw.also)
    for name, (api, cascs, sizes, prefixes, seed0) in TUNABLE_WORKLOADS.items():
        assert api in ("clod", "cv", "chain") and cascs and sizes and prefixes == tuple(sorted(prefixes)), name


# ----------------------------------------------------------------------------- frames and oracle results, once per module
_FRAMES, _ORACLE, _DEFAULTS, _BASE = {}, {}, {}, {}
_SECONDS = {"oracle": 0.0}
REGION_SECOND = "eye"                  # regions: frontalface_alt2's grouped faces, then haarcascade_eye inside each
REGION_MIN_NEIGHBORS = 3


@pytest.fixture(scope="module", autouse=True)
def oracle_seconds():
    yield
    print(f"\ntest_gpu_tunable_parity: {_SECONDS['oracle']:.1f} s of this module went to the CPU oracle")


def frame_set(wl, size):
    """The workload's distinct frames of one size; every batch is a prefix of them."""
    if (wl, size) not in _FRAMES:
        _, _, _, prefixes, seed0 = TUNABLE_WORKLOADS[wl]
        _FRAMES[wl, size] = synth.batch(max(prefixes), size[0], size[1], seed0=seed0 + size[0] % 100, kinds=TUNABLE_KINDS)
    return _FRAMES[wl, size]


def oracle_set(oracle, cascades, api, casc, wl, size, n):
    """[(rects, stats)] of the oracle for the first n frames of a set, each frame computed once per module (the C entry
    points release the GIL: the frames run side by side)."""
    have = _ORACLE.setdefault((api, casc, wl, size), {})
    missing = [i for i in range(n) if i not in have]
    if missing:
        _, a = cascades(casc)
        frames = frame_set(wl, size)
        fn = oracle.detect if api == "clod" else oracle.detect_opencvlike
        t0 = time.time()
        with ThreadPoolExecutor(8) as ex:
            for i, res in zip(missing, ex.map(lambda i: fn(a, frames[i]), missing)):
                have[i] = res
        _SECONDS["oracle"] += time.time() - t0
    return [have[i] for i in range(n)]


def regions_oracle(oracle, cascades, casc, wl, size, n):
    """Per frame: (the oracle's grouped faces [(x, y, w, h, neighbours)], the oracle's (rects, stats) of the second cascade
    on each face's sub-image)."""
    raw = oracle_set(oracle, cascades, "clod", casc, wl, size, n)
    have = _ORACLE.setdefault(("chain", casc, wl, size), {})
    frames = frame_set(wl, size)
    _, eye_a = cascades(REGION_SECOND)
    t0 = time.time()
    for f in range(n):
        if f in have:
            continue
        ro = raw[f][0]
        xywh = np.stack([ro[k] for k in ("x", "y", "w", "h")], 1) if len(ro) else np.zeros((0, 4), np.int32)
        g, wt = oracle.group_rectangles(xywh, REGION_MIN_NEIGHBORS)
        faces = [(int(q[0]), int(q[1]), int(q[2]), int(q[3]), int(m)) for q, m in zip(g, wt)]
        inside = [oracle.detect(eye_a, np.ascontiguousarray(frames[f][y:y + h, x:x + w])) for x, y, w, h, _ in faces]
        have[f] = (faces, inside)
    _SECONDS["oracle"] += time.time() - t0
    return [have[f] for f in range(n)]


def fresh_defaults(env):
    """key -> query of an environment at its shipped values."""
    if not _DEFAULTS:
        env.configure("defaults", "")
        _DEFAULTS.update({k: env.query(k) for k in TUNABLE_SWEEPS})
    return _DEFAULTS


# ----------------------------------------------------------------------------- one call against the oracle, per API
def check_cv(env, c, frames, want, label):
    """vj_detect_opencv, counted and timed, against the oracle's per-frame results (a stage tree's counted call walks the
    rows and its timed call takes the tiles and the tree queue: each is compared with the oracle itself)."""
    r = env.detect_opencv(c, frames, flags=VJ_FLAG_COUNTERS)
    r2 = env.detect_opencv(c, frames)
    entered, windows = [0] * c.info.n_stages, 0
    for i, (ro, st) in enumerate(want):
        for which, res in (("counted", r), ("timed", r2)):
            mine = sorted(rows_of(res.rects[res.rects["frame"] == i]))
            assert mine == sorted(rows_of(ro)), f"{label}: {which} call, frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: {first_difference(r.stage_entered, entered)}"
    assert r.windows == windows, f"{label}: {r.windows} windows visited, the oracle {windows}"
    assert len(r.rects) == len(r2.rects) == sum(len(ro) for ro, _ in want), f"{label}: rectangles outside the batch's frames"
    return r


def check_chain(env, c, eye, frames, want, label):
    """vj_detect_chain (faces grouped on the device, the second cascade inside each, counted and timed) and vj_detect_rois
    on the same regions, against the oracle's grouping and the oracle on every sub-image."""
    p1, p2 = default_params(min_neighbors=REGION_MIN_NEIGHBORS), default_params(flags=VJ_FLAG_COUNTERS)
    r1, r2 = env.detect_chain(c, eye, frames, p1, p2)
    faces = [(x, y, w, h, m, f) for f, (fs, _) in enumerate(want) for x, y, w, h, m in fs]
    inside = [res for _, ins in want for res in ins]
    assert len(faces) > 0, f"{label}: the frames give no grouped face, so no region was exercised"
    got = [(int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"]), int(q["weight"]), int(q["frame"])) for q in r1.rects]
    assert got == faces, f"{label}: {len(got)} grouped faces, the oracle {len(faces)}"
    rois = [(f, x, y, w, h) for x, y, w, h, _, f in faces]
    host = env.detect_rois(eye, frames, rois, p2)
    entered, windows = [0] * eye.info.n_stages, 0
    for i, (ro, st) in enumerate(inside):
        for which, res in (("vj_detect_chain", r2), ("vj_detect_rois", host)):
            mine = rows_of(res.rects[res.rects["frame"] == i])
            assert mine == rows_of(ro), f"{label}: {which}, region {i} {rois[i]}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    for which, res in (("vj_detect_chain", r2), ("vj_detect_rois", host)):
        assert res.stage_entered == entered, f"{label}: {which}: {first_difference(res.stage_entered, entered)}"
        assert res.windows == windows, f"{label}: {which}: {res.windows} windows, the oracle {windows}"
        assert len(res.rects) == sum(len(ro) for ro, _ in inside), f"{label}: {which}: rectangles outside the regions"
    t1, t2 = env.detect_chain(c, eye, frames, p1, default_params())
    assert np.array_equal(t1.rects, r1.rects) and np.array_equal(t2.rects, r2.rects), f"{label}: the timed call's rectangles differ"
    assert np.array_equal(env.detect_rois(eye, frames, rois).rects, host.rects), f"{label}: the timed vj_detect_rois differs"
    return r2


def run_check(env, cascades, api, c, frames, want, label):
    if api == "clod":
        return check_against_oracle(env, c, frames, want, label)[0]
    if api == "cv":
        return check_cv(env, c, frames, want, label)
    return check_chain(env, c, cascades(REGION_SECOND)[0], frames, want, label)


def default_call_matches(env, cascades, api, c, frames, want, label):
    """One timed call at the defaults, after a sweep: the plans were dropped or re-keyed, not left as the setting made them."""
    if api == "chain":
        r1, _ = env.detect_chain(c, cascades(REGION_SECOND)[0], frames, default_params(min_neighbors=REGION_MIN_NEIGHBORS))
        got = [(int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"]), int(q["weight"])) for q in r1.rects]
        assert got == [face for fs, _ in want for face in fs], f"{label}: the default call after the sweep differs from the oracle"
        return
    r = env.detect(c, frames) if api == "clod" else env.detect_opencv(c, frames)
    for i, (ro, _) in enumerate(want):
        assert sorted(rows_of(r.rects[r.rects["frame"] == i])) == sorted(rows_of(ro)), \
            f"{label}: frame {i} of the default call after the sweep differs from the oracle"
    assert len(r.rects) == sum(len(ro) for ro, _ in want), label


class Base:
    """What a call at the defaults reports about its plan (the effect assertions compare with it)."""
    def __init__(self, env, api, c, frames, size):
        self.passes, self.launches, self.cv = [], [], None
        if api == "clod":
            r = env.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS))
            self.passes, self.launches = bounds_of(r), r.launches
        elif api == "cv":
            info = env.cv_plan_info(c, size[1], size[0], len(frames))
            self.cv = (info.n_tile_scales, info.tree_queue)


def base_of(env, api, c, casc, wl, size, n, frames):
    k = (api, casc, wl, size, n)
    if k not in _BASE:
        env.configure("defaults", "")
        _BASE[k] = Base(env, api, c, frames, size)
    return _BASE[k]


# ----------------------------------------------------------------------------- a setting must be shown to have taken effect
def bounds_of(r):
    return [(b, e) for b, e, _ in r.passes]


def tile_scales(launches):
    return sorted(set().union(*[l["scales"] for l in launches if l["kind"] == "tile"]))


def kinds_of(launches):
    return [l["kind"] for l in launches]


def queue_entered(launches):
    return sum(sum(l["stage_entered"]) for l in launches if l["kind"] == "queue")


def stage_nodes(c):
    """Nodes per stage, as the plan counts them (build_stage_program)."""
    tr = c.trees
    return [int(tr["n_nodes"][s["first_tree"]:s["first_tree"] + s["n_trees"]].sum()) for s in c.stages]


def cut_rule(c, cuts):
    """default_pass_bounds (vj_clod_plan.cpp) for a linear cascade: a boundary after the stage at which the cumulative node count
    reaches each value of pass_cut_nodes (compared as unsigned: -1 is never reached)."""
    nodes, n = stage_nodes(c), c.info.n_stages
    cuts = [v % (1 << 32) for v in cuts]
    b, acc, ci = [0], 0, 0
    for s in range(n):
        if ci >= len(cuts):
            break
        acc += nodes[s]
        if acc >= cuts[ci] and s + 1 < n:
            b.append(s + 1)
            while ci < len(cuts) and acc >= cuts[ci]:
                ci += 1
    b.append(n)
    return list(zip(b[:-1], b[1:]))


def seg_cut2_rule(base, v, max_passes=8):
    """plan_clod's passes of a stage tree whose part after the prefix is chains of more than four stages (each cut after its
    third stage): a chain longer than v + 4 stages gets one more boundary at its start + v when v > 3 and launches are left."""
    assert len(base) >= 3 and len(base) % 2 == 1 and all(base[i][1] - base[i][0] == 3 for i in range(1, len(base), 2)), base
    chains = [(base[i][0], base[i + 1][1]) for i in range(1, len(base), 2)]
    b = [0, base[0][1]]
    for k, (cb, ce) in enumerate(chains):
        b.append(cb + 3)
        if v > 3 and ce - cb > v + 4 and len(b) + 2 * (len(chains) - (k + 1)) + 1 < max_passes:
            b.append(cb + v)
        b.append(ce)
    return list(zip(b[:-1], b[1:]))


def effect_one_pass(x):
    n_st = x.c.info.n_stages
    print(f"\n{x.label}: passes {bounds_of(x.r)} (defaults: {x.base.passes}), launches {kinds_of(x.r.launches)}")
    if x.n <= int(x.value):
        assert bounds_of(x.r) == [(0, n_st)], f"{x.label}: the gather chain is not one pass: {bounds_of(x.r)}"
        grids = [l for l in x.r.launches if l["kind"] == "grid"]
        assert "queue" not in kinds_of(x.r.launches) and len(grids) == 1, f"{x.label}: launches {kinds_of(x.r.launches)}"
        assert (grids[0]["stage_begin"], grids[0]["stage_end"]) == (0, n_st), x.label
        assert len(x.base.passes) > 1, f"{x.label}: the default plan is one pass already"
    else:   # more frames than the value: get_plan refuses
        assert bounds_of(x.r) == x.base.passes, f"{x.label}: passes {bounds_of(x.r)}, the defaults' {x.base.passes}"


def effect_seg_cut2(x):
    want = seg_cut2_rule(x.base.passes, int(x.value))
    print(f"\n{x.label}: passes {bounds_of(x.r)} (defaults: {x.base.passes})")
    assert bounds_of(x.r) == want, f"{x.label}: passes {bounds_of(x.r)}, by the rule {want}"
    if x.value in ("8", "4"):
        assert len(want) > len(x.base.passes), f"{x.label}: no chain is long enough for the second cut"
        assert queue_entered(x.r.launches) > 0, x.label
    else:   # 3: not > 3; 40: no chain is longer than 44 stages
        assert want == x.base.passes, x.label


def effect_pass_cut_nodes(x):
    want = cut_rule(x.c, [int(v) for v in x.value.split(",")])
    assert x.base.passes == cut_rule(x.c, [35]), f"{x.label}: the default passes {x.base.passes} are not the rule's for 35"
    assert bounds_of(x.r) == want, f"{x.label}: passes {bounds_of(x.r)}, by the rule {want}"
    assert want != x.base.passes, f"{x.label}: the value cuts where 35 does"


def effect_tile_scales_differ(x):
    assert tile_scales(x.r.launches) != tile_scales(x.base.launches), \
        f"{x.label}: the tile scales are the defaults' {tile_scales(x.base.launches)}"


def effect_queue_pass_ran(x):
    assert queue_entered(x.r.launches) > 0, f"{x.label}: no queue launch entered a window: {kinds_of(x.r.launches)}"


def effect_chains_overlap(x):
    effect_queue_pass_ran(x)
    assert {"tile", "grid"} <= set(kinds_of(x.r.launches)), f"{x.label}: no tile launch next to the gather chain"


def effect_cv_tile_scales_differ(x):
    info = x.env.cv_plan_info(x.c, x.size[1], x.size[0], x.n)
    assert info.n_tile_scales != x.base.cv[0], f"{x.label}: {info.n_tile_scales} tile scales, as at the defaults"


def effect_cv_tree_queue(x):
    info = x.env.cv_plan_info(x.c, x.size[1], x.size[0], x.n)
    want = 2 if ("cv_tree_chains", "0") in x.also else 1
    assert x.base.cv[1] == 1, f"{x.label}: the default plan has no chain pass over the tree queue (tree_queue {x.base.cv[1]})"
    assert info.tree_queue == want, f"{x.label}: tree_queue {info.tree_queue}, expected {want}"


EFFECTS = {
    "one_pass_max_frames": effect_one_pass, "seg_cut2": effect_seg_cut2, "pass_cut_nodes": effect_pass_cut_nodes,
    "tile_accept_windows": effect_tile_scales_differ, "cv_tile_min_windows_tree": effect_cv_tile_scales_differ,
    "gather_waves": effect_queue_pass_ran, "q_slices": effect_queue_pass_ran, "concurrent_blocks_per_cu": effect_chains_overlap,
    "cv_tree_chunk": effect_cv_tree_queue, "cv_tree_chain_blocks": effect_cv_tree_queue, "cv_row_blocks_tree": effect_cv_tree_queue,
}


class Cell:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def cells():
    out = []
    for key, sweeps in TUNABLE_SWEEPS.items():
        for sw in sweeps:
            for value in sw.values:
                for wl in sw.workloads:
                    _, cascs, sizes, prefixes, _ = TUNABLE_WORKLOADS[wl]
                    also = "".join(f"+{k}={v}" for k, v in sw.also)
                    out += [pytest.param(key, value, sw.also, wl, casc, size, n,
                                         id=f"{key}={value or 'empty'}{also}-{wl}-{casc}-{size[0]}x{size[1]}-n{n}")
                            for casc in cascs for size in sizes for n in prefixes]
    return out


def run_cell(env, oracle, cascades, settings, key, value, also, wl, casc, size, n, effect):
    api = TUNABLE_WORKLOADS[wl][0]
    c, _ = cascades(casc)
    frames = frame_set(wl, size)[:n]
    if api == "chain":
        want = regions_oracle(oracle, cascades, casc, wl, size, n)
    else:
        want = oracle_set(oracle, cascades, api, casc, wl, size, n)
    label = f"{casc} {size[0]}x{size[1]} n={n} " + " ".join(f"{k}={v}" for k, v in settings)
    shipped = fresh_defaults(env)
    base = base_of(env, api, c, casc, wl, size, n, frames)
    with tunables(env, *settings):
        if key is not None:
            assert env.query(key) != shipped[key], f"{label}: {key} reads {env.query(key)!r}, its default"
        r = run_check(env, cascades, api, c, frames, want, label)
        if effect is not None:
            effect(Cell(env=env, c=c, r=r, base=base, n=n, value=value, also=also, size=size, label=label))
    assert {k: env.query(k) for k in shipped} == shipped, f"{label}: not every key is back at its default"
    default_call_matches(env, cascades, api, c, frames, want, label)


@gpu
@pytest.mark.parametrize("key,value,also,wl,casc,size,n", cells())
def test_tunable_value_matches_the_oracle(env, oracle, cascades, key, value, also, wl, casc, size, n):
    run_cell(env, oracle, cascades, (*also, (key, value)), key, value, also, wl, casc, size, n, EFFECTS.get(key))


@gpu
@pytest.mark.parametrize("wl,casc,size,n", [pytest.param(wl, casc, size, n, id=f"{wl}-{casc}-{size[0]}x{size[1]}-n{n}")
                                            for wl, (_, cascs, sizes, prefixes, _) in TUNABLE_WORKLOADS.items()
                                            for casc in cascs for size in sizes for n in prefixes])
def test_the_workloads_match_the_oracle_at_the_defaults(env, oracle, cascades, wl, casc, size, n):
    """The same cell with nothing set: what every sweep is measured against, and the dry run that sizes the file's time."""
    run_cell(env, oracle, cascades, (), None, None, (), wl, casc, size, n, None)


# one_pass_max_frames is refused by plan_clod for cascades of multi-node trees, for stage trees and under a pass_split, and
# by get_plan below 800000 pixels: the passes are the ones without it, and the result is the oracle's all the same
ONE_PASS_REFUSALS = [  # (id, cascade, workload whose frames are used, size, other settings)
    ("two_node_trees", "frontalface_alt2", "lin_few", (720, 1280), ()),
    ("stage_tree", "frontalface_alt_tree", "lin_few", (720, 1280), ()),
    ("pass_split", "frontalface_alt", "lin_few", (720, 1280), (("pass_split", "3,9"),)),
    ("below_800000_px", "frontalface_alt", "lin_batch", (479, 641), ()),
]


@gpu
@pytest.mark.parametrize("rid,casc,wl,size,other", ONE_PASS_REFUSALS, ids=[r[0] for r in ONE_PASS_REFUSALS])
def test_one_pass_refusals_keep_the_default_passes(env, oracle, cascades, rid, casc, wl, size, other):
    c, _ = cascades(casc)
    frames = frame_set(wl, size)[:1]
    want = oracle_set(oracle, cascades, "clod", casc, wl, size, 1)
    label = f"{casc} {size[0]}x{size[1]} n=1 one_pass_max_frames=4 " + " ".join(f"{k}={v}" for k, v in other)
    with tunables(env, *other):
        without, _ = check_against_oracle(env, c, frames, want, label + " (without the key)")
    with tunables(env, *other, ("one_pass_max_frames", "4")):
        r, _ = check_against_oracle(env, c, frames, want, label)
    assert bounds_of(r) == bounds_of(without) and len(bounds_of(r)) > 1, f"{label}: passes {bounds_of(r)}, without the key {bounds_of(without)}"
    assert kinds_of(r.launches) == kinds_of(without.launches), label
    default_call_matches(env, cascades, "clod", c, frames, want, label)
