"""The premises of tests/test_gpu_topologies.py, on the CPU: the cascades of cases.TOPOLOGY_CELLS — stage counts, stage widths,
node trees and stage trees on each side of the planners' and kernels' fixed-size assumptions — really exercise what their names
say, on the oracle alone and in both profiles: every reachable stage is entered by at least MIN_ENTERED windows of the cell's
frames, an unreachable one by none, the frames give at least MIN_RECTS rectangles and fewer than a tenth of the windows, every
chain of a stage tree decides something, and the decisive stage of a wide cell passes and rejects.  The counts are conditions
on the inputs (change a spot, a threshold or a seed if one fails, not the bound).  The straddle test reads the limits from the
headers and fails when the table no longer has a case on each side of each of them; the planner tests run the host-only tile
plan of every case and the two refusals."""
import os
import re

import numpy as np
import pytest

from cases import (ARITH_FRAMES, TOPOLOGY_CELLS, TOPOLOGY_RUNNABLE, TOPOLOGY_WIDE_STAGE, cascade_to_product, linked_linearly,
                   reachable_stages, stage_links, topology_cascade, topology_cell, topology_chains, topology_frames, topology_passes,
                   without_chain)
from clfacedetection_amd import VjError
from clfacedetection_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_ENTERED, MIN_RECTS = 64, 10
VJ_ERR_UNSUPPORTED, VJ_ERR_LIMIT = 4, 8
RUNNABLE_IDS = [c[0] for c in TOPOLOGY_RUNNABLE]
STAGE_TREES = [c[0] for c in TOPOLOGY_RUNNABLE if c[1] == "stage_tree"]
_TOTALS = {}


def rows(r):
    return sorted(tuple(int(q[k]) for k in ("scale_idx", "x", "y", "w", "h")) for q in r)


def run(oracle, a, frames, profile):
    """(rectangle rows per frame, stages entered over the frames, windows over the frames)."""
    out, entered, windows = [], np.zeros(a.n_stages, np.int64), 0
    for f in frames:
        r, st = oracle.detect(a, f, mode=None if np.all(a.stage_next == -1) else 1) if profile == "clod" else oracle.detect_opencvlike(a, f)
        out.append(rows(r))
        entered += np.array(st["stage_entered"], np.int64)
        windows += st["windows"]
    return out, entered, windows


def totals(oracle, cid, profile):
    if (cid, profile) not in _TOTALS:
        _TOTALS[cid, profile] = run(oracle, topology_cascade(cid), topology_frames(topology_cell(cid)), profile)
    return _TOTALS[cid, profile]


def test_the_table_names_every_case_once():
    ids = [c[0] for c in TOPOLOGY_CELLS]
    assert len(set(ids)) == len(ids) and [c[0] for c in TOPOLOGY_CELLS if not c[4]] == ["lin65", "st_cycle"]
    for cid, family, size, seed, runnable in TOPOLOGY_CELLS:
        a = topology_cascade(cid)
        assert (a.win_w, a.win_h) == (20, 20) and len(topology_frames(topology_cell(cid))) == ARITH_FRAMES
        lv = a.alpha.astype(np.float64) * 64.0                   # leaves: multiples of 2^-6 of magnitude <= 2
        assert np.array_equal(lv, np.rint(lv)) and np.abs(a.alpha).max() <= 2.0, cid
        assert bool(np.any(a.stage_next != -1)) == (family == "stage_tree"), cid


@pytest.mark.parametrize("profile", ["clod", "cv"])
@pytest.mark.parametrize("cid", RUNNABLE_IDS)
def test_every_reachable_stage_is_entered_and_rectangles_are_few(oracle, cid, profile):
    a = topology_cascade(cid)
    rects, entered, windows = totals(oracle, cid, profile)
    reach = reachable_stages(a)
    assert reach == set(range(a.n_stages)) or cid == "st_dead"
    for s in range(a.n_stages):
        if s in reach:
            assert entered[s] >= MIN_ENTERED, f"{cid} {profile}: stage {s} is entered by {entered[s]} windows"
        else:
            assert entered[s] == 0, f"{cid} {profile}: the unreachable stage {s} is entered"
    n = sum(len(r) for r in rects)
    assert MIN_RECTS <= n < windows / 10, f"{cid} {profile}: {n} rectangles of {windows} windows"
    assert len(rects[0]) > 0, f"{cid} {profile}: the single frame gives no rectangle"


def test_the_dead_stage_is_the_only_unreachable_one():
    a = topology_cascade("st_dead")
    assert reachable_stages(a) == set(range(a.n_stages - 1))
    on_pass, on_fail = stage_links(topology_cascade("st_cycle"))
    first, last = topology_chains("st_cycle")[0][0], topology_chains("st_cycle")[-1][0]
    assert on_fail[last] == first and on_fail[first] != -2          # the fail edges close a loop


@pytest.mark.parametrize("profile", ["clod", "cv"])
@pytest.mark.parametrize("cid", STAGE_TREES)
def test_every_chain_of_a_stage_tree_decides_something(oracle, cid, profile):
    """The rectangle set differs from that of the same stages in one chain, and taking any one chain out (the `next` that leads
    to it cut and joined to the chain behind it, so the others stay) changes the set as well.  st_root's first chain begins
    with stage 0, where every walk starts: it cannot be taken out, and is covered by the linear comparison."""
    a = topology_cascade(cid)
    frames = topology_frames(topology_cell(cid))
    base = totals(oracle, cid, profile)[0]
    assert run(oracle, linked_linearly(a), frames, profile)[0] != base, f"{cid} {profile}: the links decide nothing"
    chains = topology_chains(cid)
    assert len(chains) >= 2
    for k, (b, e) in enumerate(chains):
        if b == 0:
            continue
        assert run(oracle, without_chain(a, chains, k), frames, profile)[0] != base, f"{cid} {profile}: chain {k} ({b}..{e - 1}) decides nothing"


@pytest.mark.parametrize("profile", ["clod", "cv"])
@pytest.mark.parametrize("cid", ["lin64", "st_64"])
def test_counts_differ_in_the_last_two_slots(oracle, cid, profile):
    """Counter slot 63 and mask bit 63 carry a value that slot 62 does not (st_64: the entered masks exist in the stage-tree
    kernels only)."""
    _, entered, _ = totals(oracle, cid, profile)
    assert len(entered) == 64 and entered[63] != entered[62] and entered[63] > 0 and entered[62] > 0


@pytest.mark.parametrize("profile", ["clod", "cv"])
@pytest.mark.parametrize("cid", [c[0] for c in TOPOLOGY_RUNNABLE if c[1] == "wide"])
def test_wide_stages_pass_and_reject(oracle, cid, profile):
    a = topology_cascade(cid)
    rects, entered, _ = totals(oracle, cid, profile)
    for s in range(TOPOLOGY_WIDE_STAGE, a.n_stages):
        passed = entered[s + 1] if s + 1 < a.n_stages else sum(len(r) for r in rects)
        assert passed >= MIN_ENTERED and entered[s] - passed >= MIN_ENTERED, f"{cid} {profile}: stage {s}: {passed} of {entered[s]} pass"


# ------------------------------------------------------------------------------------------------ both sides of every limit
def header_limits():
    """The fixed sizes, read from the headers the way cases.configure_keys() reads vj_env.cpp."""
    pub = open(os.path.join(ROOT, "include", "vj.h")).read()
    dev = open(os.path.join(ROOT, "clfacedetection_amd", "csrc", "vj_device.hpp")).read()
    out = {k: int(re.search(rf"^#define {k} (\d+)", pub, re.M).group(1)) for k in ("VJ_MAX_STAGES", "VJ_MAX_PASSES")}
    for k in ("TILE_SP_MAX_BLOCKS", "TILE_SP_BLOCK", "CV_TAIL_BLOCKS"):
        out[k] = int(re.search(rf"^constexpr \w+ {k} = (\d+);", dev, re.M).group(1))
    chain = re.search(r"struct CvChainDev \{(.*?)\n\};", dev, re.S).group(1)
    out["CvChainDev::begin"] = int(re.search(r"\bbegin\[(\d+)\]", chain).group(1))
    args = re.search(r"struct CascadeArgs \{(.*?)\n\};", dev, re.S).group(1)
    out["CascadeArgs::seg_end"] = int(re.search(r"\bseg_end\[(\d+)\]", args).group(1))
    return out


def widest_stage(cid):
    a = topology_cascade(cid)
    return max(int(a.tree_n_nodes[t0:t0 + n].sum()) for t0, n in zip(a.stage_first_tree, a.stage_n_trees))


def chain_lengths(cid):
    return [e - b for b, e in topology_chains(cid)]


def test_the_table_stands_on_both_sides_of_every_limit():
    lim = header_limits()
    assert api.VJ_MAX_STAGES == lim["VJ_MAX_STAGES"] and api.VJ_MAX_PASSES == lim["VJ_MAX_PASSES"]
    n = lim["VJ_MAX_STAGES"]
    assert topology_cascade("lin64").n_stages == n and topology_cascade("lin65").n_stages == n + 1
    assert topology_cell("lin64")[4] and not topology_cell("lin65")[4]
    assert topology_cascade("st_64").n_stages == n and np.any(topology_cascade("st_64").stage_next != -1)   # ... and as a stage tree
    assert topology_passes(3, chain_lengths("st_64")) <= lim["VJ_MAX_PASSES"]
    tile_tail = lim["TILE_SP_MAX_BLOCKS"] * lim["TILE_SP_BLOCK"]           # the clod tile plan's wave-independent tail
    assert widest_stage("w256") == tile_tail and widest_stage("w257") == tile_tail + 1 and widest_stage("w257x2") == tile_tail + 1
    # (the public plan of a call does not show the tail; the plan dump's former shape search budgets its tables where it is on)
    former = {cid: cascade_to_product(topology_cascade(cid)).plan_tiles(320, 240, ARITH_FRAMES, flags=api.VJ_PLAN_TILES_FORMER_SHAPES)
              for cid in ("w256", "w257")}
    assert [list(former[cid][0].class_lds) for cid in former][0] != [list(former[cid][0].class_lds) for cid in former][1]
    cv_tail = lim["CV_TAIL_BLOCKS"] * 64                                   # the OpenCV profile's stump-parallel chain tail
    assert widest_stage("w512") == cv_tail and widest_stage("w513") == cv_tail + 1
    for key in ("CvChainDev::begin", "CascadeArgs::seg_end"):             # chains the OpenCV chain sweep / the clod tiles take
        assert len(chain_lengths("st_c4")) == lim[key] and len(chain_lengths("st_c5")) == lim[key] + 1, key
        assert len(chain_lengths("st_tree2")) == lim[key] and len(chain_lengths("st_c3")) == lim[key] - 1
    # the clod segment plan is kept up to VJ_MAX_PASSES passes
    assert topology_passes(3, chain_lengths("st_c3long")) == lim["VJ_MAX_PASSES"] - 1
    assert topology_passes(3, chain_lengths("st_c4long")) == lim["VJ_MAX_PASSES"] + 1
    assert topology_passes(3, chain_lengths("st_c5")) <= lim["VJ_MAX_PASSES"]
    # tile_sp_begin = 3 and the default pass bounds: cascades shorter than, as long as and longer than it
    assert [topology_cascade(c).n_stages for c in ("lin1", "lin2", "lin3")] == [1, 2, 3]
    # prefixes of 0, 1 and 3 stages: the linear prefix counts from 2 stages (clod) and from 1 (OpenCV profile)
    assert [topology_chains(c)[0][0] for c in ("st_root", "st_p1", "st_c3")] == [0, 1, 3]
    assert 1 in chain_lengths("st_c1") and chain_lengths("st_c1")[0] == 1 and chain_lengths("st_c1")[-1] == 1


# ------------------------------------------------------------------------------------------------ the host-only planner
@pytest.mark.parametrize("n_frames", [1, ARITH_FRAMES])
@pytest.mark.parametrize("cid", RUNNABLE_IDS)
def test_the_tile_plan_of_every_case_is_a_partition(cid, n_frames):
    cell = topology_cell(cid)
    c = cascade_to_product(topology_cascade(cid))
    h, w = cell[2]
    windows = c.count_windows(w, h)
    info, tiles = c.plan_tiles(w, h, n_frames)                               # VJ_OK, or VjError
    cut_info, cut_tiles = c.plan_tiles(w, h, n_frames, tile_split=-1.0)
    assert [(t.scale_idx, t.lds_class, t.tile_w, t.tile_h) for t in tiles] == [(t.scale_idx, t.lds_class, t.tile_w, t.tile_h) for t in cut_tiles]
    tile_windows = sum(t.nx * t.tile_row_end for t in cut_tiles if t.lds_class >= 0)
    assert cut_info.cut.plan_windows == windows == sum(t.nx * t.ny for t in cut_tiles)
    assert tile_windows + cut_info.cut.gather_windows == windows, (cid, tile_windows, cut_info.cut.gather_windows, windows)


@pytest.mark.parametrize("cid,code", [("st_cycle", VJ_ERR_UNSUPPORTED), ("lin65", VJ_ERR_LIMIT)])
def test_the_planner_refuses(cid, code):
    c = cascade_to_product(topology_cascade(cid))            # the loader takes both: the limits are the planners'
    h, w = topology_cell(cid)[2]
    for n_frames in (1, ARITH_FRAMES):
        with pytest.raises(VjError) as ei:
            c.plan_tiles(w, h, n_frames)
        assert ei.value.code == code


@pytest.mark.parametrize("cid", [c[0] for c in TOPOLOGY_CELLS])
def test_every_case_survives_save_and_load(tmp_path, cid):
    from clfacedetection_amd import Cascade
    from oracle.oracle import load_vjc
    a = topology_cascade(cid)
    c = cascade_to_product(a)
    assert c.info.n_stages == a.n_stages and bool(c.info.is_stage_tree) == bool(np.any(a.stage_next != -1))
    path = str(tmp_path / f"{cid}.vjc")
    c.save(path)
    d = Cascade.load(path)
    for f in ("stages", "trees", "nodes", "alpha"):
        assert getattr(c, f).tobytes() == getattr(d, f).tobytes(), (cid, f)
    b = load_vjc(path)                                       # the independent reader gives the oracle's arrays back
    b.node_tilted = b.node_tilted.astype(np.int32)
    assert a.same_as(b) == [], (cid, a.same_as(b))
