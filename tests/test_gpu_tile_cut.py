"""Every position of the chain-balance cut against the C oracle, frame by frame: rectangles, per-stage counts and windows,
all exact.  The cut hands the upper rows of the largest tile scales to the global-gather chain in whole tile rows of the
scale's GROUP LEAD; since the tiles grew, a member's own shape regularly differs from the lead's, heights of 28, 24 and 20
rows exist, and a group can lose its lead to the gather chain while members staged in the lead's shape stay on tiles.

Frames are 310 x 230 (partial tiles at both edges for every shape, 14 tile scales).  Each cell names a regime; its split is
found through the host-only plan query at the cell's frame count (tile_cut_cases.find_split; tests/test_tile_cut_cpu.py
asserts that every regime is still reachable), and the same query says what the launches must show, so that a wrong cut
shows as itself and not as a missing rectangle: the windows entering stage 0 inside the tile launches, the rest in the
other launches, which scales each launch names, and the LDS block of each tile launch.

A call of 5 .. 7 frames caps its split at 0.5, so the tree cascades and the candidate-heavy content run 8 frames."""
import numpy as np
import pytest

import tile_cut_cases as tc
from cases import check_against_oracle, first_difference, rows_of, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_SKIP_LIST, Environment, default_params, synth
from clfacedetection_amd.api import VJ_PLAN_TILES_NO_GROUPS

pytestmark = pytest.mark.gpu

H, W = tc.H, tc.W
KINDS = ("noise", "faces", "blocks")
_FRAMES = {}
_ORACLE = {}


def frames_of(n, kinds=KINDS, seed0=1100):
    """a prefix of ONE set of distinct frames per kind tuple"""
    key = (kinds, seed0)
    if key not in _FRAMES or len(_FRAMES[key]) < n:
        _FRAMES[key] = synth.batch(max(n, 33 if kinds == KINDS else 8), H, W, seed0=seed0, kinds=kinds)
    return _FRAMES[key][:n]


def oracle_runs(oracle, cascades, name, frames, tag, mode=None):
    """[(rects, stats)] per frame, computed once per module, cascade and frame"""
    _, a = cascades(name)
    done = _ORACLE.setdefault((name, tag, mode), [])
    while len(done) < len(frames):
        done.append(oracle.detect(a, frames[len(done)]) if mode is None else oracle.detect(a, frames[len(done)], mode=mode))
    return done[:len(frames)]


def assert_cut(r, info, tiles, n_frames, split, label, counted_windows=True):
    """what the plan query promises about the launches of a call at this split"""
    ts = tc.tile_scales(tiles)
    by = tc.by_idx(tiles)
    tile = [l for l in r.launches if l["kind"] == "tile"]
    other = [l for l in r.launches if l["kind"] != "tile"]
    print(f"{label}: split {split:g}, tile_row_end {[t.tile_row_end for t in ts]}; " +
          "; ".join(f"{l['kind']}{l['lds_class'] if l['kind'] == 'tile' else ''} [{l['stage_begin']},{l['stage_end']}) "
                    f"{l['stage_entered'][0]}" for l in r.launches))
    assert r.tile_split == np.float32(split), (label, r.tile_split)
    # which scales a launch names
    on_tiles = {t.scale_idx for t in ts if t.tile_row_end > 0}
    assert {l["lds_class"] for l in tile} == {k for k in range(info.n_classes) if info.class_tiles[k]}, label
    assert len(tile) == len({l["lds_class"] for l in tile}), label
    for l in tile:
        want = {t.scale_idx for t in ts if t.tile_row_end > 0 and by[t.lead_scale_idx].lds_class == l["lds_class"]}
        assert set(l["scales"]) == want, (label, l["lds_class"], l["scales"], sorted(want))
        assert l["lds_bytes"] == info.class_lds[l["lds_class"]], (label, l["lds_class"], l["lds_bytes"], list(info.class_lds))
    assert set().union(*[l["scales"] for l in tile]) == on_tiles if tile else not on_tiles, label
    on_gather = {t.scale_idx for t in tiles if t.tile_row_end < t.ny}     # (no tile scale: tile_row_end 0)
    grid = [l for l in r.launches if l["kind"] == "grid"]
    assert bool(grid) == bool(on_gather), label
    for l in grid:
        assert set(l["scales"]) == on_gather, (label, l["scales"], sorted(on_gather))
    if counted_windows:
        # the windows each chain starts with
        want_tile = n_frames * tc.tile_windows(tiles)
        got_tile = sum(l["stage_entered"][0] for l in tile)
        assert got_tile == want_tile, f"{label}: {got_tile} windows enter the tile launches, the plan gives them {want_tile}"
        got_other = sum(l["stage_entered"][0] for l in other)
        assert got_other == r.windows - want_tile == n_frames * info.cut.gather_windows, \
            f"{label}: {got_other} windows enter the other launches, {r.windows - want_tile} are left to them"


def run_cell(env, c, frames, want, found, label, *settings):
    split, info, tiles = found
    with tunables(env, ("tile_split", tc.split_text(split)), *settings):
        r, _ = check_against_oracle(env, c, frames, want, label)
    assert_cut(r, info, tiles, len(frames), split, label)
    return r


@pytest.fixture
def fresh(monkeypatch):
    """make(VJ_TILE_GROUP=...) -> a fresh environment (the variable is read when one is created); closed afterwards."""
    made = []

    def make(**envvars):
        for k, v in envvars.items():
            monkeypatch.setenv(k, str(v))
        e = Environment(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


# ----------------------------------------------------------------------------- frontalface_alt, 8 frames: every regime
@pytest.mark.parametrize("cell", sorted(tc.REGIMES))
def test_cut_regimes(env, oracle, cascades, cell):
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    run_cell(env, c, frames, want, tc.find_split(c, 8, *tc.REGIMES[cell]), cell)


@pytest.mark.parametrize("n", tc.WHOLE)
def test_whole_scales(env, oracle, cascades, n):
    """exactly n scales' worth: no scale is partial"""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    run_cell(env, c, frames, want, tc.whole_split(c, 8, n), f"split {n}")


@pytest.mark.parametrize("n", [14, 99])
def test_everything_on_the_gather_chain(env, oracle, cascades, n):
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    r = run_cell(env, c, frames, want, tc.whole_split(c, 8, n), f"split {n}")
    assert not any(l["kind"] == "tile" for l in r.launches)


# ----------------------------------------------------------------------------- the subset in the other situations
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("cell", sorted(tc.SUBSET))
def test_other_batch_sizes(env, oracle, cascades, cell, n):
    """1 frame: the single-frame class of the balance (20 tile scales); 33: the >= 32 defaults and the band-major queue pass."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(n)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    run_cell(env, c, frames, want, tc.find_split(c, n, *tc.SUBSET[cell]), f"{n} frames, {cell}")


SETTINGS = {
    "one_stream": (("concurrent", "0"),),
    "chunked_queue_pass": (("q_band_px", "0"),),
    # every survivor of the cut scales is handed over at the first pass boundary: cut rows and hand-offs meet
    "handoff_at_first_boundary": (("tile_sp_begin", "64"), ("tile_end", "0")),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("cell", sorted(tc.SUBSET))
def test_tunables_at_the_cut(env, oracle, cascades, cell, setting):
    c, _ = cascades("frontalface_alt")
    n = 33 if setting == "chunked_queue_pass" else 8       # (the band-major pass it switches off takes batches of >= 32)
    frames = frames_of(n)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    r = run_cell(env, c, frames, want, tc.find_split(c, n, *tc.SUBSET[cell]), f"{setting}, {cell}", *SETTINGS[setting])
    if setting == "handoff_at_first_boundary":
        tile = [l for l in r.launches if l["kind"] == "tile"]
        queue = [l for l in r.launches if l["kind"] == "queue"]
        assert tile and queue and max(l["stage_end"] for l in tile) == min(l["stage_begin"] for l in queue)


@pytest.mark.parametrize("group,cell", [(1, k) for k in sorted(tc.GROUP1_REGIMES)] + [(8, k) for k in sorted(tc.GROUP8_REGIMES)])
def test_group_sizes(fresh, oracle, cascades, group, cell):
    """VJ_TILE_GROUP=1: every scale is cut in its own height; 8: scales 0 .. 7 are one group in the shape of scale 7."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    e = fresh(VJ_TILE_GROUP=group)       # (the plan query reads the variable as the environment does)
    _, base = c.plan_tiles(W, H, 8, tile_split=0.0)
    assert max(len(g) for g in tc.groups(base)) == group
    regimes = tc.GROUP1_REGIMES if group == 1 else tc.GROUP8_REGIMES
    found = tc.find_split(c, 8, *regimes[cell])
    if group == 1:
        flagged = c.plan_tiles(W, H, 8, flags=VJ_PLAN_TILES_NO_GROUPS, tile_split=found[0])[1]
        assert [t.tile_row_end for t in flagged] == [t.tile_row_end for t in found[2]]
    run_cell(e, c, frames, want, found, f"VJ_TILE_GROUP={group}, {cell}")


@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
@pytest.mark.parametrize("cell", sorted(tc.TREE_REGIMES))
def test_tree_cascades(env, oracle, cascades, casc, cell):
    """Two-node trees (the wave-split finish) and the stage tree (prefix on tiles), faces and blocks."""
    c, _ = cascades(casc)
    frames = frames_of(8, ("faces", "blocks"), 1200)
    want = oracle_runs(oracle, cascades, casc, frames, "fb")
    run_cell(env, c, frames, want, tc.find_split(c, 8, *tc.TREE_REGIMES[cell]), f"{casc}, {cell}")


def test_skip_list_at_an_in_group_cut(env, oracle, cascades):
    """VJ_FLAG_SKIP_LIST: the tile kernel reads each member's own skip bits; against the oracle's per-stage-list CPU loop."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix", mode=2)
    split, info, tiles = tc.find_split(c, 8, *tc.REGIMES["lead_gone_upper_group"])
    p = default_params(flags=VJ_FLAG_COUNTERS | VJ_FLAG_SKIP_LIST)
    # (the skip modes take the plan's cut like any other call; which windows are visited does not depend on it)
    assert [t.tile_row_end for t in c.plan_tiles(W, H, 8, p, tile_split=split)[1]] == [t.tile_row_end for t in tiles]
    with tunables(env, ("tile_split", tc.split_text(split))):
        r = env.detect(c, frames, p)
        r2 = env.detect(c, frames, default_params(flags=VJ_FLAG_SKIP_LIST))
    entered, windows = [0] * c.info.n_stages, 0
    for i, (ro, st) in enumerate(want):
        mine = rows_of(r.rects[r.rects["frame"] == i])
        assert mine == rows_of(ro), f"frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, first_difference(r.stage_entered, entered)
    assert r.windows == windows
    per_launch = [sum(l["stage_entered"][s] for l in r.launches) for s in range(c.info.n_stages)]
    assert per_launch == r.stage_entered
    assert np.array_equal(r2.rects, r.rects)
    assert_cut(r, info, tiles, 8, split, "skip list", counted_windows=False)
    assert sum(l["stage_entered"][0] for l in r.launches if l["kind"] == "tile") > 0


@pytest.mark.parametrize("cell,n", [("lead_gone_upper_group", 22), ("h20", 8)])
def test_candidate_heavy_content(env, oracle, cascades, cell, n):
    """Blocks and drawn faces only: the re-packs and the wave tail run on cut groups.  The smallest faces this content draws
    are found at scales 7 and up, which the "lead gone" cut has given to the gather chain; the first frame on which the
    oracle finds some at scales 0 and 2 is the 21st, so that cell takes 22 frames (the same batch-size class as 8)."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(22, ("blocks", "faces"), 1300)[:n]
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "heavy")
    found = tc.find_split(c, n, *tc.SUBSET[cell])
    assert [t.tile_row_end for t in found[2]] == [t.tile_row_end for t in tc.find_split(c, 8, *tc.SUBSET[cell])[2]]
    r = run_cell(env, c, frames, want, found, f"blocks / faces, {cell}")
    deep = [sum(l["stage_entered"][s] for l in r.launches if l["kind"] == "tile") for s in range(c.info.n_stages)]
    print("windows entering each stage inside tile launches:", deep)
    assert deep[3] > 0 and deep[-1] > 0, "survivors reach the finish stages and the last stage inside the tiles"
