"""Every position of the chain-balance cut, on the host alone through vj_plan_tiles_split: the rows the tile chain keeps
and the first-pass units of the global-gather chain must divide a plan's windows exactly, for every shipped cascade, five
frame sizes, the three batch-size classes, grouped and ungrouped tile lists, and a ladder of splits that puts the cut into
every tile scale at five depths.  The last tests record that the cells of tests/test_gpu_tile_cut.py land in the regimes
they are named after."""
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

import tile_cut_cases as tc
from clfacedetection_amd import VJ_FLAG_TILTED_AS_UPRIGHT, Cascade, default_params
from clfacedetection_amd.api import DATA_DIR, VJ_PLAN_TILES_NO_GROUPS

NAMES = sorted(os.path.basename(p)[len("haarcascade_"):-len(".vjc")] for p in glob.glob(os.path.join(DATA_DIR, "haarcascade_*.vjc")))
SIZES = [(1920, 1080), (1280, 720), (640, 480), (310, 230), (100, 80)]
BATCHES = [1, 8, 64]
DEPTHS = (0.01, 0.25, 0.5, 0.75, 0.99)
_CASC = {}
# (the query is read-only and the library's error text is per thread: a ladder's plans are built side by side)
_POOL = ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))


def cascade(name):
    if name not in _CASC:
        _CASC[name] = Cascade.load(name)
    return _CASC[name]


def params():
    return default_params(flags=VJ_FLAG_TILTED_AS_UPRIGHT)


def fields(s):
    return [getattr(s, f) if not hasattr(getattr(s, f), "__len__") else list(getattr(s, f)) for f, _ in s._fields_]


def check_plan(info, tiles, windows, what):
    ts = tc.tile_scales(tiles)
    for t in tiles:
        if t.lds_class < 0:
            assert t.tile_row_end == 0 and t.gather_windows == t.nx * t.ny, (what, t.scale_idx)
            continue
        # range of the cut: whole tile rows of the LEAD's shape, or every row
        th = tc.lead_of(tiles, t).tile_h
        assert 0 <= t.tile_row_end <= t.ny, (what, t.scale_idx, t.tile_row_end)
        assert t.tile_row_end == t.ny or t.tile_row_end % th == 0, (what, t.scale_idx, t.tile_row_end, th)
        # the rows the tiles leave are the gather chain's, no more and no fewer
        assert t.gather_windows == t.nx * (t.ny - t.tile_row_end), (what, t.scale_idx, t.gather_windows)
    # consumed from the largest tile scale down: at most one partial scale, 0 above it, every row below it
    cut = [i for i, t in enumerate(ts) if t.tile_row_end < t.ny]
    if cut:
        assert all(t.tile_row_end == 0 for t in ts[cut[0] + 1:]), (what, [t.tile_row_end for t in ts])
    assert sum(1 for t in ts if tc.partial(t)) <= 1, (what, [t.tile_row_end for t in ts])
    # tile count of every class launch
    assert list(info.class_tiles) == tc.expected_class_tiles(info, tiles), (what, list(info.class_tiles))
    # a full partition
    assert info.cut.plan_windows == windows == sum(t.nx * t.ny for t in tiles), what
    assert tc.tile_windows(tiles) + info.cut.gather_windows == windows, (what, tc.tile_windows(tiles), info.cut.gather_windows)
    assert (info.cut.gather_units > 0) == (info.cut.gather_windows > 0), what


@pytest.mark.parametrize("flags", [0, VJ_PLAN_TILES_NO_GROUPS])
@pytest.mark.parametrize("nf", BATCHES)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_every_position_of_the_cut(name, W, H, nf, flags):
    c = cascade(name)
    windows = c.count_windows(W, H, params())
    shipped_info, shipped = c.plan_tiles(W, H, nf, params(), flags)
    n_tile = len(tc.tile_scales(shipped))
    ladder = [0.0] + [tc.f32(j + f) for j in range(n_tile + 1) for f in DEPTHS] + [99.0]
    plans = list(_POOL.map(lambda s: c.plan_tiles(W, H, nf, params(), flags, tile_split=s), ladder))
    prev = None
    for split, (info, tiles) in zip(ladder, plans):
        assert info.cut.tile_split == split
        check_plan(info, tiles, windows, (name, W, H, nf, flags, split))
        rows = [t.tile_row_end for t in tiles]
        # monotone: a larger split never gives a scale more tile rows
        assert prev is None or all(a >= b for a, b in zip(prev, rows)), (name, W, H, nf, flags, split)
        prev = rows
    assert [t.tile_row_end for t in plans[0][1]] == [t.ny if t.lds_class >= 0 else 0 for t in plans[0][1]], "split 0: nothing moves"
    assert not any(prev), "split 99: no tile rows are left"
    assert not any(plans[-1][0].class_tiles)
    # a negative split is the shipped one, field for field
    info, tiles = c.plan_tiles(W, H, nf, params(), flags, tile_split=-1.0)
    assert fields(info) == fields(shipped_info) and [fields(t) for t in tiles] == [fields(t) for t in shipped]
    assert info.cut.tile_split >= 0.0
    check_plan(info, tiles, windows, (name, W, H, nf, flags, "shipped"))


def test_bad_splits_are_refused():
    from clfacedetection_amd import VjError
    with pytest.raises(VjError):
        cascade("frontalface_alt").plan_tiles(310, 230, 8, tile_split=float("nan"))


# ----------------------------------------------------------------------------- the cells of tests/test_gpu_tile_cut.py
def describe(split, tiles):
    return f"split {split:g}: tile_row_end {[t.tile_row_end for t in tc.tile_scales(tiles)]}"


def test_the_plan_the_gpu_cells_are_named_after():
    """frontalface_alt, 310 x 230, 8 frames: 14 tile scales, two groups of four, heights 20, 24 and 28 among the shapes,
    groups staged in a shape that is not every member's own."""
    c = cascade("frontalface_alt")
    _, tiles = c.plan_tiles(tc.W, tc.H, 8, tile_split=0.0)
    ts = tc.tile_scales(tiles)
    assert len(ts) == 14 and [len(g) for g in tc.groups(tiles)].count(4) == 2
    assert {20, 24, 28} <= {tc.lead_of(tiles, t).tile_h for t in ts}
    assert any((t.tile_w, t.tile_h) != (tc.lead_of(tiles, t).tile_w, tc.lead_of(tiles, t).tile_h) for t in ts)
    assert all(t.nx % tc.lead_of(tiles, t).tile_w and t.ny % tc.lead_of(tiles, t).tile_h for t in ts), "partial tiles at both edges"


@pytest.mark.parametrize("cell", sorted(tc.REGIMES))
def test_gpu_cells_of_8_frames_land_in_their_regimes(cell):
    c = cascade("frontalface_alt")
    split, info, tiles = tc.find_split(c, 8, *tc.REGIMES[cell])
    print(cell, describe(split, tiles))
    assert split != int(split) and sum(1 for t in tiles if tc.partial(t)) <= 1
    if cell == "h24_zero_rows":
        assert not any(tc.partial(t) for t in tiles)
    if cell.startswith("lead_gone") or cell.startswith("first_member_alone"):
        # members remain in a tile list that is laid out in the shape of a scale without tile rows
        g = next(g for g in tc.groups(tiles) if g[-1].tile_row_end == 0 and any(m.tile_row_end for m in g))
        assert info.class_tiles[g[-1].lds_class] > 0


def test_gpu_cells_of_whole_splits_and_of_no_tiles():
    c = cascade("frontalface_alt")
    for n in tc.WHOLE:
        split, info, tiles = tc.whole_split(c, 8, n)
        print(describe(split, tiles))
        assert any(info.class_tiles)
    for n in (14, 99):
        _, info, tiles = tc.whole_split(c, 8, n)
        assert not any(info.class_tiles) and not any(t.tile_row_end for t in tiles)


@pytest.mark.parametrize("nf", [1, 8, 33])
@pytest.mark.parametrize("cell", sorted(tc.SUBSET))
def test_gpu_cells_of_the_subset(cell, nf):
    split, _, tiles = tc.find_split(cascade("frontalface_alt"), nf, *tc.SUBSET[cell])
    print(nf, cell, describe(split, tiles))


@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
@pytest.mark.parametrize("cell", sorted(tc.TREE_REGIMES))
def test_gpu_cells_of_the_tree_cascades(casc, cell):
    split, _, tiles = tc.find_split(cascade(casc), 8, *tc.TREE_REGIMES[cell])
    print(casc, cell, describe(split, tiles))


def test_gpu_cells_of_the_group_sizes(monkeypatch):
    c = cascade("frontalface_alt")
    for cell in sorted(tc.GROUP1_REGIMES):
        split, _, tiles = tc.find_split(c, 8, *tc.GROUP1_REGIMES[cell], flags=VJ_PLAN_TILES_NO_GROUPS)
        assert all(t.lead_scale_idx == t.scale_idx for t in tiles)
        print("group 1", cell, describe(split, tiles))
    monkeypatch.setenv("VJ_TILE_GROUP", "8")     # the query reads it as a new environment does
    _, tiles = c.plan_tiles(tc.W, tc.H, 8, tile_split=0.0)
    assert max(len(g) for g in tc.groups(tiles)) == 8
    for cell in sorted(tc.GROUP8_REGIMES):
        split, _, tiles = tc.find_split(c, 8, *tc.GROUP8_REGIMES[cell])
        print("group 8", cell, describe(split, tiles))
