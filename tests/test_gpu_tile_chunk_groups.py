"""The chunk groups of the tile kernel's dense sweep against the oracle (sweep_stages<..., MULTI>): a wave
sweeps its queue in groups of 4 chunks while more than 192 entries are left, then ONE group of 3 (129..192 left) or of 2 (65..128),
then a lone chunk (1..64), which on the staged tile walks two stumps per step whatever gather_pairs says.  How a wave's windows
are grouped must not show: per frame the rectangles are the oracle's, and with VJ_FLAG_COUNTERS the windows entering every stage
are too.  Every case runs once timed and once counted, and first shows on the CPU that it reaches the path it is named for: the
tile shapes come from Cascade.plan_tiles, a wave's entries at stage 0 from the kernel's dealing rule (whole chunks, the first
n_chunks % 8 waves one more, windows outside the grid dropped), its share after a re-pack from the kernel's rule
(64 * ceil(chunks / 8)), and that a crafted stage passes every window, none or about half from the oracle's stage_entered.

What the ladder's edges get: with a pass-everything first stage a wave enters stage 1 with exactly its stage-0 entries, and the
full and edge tiles of the 640 x 480 and 320 x 240 plans give 64, 128, 136, 192 and 256 exactly, 66 for 65, 130 for 129 and 216
for 193 (each asserted to take the same groups as the count it stands for); crafted windows add waves of exactly 129 and of 200
entries at stage 0; a pass-nothing stage leaves 0, and a stage that
passes alternate columns leaves the waves of the finest scale half of their entries."""
import numpy as np
import pytest

from cases import SURVIVOR_SPOT_THRESHOLD, cascade_to_product, dot_frame, geometry_cascade, rows_of, survivor_cascade, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, default_params, synth

pytestmark = pytest.mark.gpu

SIZES = {"vga": (480, 640), "qvga": (240, 320)}
KINDS = ("faces", "noise", "blocks")
ALL_STAGES = ",".join(str(s) for s in range(1, 22))      # tile_repack with bit 1 set (the default is every stage from 2 on)
_CACHE = {}


# ----------------------------------------------------------------------------- the kernel's rules, on the CPU
def ladder(n):
    """the chunk groups a wave with n entries sweeps a stage in"""
    g, base = [], 0
    while base + 192 < n:
        g.append(4)
        base += 256
    if base + 128 < n:
        g.append(3)
        base += 192
    elif base + 64 < n:
        g.append(2)
        base += 128
    if base < n:
        g.append(1)
    return tuple(g)


def stage0_counts(t, lead):
    """per tile of member t of lead's group: (the eight waves' entries at stage 0, the tile's valid windows)"""
    tw, th = lead.tile_w, lead.tile_h
    n_tile = tw * th
    c_base, c_extra = divmod((n_tile + 63) // 64, 8)
    out = []
    for iy0 in range(0, t.tile_row_end, th):
        for ix0 in range(0, t.nx, tw):
            waves = []
            for w in range(8):
                b = min((w * c_base + min(w, c_extra)) * 64, n_tile)
                e = min(b + (c_base + (1 if w < c_extra else 0)) * 64, n_tile)
                waves.append(sum(1 for i in range(b, e) if iy0 + i // tw < t.ny and ix0 + i % tw < t.nx))
            out.append(waves)
    return out


def shares(total):
    """the eight waves' entries after a re-pack of `total` survivors"""
    s = 64 * (((total + 63) // 64 + 7) // 8)
    return [min(s, total - min(w * s, total)) for w in range(8)]


def tile_scales(c, size, n):
    """[(member, its group's lead)] of the plan's tile scales"""
    h, w = SIZES[size]
    _, tiles = c.plan_tiles(w, h, n)
    by_idx = {t.scale_idx: t for t in tiles}
    return [(t, by_idx[t.lead_scale_idx]) for t in tiles if t.tile_w != 0]


def all_counts(c, size, n):
    """(every wave's stage-0 entries, every wave's share after a re-pack of a tile whose windows all survive, the tiles' totals
    with their tile's size) over the plan's tile scales"""
    first, packed, totals = set(), set(), []
    for t, lead in tile_scales(c, size, n):
        for waves in stage0_counts(t, lead):
            first |= set(waves)
            packed |= set(shares(sum(waves)))
            totals.append((sum(waves), lead.tile_w * lead.tile_h))
    return first, packed, totals


# ----------------------------------------------------------------------------- cascades, frames, the oracle's results
def cascade_of(cascades, which):
    """(product cascade, oracle arrays): a shipped name, ("geometry", ww, wh) or ("survivor", variant, pass-everything stages)"""
    if isinstance(which, str):
        return cascades(which)
    if which not in _CACHE:
        if which[0] == "geometry":
            arrays = geometry_cascade(which[1], which[2], "upright")
        else:
            arrays = survivor_cascade("stumps", which[2])
            if which[1] == "nothing":        # the first stage's one stump gives 0 or 1: no window reaches 2
                arrays.stage_threshold[0] = 2.0
            elif which[1] == "columns":      # the first stage compares the window's two left-most columns with the window
                arrays.node_rect.reshape(-1, 3, 4)[0, 1] = (0, 0, 2, 20)
                arrays.node_threshold[0] = SURVIVOR_SPOT_THRESHOLD
                arrays.stage_threshold[0] = 0.5
        _CACHE[which] = (cascade_to_product(arrays), arrays)
    return _CACHE[which]


def frames_of(size, content="mix"):
    if (size, content) not in _CACHE:
        h, w = SIZES[size]
        if content == "mix":
            f = synth.batch(3, h, w, seed0=7300, kinds=KINDS)
        elif content == "dots":
            f = np.stack([dot_frame(7400 + i, h, w, 40) for i in range(3)])
        else:   # stripes of two bright and two dark columns under the dots: a window at an even x has bright left columns or dark ones
            f = np.stack([dot_frame(7500 + i, h, w, 40) for i in range(3)])
            f[:, :, 0::4] = np.maximum(f[:, :, 0::4], 200)
            f[:, :, 1::4] = np.maximum(f[:, :, 1::4], 200)
        _CACHE[(size, content)] = f
    return _CACHE[(size, content)]


def wanted(oracle, arrays, key, frames, n):
    """per frame (rectangles, stage_entered), computed once per cascade and content"""
    if ("want", key) not in _CACHE:
        out = []
        for f in frames:
            ro, st = oracle.detect(arrays, f)
            out.append((rows_of(ro), list(st["stage_entered"])))
        _CACHE[("want", key)] = out
    return _CACHE[("want", key)][:n]


def totals(want):
    return [sum(v) for v in zip(*[st for _, st in want])]


def check(r, want, label, counted):
    for f, (rects, _) in enumerate(want):
        assert sorted(rows_of(r.rects[r.rects["frame"] == f])) == sorted(rects), f"{label}: frame {f}"
    assert len(r.rects) == sum(len(w[0]) for w in want), label
    if counted:
        entered = totals(want)
        assert r.stage_entered[:len(entered)] == entered, f"{label}: windows entering each stage"


def run_both(env, c, frames, want, label, settings=()):
    with tunables(env, *settings):
        timed = env.detect(c, frames)
        counted = env.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS))
    assert any(l["kind"] == "tile" for l in counted.launches), f"{label}: no tile launch"
    check(timed, want, f"{label} {settings} timed", False)
    check(counted, want, f"{label} {settings} counted", True)
    return counted


# ----------------------------------------------------------------------------- waves of 1, 2, 3 and 4 chunks in stage 0
# (id, cascade, frames per call, the group's members, its tile's width and height, its chunks, the groups a full tile's waves sweep in)
WAVES = [
    ("chunks28_waves_of_3_and_4", "frontalface_alt", 2, (0, 1, 2, 3), 56, 32, 28, {(4,), (3,)}),
    ("chunks21_waves_of_2_and_3", "frontalface_alt", 2, (4, 5, 6, 7), 48, 28, 21, {(3,), (2,)}),
    ("chunks13_waves_of_1_and_2", ("geometry", 27, 32), 2, (4, 5, 6, 7), 40, 20, 13, {(2,), (1,)}),
    ("chunks7_fewer_than_waves", ("geometry", 22, 62), 2, (4, 5, 6, 7), 16, 28, 7, {(1,), ()}),
]


@pytest.mark.parametrize("cid,which,n,members,tw,th,chunks,forms", WAVES, ids=[w[0] for w in WAVES])
def test_waves_of_one_to_four_chunks_in_stage_0(env, oracle, cascades, cid, which, n, members, tw, th, chunks, forms):
    c, arrays = cascade_of(cascades, which)
    group = [(t, lead) for t, lead in tile_scales(c, "vga", n) if t.scale_idx in members]
    assert [t.scale_idx for t, _ in group] == list(members)
    lead = group[-1][0]
    assert all(l.scale_idx == lead.scale_idx and t.step == 2.0 for t, l in group)
    assert (lead.tile_w, lead.tile_h) == (tw, th) and (tw * th + 63) // 64 == chunks
    for t, _ in group:   # a full tile and an edge tile of every member, and the waves of the full tile take the forms of the case
        assert t.nx > tw and t.ny > th and (t.nx % tw != 0 or t.ny % th != 0) and t.tile_row_end == t.ny, (t.scale_idx, t.nx, t.ny)
        per_tile = stage0_counts(t, lead)
        assert {ladder(k) for k in per_tile[0]} == forms, (t.scale_idx, per_tile[0])
        assert sum(per_tile[0]) == tw * th and sum(per_tile[-1]) < tw * th
    frames = frames_of("vga")[:n]
    want = wanted(oracle, arrays, (which, "vga", "mix"), frames_of("vga"), n)
    for settings in ((), (("concurrent", 0),)):
        run_both(env, c, frames, want, cid, settings)


# ----------------------------------------------------------------------------- entry counts at the ladder's edges
# target entries -> the count the plans give (module docstring); (size, frames per call) of the plan that holds it
EDGES = {64: 64, 65: 66, 128: 128, 129: 130, 136: 136, 192: 192, 193: 216, 256: 256}
# nearer still, at stage 0 of crafted windows: (cascade, size, frames per call, a wave's entries)
EDGES_STAGE_0 = [(("geometry", 26, 26), "qvga", 3, 129), (("geometry", 26, 26), "qvga", 3, 200)]


@pytest.mark.parametrize("size,n", [("vga", 1), ("qvga", 3)])
def test_entry_counts_at_the_ladders_edges(env, oracle, cascades, size, n):
    """Two pass-everything stages, then one that follows the dots: a wave enters stage 1 with its stage-0 entries (compacted onto
    themselves) and stage 2 with its share of a tile whose windows all survive; with a re-pack before stage 1 that share is
    stage 1's too."""
    which = ("survivor", "everything", 2)
    c, arrays = cascade_of(cascades, which)
    frames = frames_of(size, "dots")[:n]
    want = wanted(oracle, arrays, (which, size, "dots"), frames_of(size, "dots"), n)
    entered = totals(want)
    assert entered[0] == entered[1] == entered[2] > 0, entered              # every window passes stages 0 and 1
    first, packed, _ = all_counts(c, size, n)
    both = all_counts(c, "vga", 1)[0] | all_counts(c, "qvga", 3)[0]
    for target, got in EDGES.items():
        assert got in both and ladder(got) == ladder(target), (target, got)
    assert {ladder(k) for k in first} >= {(), (1,), (2,), (3,), (4,)}, sorted(first)
    assert {64, 128, 192, 256} <= first and {64, 128, 192, 256} <= packed, (sorted(first), sorted(packed))
    assert (first >= {216, 66} if size == "qvga" else first >= {130, 136}), sorted(first)
    for settings in ((), (("tile_repack", ALL_STAGES),)):
        run_both(env, c, frames, want, f"edges {size}", settings)


@pytest.mark.parametrize("which,size,n,entries", EDGES_STAGE_0, ids=[f"{e[3]}_entries" for e in EDGES_STAGE_0])
def test_stage_0_waves_next_to_the_ladders_edges(env, oracle, cascades, which, size, n, entries):
    """Edge tiles of crafted windows whose waves enter stage 0 with exactly 129 entries (the smallest group of three) and with 200
    (a group of four on 3 chunks and 8 windows; the plans looked at hold no wave nearer to 193)."""
    c, arrays = cascade_of(cascades, which)
    first, _, _ = all_counts(c, size, n)
    assert entries in first and ladder(entries) == {129: (3,), 200: (4,)}[entries], sorted(first)
    frames = frames_of(size)[:n]
    want = wanted(oracle, arrays, (which, size, "mix"), frames_of(size), n)
    run_both(env, c, frames, want, f"{entries} entries at stage 0")


@pytest.mark.parametrize("variant", ["nothing", "columns"])
def test_compaction_to_nothing_and_to_alternate_columns(env, oracle, cascades, variant):
    """A first stage that passes no window (every wave is left with 0 entries after its groups), and one that passes the windows
    whose two left-most columns are bright on striped frames (two bright, two dark): about every other window of the finest scale,
    whose windows start at even columns, so its waves go on with survivors compacted from all of their chunks; at coarser scales
    the stripes blur and fewer pass.  Asserted from the oracle's totals: never more than about every other window, and at least
    most of the finest scale's half (the oracle gives no count per wave)."""
    which = ("survivor", variant, 2)
    c, arrays = cascade_of(cascades, which)
    content = "dots" if variant == "nothing" else "stripes"
    frames = frames_of("vga", content)[:2]
    want = wanted(oracle, arrays, (which, "vga", content), frames_of("vga", content), 2)
    entered = totals(want)
    if variant == "nothing":
        assert entered[0] > 0 and entered[1] == 0, entered
    else:
        finest = tile_scales(c, "vga", 2)[0][0]
        assert finest.scale_idx == 0 and finest.step == 2.0
        assert 0.4 * 2 * finest.nx * finest.ny <= entered[1] <= 0.6 * entered[0] and entered[2] == entered[1], entered
    assert {(4,), (3,)} <= {ladder(k) for k in all_counts(c, "vga", 2)[0]}
    run_both(env, c, frames, want, variant)


# ----------------------------------------------------------------------------- shares of three after a re-pack
@pytest.mark.parametrize("size,n", [("qvga", 2), ("vga", 2)])
def test_shares_of_three_and_a_thin_lone_chunk_after_a_repack(env, oracle, cascades, size, n):
    """Four pass-everything stages and tile_ws_max 0 (no wave-split finish: the dense sweep runs to the cascade's end, re-packing
    before every stage from 2 on).  320 x 240: the right-edge tiles of the 56 x 32 group (1792 windows) keep 1088 .. 1216 of
    them — eight ragged queues of 4 partial chunks, 120 .. 184 entries each, groups of three on partial chunks — and re-pack to
    shares of three.  640 x 480: a full 48 x 28 tile keeps its 1344 windows, 192 or 128 per wave before and 192 after; full
    56 x 32 tiles keep 1792: shares of four.  Edge tiles leave last waves with 1 .. 16 windows."""
    which = ("survivor", "everything", 4)
    c, arrays = cascade_of(cascades, which)
    frames = frames_of(size, "dots")[:n]
    want = wanted(oracle, arrays, (which, size, "dots"), frames_of(size, "dots"), n)
    entered = totals(want)
    assert entered[0] == entered[3] == entered[4] > 0, entered
    _, packed, tot = all_counts(c, size, n)
    three = [(t, windows) for t, windows in tot if 1024 < t <= 1536]
    assert three and all(shares(t)[0] == 192 and ladder(shares(t)[0]) == (3,) for t, _ in three), tot
    if size == "qvga":   # more than 1024 survivors in a tile of at least 1536 windows, whose waves hold ragged queues before the re-pack
        assert any(windows >= 1536 for _, windows in three), three
        ragged = [waves for t, lead in tile_scales(c, size, n) if lead.tile_w * lead.tile_h >= 1536
                  for waves in stage0_counts(t, lead) if 1024 < sum(waves) <= 1536]
        assert ragged and all(0 < k < 192 for waves in ragged for k in waves), ragged
        assert any(ladder(k) == (3,) for waves in ragged for k in waves) and any(ladder(k) == (2,) for waves in ragged for k in waves)
    else:
        assert any(t == windows == 1344 for t, windows in three), three
    assert any(t > 1536 and shares(t)[0] == 256 for t, _ in tot)
    assert any(1 <= k <= 16 for k in packed), sorted(packed)
    for settings in ((("tile_ws_max", 0),), (("tile_ws_max", 0), ("tile_repack", ALL_STAGES))):
        run_both(env, c, frames, want, f"shares of three {size}", settings)


# ----------------------------------------------------------------------------- the gather chain's flag, configurations
def alt_case(oracle, cascades, name="frontalface_alt", size="vga", n=2):
    c, arrays = cascades(name)
    return c, frames_of(size)[:n], wanted(oracle, arrays, (name, size, "mix"), frames_of(size), n)


def test_lone_chunks_do_not_depend_on_gather_pairs(env, oracle, cascades):
    c, frames, want = alt_case(oracle, cascades)
    first, _, _ = all_counts(c, "vga", 2)
    assert any(ladder(k)[-1:] == (1,) for k in first)      # waves that end in a lone chunk
    got = [run_both(env, c, frames, want, f"gather_pairs {v}", (("gather_pairs", v),)) for v in (0, 1, 2)]
    for r in got[1:]:
        assert np.array_equal(r.rects, got[0].rects) and r.stage_entered == got[0].stage_entered


@pytest.mark.parametrize("concurrent", (1, 0))
@pytest.mark.parametrize("repack", ("default", "bit1", "none"))
def test_repack_masks_and_chain_modes(env, oracle, cascades, repack, concurrent):
    """tile_repack at its default, with a re-pack before stage 1 as well, and without any (a wave keeps its own windows to the
    end of the dense sweep: ever thinner lone chunks)."""
    c, frames, want = alt_case(oracle, cascades)
    settings = [("concurrent", concurrent)] + {"default": [], "bit1": [("tile_repack", ALL_STAGES)], "none": [("tile_repack", "")]}[repack]
    run_both(env, c, frames, want, f"tile_repack {repack}", tuple(settings))


@pytest.mark.parametrize("name", ["frontalface_alt2", "frontalface_alt_tree"])
def test_tree_cascades_keep_their_paths(env, oracle, cascades, name):
    """Two-node trees sweep in pairs of chunks and the stage tree's prefix per chunk: neither takes the stump groups."""
    c, frames, want = alt_case(oracle, cascades, name, "qvga", 2)
    run_both(env, c, frames, want, name)


def test_regions_on_tiles(env, oracle, cascades):
    """vj_detect_rois: the region pass shares tile_pass_body and gets the groups with it."""
    c, arrays = cascades("frontalface_alt")
    f = frames_of("vga")
    rois = [(0, 0, 0, 640, 480), (1, 40, 30, 400, 300), (2, 201, 99, 320, 240)]
    # the region pass lays the tiles of the frame plan's class-0 scales inside a region whose grid at such a scale holds at least
    # roi_tiles windows (a linear stump cascade): every region here has such grids, of tiles of several chunks
    _, frame_tiles = c.plan_tiles(640, 480, len(f))
    class0 = {t.scale_idx for t in frame_tiles if t.tile_w != 0 and t.lds_class == 0 and t.tile_w * t.tile_h > 192}
    assert class0
    for _, _, _, w, h in rois:
        _, own = c.plan_tiles(w, h, 1)
        assert any(t.scale_idx in class0 and t.nx * t.ny >= 512 for t in own), (w, h)
    want = [oracle.detect(arrays, np.ascontiguousarray(f[fr][y:y + h, x:x + w])) for fr, x, y, w, h in rois]
    with tunables(env, ("roi_tiles", 512)):
        timed = env.detect_rois(c, f, rois)
        counted = env.detect_rois(c, f, rois, default_params(flags=VJ_FLAG_COUNTERS))
    for r in (timed, counted):
        for i, (ro, _) in enumerate(want):
            assert sorted(rows_of(r.rects[r.rects["frame"] == i])) == sorted(rows_of(ro)), rois[i]
    assert counted.stage_entered == [sum(v) for v in zip(*[st["stage_entered"] for _, st in want])]
