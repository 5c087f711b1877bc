"""The chunks of a scale group's tile against the oracle (tile_pass_body): a tile of
n_chunks = ceil(tw * th / 64) chunks gives every wave n_chunks / 8 of them, and n_chunks % 8 spare ones are left over — today
they go to the first waves, one each; round 13 measured handing them to the waves that arrive first and did not ship it
(profiles/r13_notes.md).  However they are dealt, which wave evaluates a window must not show: per frame the rectangles are
the oracle's, and with VJ_FLAG_COUNTERS the windows entering every stage are too (a chunk dealt twice or never changes those
even where it holds no detection).  Group tiles with 0, 1 and 7 spare chunks — 7 both with and without whole chunks per
wave — found with Cascade.plan_tiles on the CPU and asserted here; grids that leave a full tile and an edge tile; a chain
balance that cuts inside a group, so that members are skipped by tile_row_end; frames of faces, whose members end in the wave
tail, in the finish and in the dense sweep."""
import pytest

from cases import cascade_to_product, geometry_cascade, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, default_params, synth

pytestmark = pytest.mark.gpu

H, W, N = 480, 640, 3
KINDS = ("faces", "noise", "blocks")
# (id, cascade: a shipped name or the window of a crafted one (cases.geometry_cascade), frames per call (the plan depends on it),
#  the group: its members' scale indices, the tile's width and height, its chunks)
SHAPES = [
    ("spare0", (29, 13), 3, (4, 5, 6, 7), 64, 24, 24),
    ("spare1", "frontalface_default", 3, (0, 1, 2, 3), 56, 28, 25),
    ("spare7_base1", (27, 28), 3, (4, 5, 6, 7), 40, 24, 15),
    ("spare7_base0", (22, 62), 2, (4, 5, 6, 7), 16, 28, 7),                  # fewer chunks than waves: one wave gets none
    ("spare4", "frontalface_alt", 3, (0, 1, 2, 3), 56, 32, 28),              # the shipped plan of the benchmark's cascade
]
_CACHE = {}


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


def cascade_of(cascades, which):
    """(product cascade, oracle arrays)"""
    if isinstance(which, str):
        return cascades(which)
    if which not in _CACHE:
        arrays = geometry_cascade(which[0], which[1], "upright")
        _CACHE[which] = (cascade_to_product(arrays), arrays)
    return _CACHE[which]


def frames():
    if "frames" not in _CACHE:
        _CACHE["frames"] = synth.batch(N, H, W, seed0=5200, kinds=KINDS)
    return _CACHE["frames"]


def wanted(oracle, arrays, key, n):
    """per frame (rectangles, stage_entered), computed once per cascade"""
    if ("want", key) not in _CACHE:
        out = []
        for f in frames():
            ro, st = oracle.detect(arrays, f)
            out.append((rows(ro), list(st["stage_entered"])))
        _CACHE[("want", key)] = out
    return _CACHE[("want", key)][:n]


def check(r, want, label, counted):
    entered = [0] * len(want[0][1])
    for f, (rects, st) in enumerate(want):
        assert rows(r.rects[r.rects["frame"] == f]) == rects, f"{label}: frame {f}"
        entered = [a + b for a, b in zip(entered, st)]
    assert len(r.rects) == sum(len(w[0]) for w in want), label
    if counted:
        assert r.stage_entered[:len(entered)] == entered, f"{label}: windows entering each stage"


def group_of(c, n, members, tile_split=None):
    _, tiles = c.plan_tiles(W, H, n, tile_split=tile_split)
    by_idx = {t.scale_idx: t for t in tiles}
    return [by_idx[m] for m in members]


@pytest.mark.parametrize("sid,which,n,members,tw,th,chunks", SHAPES, ids=[s[0] for s in SHAPES])
def test_group_tiles_with_spare_chunks_match_the_oracle(env, oracle, cascades, sid, which, n, members, tw, th, chunks):
    c, arrays = cascade_of(cascades, which)
    group = group_of(c, n, members)
    lead = group[-1]
    # the shape the test is about: one staged tile for all members, of `chunks` chunks
    assert all(t.lead_scale_idx == lead.scale_idx and t.tile_w != 0 and t.step == 2.0 for t in group), [(t.scale_idx, t.lead_scale_idx) for t in group]
    assert (lead.tile_w, lead.tile_h) == (tw, th) and (tw * th + 63) // 64 == chunks
    assert {"spare0": 0, "spare1": 1, "spare7_base1": 7, "spare7_base0": 7, "spare4": 4}[sid] == chunks % 8
    assert (chunks // 8 == 0) == (sid == "spare7_base0")
    # a full tile and an edge tile of every member
    for t in group:
        assert t.nx > tw and t.ny > th and (t.nx % tw != 0 or t.ny % th != 0), (t.scale_idx, t.nx, t.ny)
        assert t.tile_row_end == t.ny
    want = wanted(oracle, arrays, which, n)
    for settings in ((), (("concurrent", 0),), (("tile_ws_min", 0),)):   # (tile_ws_min 0: no wave tail, the finish to the end)
        with tunables(env, *settings):
            timed = env.detect(c, frames()[:n])
            counted = env.detect(c, frames()[:n], default_params(flags=VJ_FLAG_COUNTERS))
        assert any(l["kind"] == "tile" for l in counted.launches), "no tile launch"
        check(timed, want, f"{sid} {settings} timed", False)
        check(counted, want, f"{sid} {settings} counted", True)


@pytest.mark.parametrize("tile_split", (7.0, 8.0, 8.5))
def test_members_skipped_by_the_chain_balance(env, oracle, cascades, tile_split):
    """tile_split at a value that cuts inside the group of scales 4-7: its last members give all (or the lower part) of their
    rows to the gather chain, so the tile skips them (or clips them) while the earlier members run whole."""
    c, arrays = cascades("frontalface_alt")
    group = group_of(c, N, (4, 5, 6, 7), tile_split=tile_split)
    assert all(t.lead_scale_idx == 7 for t in group)
    assert group[0].tile_row_end == group[0].ny and group[-1].tile_row_end < group[-1].ny, [(t.tile_row_end, t.ny) for t in group]
    assert ((group[-1].tile_w * group[-1].tile_h + 63) // 64) % 8 == 5
    want = wanted(oracle, arrays, "frontalface_alt", N)
    with tunables(env, ("tile_split", tile_split)):
        timed = env.detect(c, frames())
        counted = env.detect(c, frames(), default_params(flags=VJ_FLAG_COUNTERS))
    check(timed, want, f"tile_split {tile_split} timed", False)
    check(counted, want, f"tile_split {tile_split} counted", True)
