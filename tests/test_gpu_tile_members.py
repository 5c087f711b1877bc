"""The members of a scale group without a barrier between them, and whole-chunk dealing, against the C oracle frame by
frame (the whole rectangle list and, in the counted run, per-stage counts).

Where a member of a group that is not its last ends in the wave-independent tail — or in the wave-split finish with nothing
left, or with only wave 0's detections — its waves go on to the next member's variance fill and first stages without waiting
for the workgroup's slowest tail; the tail's scratch then lives in the wave's own queue region behind one barrier after the
windows are dealt.  A wave's share of a tile is a whole number of 64-window chunks.  Neither changes a result:

  * 320 x 240 and 200 x 160 frames (four-member step-2 groups: asserted from the plan), 1 frame and 9 (the band-major queue
    pass), drawn faces and blocks (survivors reach the tail in several members of a tile) and noise (most members end with
    nothing left), VJ_TILE_GROUP 1 against 4;
  * tile_ws_min 0 (the finish runs to the end: the tail is never entered) and 256 (the tail is entered from as many windows
    as it takes), tile_ws_max 0 (no finish at all: every member ends in the dense sweep and keeps its barriers);
  * a tile_split that cuts a group: a member is skipped on some tiles and on all tiles of the members behind it;
  * tile shapes whose chunk count does not divide by the eight waves (asserted from the plan);
  * the region tile pass (vj_detect_chain) and the stage tree, which never relax."""
import numpy as np
import pytest

from cases import check_against_oracle, rows_of, tunables
from clfacedetection_amd import Environment, synth

pytestmark = pytest.mark.gpu

SIZES = ((240, 320), (160, 200))                 # (height, width)
KINDS = ("faces", "blocks", "noise")
SEED0 = 40
_FRAMES, _ORACLE = {}, {}


def frame_of(kind, seed, h, w):
    if (kind, seed, h, w) not in _FRAMES:
        _FRAMES[kind, seed, h, w] = synth.frame(kind, seed, h, w)
    return _FRAMES[kind, seed, h, w]


def batch_of(which, h, w):
    """"faces" / "blocks" / "noise": one frame of that kind; "nine": nine distinct frames, the kinds cycling."""
    if which == "nine":
        return np.stack([frame_of(KINDS[i % 3], SEED0 + i, h, w) for i in range(9)])
    return np.stack([frame_of(which, SEED0 + KINDS.index(which), h, w)])


def oracle_of(oracle, cascades, name, frames):
    """[(rects, stats)] per frame; every frame is run once per module."""
    _, a = cascades(name)
    out = []
    for f in frames:
        key = (name, f.shape, f.tobytes())
        if key not in _ORACLE:
            _ORACLE[key] = oracle.detect(a, f)
        out.append(_ORACLE[key])
    return out


@pytest.fixture
def fresh(monkeypatch):
    """make(group) -> a fresh environment with VJ_TILE_GROUP = group (read when one is created; None: unset); closed and the
    variable removed after the test."""
    made = []

    def make(group=None):
        if group is None:
            monkeypatch.delenv("VJ_TILE_GROUP", raising=False)
        else:
            monkeypatch.setenv("VJ_TILE_GROUP", str(group))
        e = Environment(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()
    monkeypatch.delenv("VJ_TILE_GROUP", raising=False)


def groups_of(tiles):
    """lead scale -> member scales, for the groups of more than one member."""
    g = {}
    for t in tiles:
        if t.tile_w:
            g.setdefault(t.lead_scale_idx, []).append(t)
    return {k: v for k, v in g.items() if len(v) > 1}


# ----------------------------------------------------------------------------- 1. members of a group, every content
@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("which", ["faces", "blocks", "noise", "nine"])
@pytest.mark.parametrize("h,w", SIZES)
def test_group_members(fresh, oracle, cascades, h, w, which, group):
    c, _ = cascades("frontalface_alt")
    frames = batch_of(which, h, w)
    _, tiles = c.plan_tiles(w, h, len(frames))
    g = groups_of(tiles)
    assert g and all(len(v) == 4 for v in g.values()), "the shipped plan forms four-member groups at this size"
    # the groups' tiles (the lead's shape) hold a chunk count that the eight waves do not share evenly
    leads = [next(t for t in v if t.scale_idx == k) for k, v in g.items()]
    assert any(((t.tile_w * t.tile_h + 63) // 64) % 8 for t in leads), [(t.tile_w, t.tile_h) for t in leads]
    want = oracle_of(oracle, cascades, "frontalface_alt", frames)
    r, _ = check_against_oracle(fresh(group), c, frames, want, f"{w}x{h} {which} VJ_TILE_GROUP={group}")
    assert any(l["kind"] == "tile" for l in r.launches)
    if which in ("faces", "nine"):
        assert len(r.rects) > 0, "the drawn faces are found: windows ran to the cascade's end"


# ----------------------------------------------------------------------------- 2. how a member ends
@pytest.mark.parametrize("key,value", [("tile_ws_min", 0), ("tile_ws_min", 256), ("tile_ws_max", 0)])
@pytest.mark.parametrize("which", ["faces", "nine"])
def test_member_ends(env, oracle, cascades, which, key, value):
    """tile_ws_min 0: the wave-split finish takes every tile to the cascade's end, detections included; 256: the tail
    starts from up to 255 windows, 32 per wave; tile_ws_max 0: neither runs."""
    c, _ = cascades("frontalface_alt")
    h, w = SIZES[0]
    frames = batch_of(which, h, w)
    want = oracle_of(oracle, cascades, "frontalface_alt", frames)
    with tunables(env, (key, value)):
        assert int(env.query(key)) == value
        check_against_oracle(env, c, frames, want, f"{which} {key}={value}")
    assert int(env.query(key)) != value      # (back at its default)


# ----------------------------------------------------------------------------- 3. skipped members
@pytest.mark.parametrize("split", ["7.5", "11.5"])
def test_members_cut_by_the_chain_balance(env, oracle, cascades, split):
    """A tile_split that ends inside a group: the member at the cut runs on the first tile rows only, the members behind it
    on none — a relaxed member is then followed by skipped ones, up to the end of the tile."""
    c, _ = cascades("frontalface_alt")
    h, w = SIZES[0]
    frames = batch_of("nine", h, w)
    _, tiles = c.plan_tiles(w, h, len(frames), tile_split=float(split))
    cut = [v for v in groups_of(tiles).values()
           if any(t.tile_row_end < t.ny for t in v) and any(t.tile_row_end > 0 for t in v)]
    assert cut, f"tile_split {split} cuts no group"
    print(f"tile_split {split}: " + "; ".join(str([(t.scale_idx, t.tile_row_end, t.ny) for t in v]) for v in cut))
    want = oracle_of(oracle, cascades, "frontalface_alt", frames)
    with tunables(env, ("tile_split", split)):
        check_against_oracle(env, c, frames, want, f"tile_split {split}")


# ----------------------------------------------------------------------------- 4. uneven chunks
def test_uneven_chunks(env, oracle, cascades):
    """333 x 251: no grid is a multiple of its tile, so edge tiles are partly empty in both directions; the plan's shapes give
    chunk counts (28, 21, 18, 13, ... ) that leave the eight waves different numbers of chunks, a last chunk partly filled."""
    c, _ = cascades("frontalface_alt")
    frames = np.stack([frame_of("blocks", SEED0 + 20, 251, 333), frame_of("faces", SEED0 + 21, 251, 333)])
    _, tiles = c.plan_tiles(333, 251, len(frames))
    shapes = {(t.tile_w, t.tile_h) for t in tiles if t.tile_w}
    assert any((tw * th) % 64 for tw, th in shapes) and any(((tw * th + 63) // 64) % 8 for tw, th in shapes), shapes
    want = oracle_of(oracle, cascades, "frontalface_alt", frames)
    check_against_oracle(env, c, frames, want, "333x251")


# ----------------------------------------------------------------------------- 5. kernels that do not relax
def test_region_pass_unchanged(env, oracle, cascades):
    """vj_detect_chain on two frames: the second cascade runs inside device-built regions on cascade_tile_roi_pass (one
    member per tile), whose tiles take the new dealing."""
    face, _ = cascades("frontalface_alt2")
    eye, eye_a = cascades("eye")
    frames = np.stack([frame_of("faces", 5, 240, 320), frame_of("blocks", 8, 240, 320)])
    with tunables(env, ("roi_tiles", 64)):
        got = env.detect_chain(face, eye, frames)
    cand = got[0].rects
    assert len(cand), "the drawn faces give the chain candidates"
    for k in range(min(len(cand), 6)):
        q = cand[k]
        crop = np.ascontiguousarray(frames[q["frame"]][q["y"]:q["y"] + q["h"], q["x"]:q["x"] + q["w"]])
        assert rows_of(got[1].rects[got[1].rects["frame"] == k]) == rows_of(oracle.detect(eye_a, crop)[0]), k


def test_stage_tree_unchanged(env, oracle, cascades):
    c, _ = cascades("frontalface_alt_tree")
    frames = batch_of("faces", *SIZES[0])
    want = oracle_of(oracle, cascades, "frontalface_alt_tree", frames)
    r, _ = check_against_oracle(env, c, frames, want, "frontalface_alt_tree")
    assert any(l["kind"] == "tile" for l in r.launches)
