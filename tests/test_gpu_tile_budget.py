"""The tile shapes of round 11 (image tiles grown into the LDS of the former stump-parallel finish, intermediate widths and
heights) against the C oracle, frame by frame: rectangles and, in counted runs, per-stage counts, both exact.

Frames are 310 x 230: the window grid of the smallest scale is 145 x 105, so a 64 x 32 tile (and every other candidate
shape) leaves partial tiles at the right and at the bottom edge; from three frames on a call plans with the thresholds of
a batch, and the host plan query says that every tile scale of that plan has a shape or class the former search did not
give it (asserted below).  The region case runs 320 x 240 regions of the eye cascade, 150 x 110 windows."""
import numpy as np
import pytest

from cases import check_against_oracle, rows_of, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, Environment, default_params, synth
from clfacedetection_amd.api import VJ_PLAN_TILES_FORMER_SHAPES, VJ_PLAN_TILES_NO_GROUPS

pytestmark = pytest.mark.gpu

H, W = 230, 310
KINDS = ("noise", "faces", "blocks")
_FRAMES = {}
_ORACLE = {}


def frames_of(n, kinds=KINDS, seed0=1100):
    """a prefix of ONE set of distinct frames per kind tuple"""
    key = (kinds, seed0)
    if key not in _FRAMES or len(_FRAMES[key]) < n:
        _FRAMES[key] = synth.batch(max(n, 33 if kinds == KINDS else n), H, W, seed0=seed0, kinds=kinds)
    return _FRAMES[key][:n]


def oracle_runs(oracle, cascades, name, frames, tag):
    """[(rects, stats)] per frame, computed once per module and frame"""
    _, a = cascades(name)
    done = _ORACLE.setdefault((name, tag), [])
    while len(done) < len(frames):
        done.append(oracle.detect(a, frames[len(done)]))
    return done[:len(frames)]


def shapes(tiles):
    return [(t.lds_class, t.tile_w, t.tile_h, t.pitch, t.rows) for t in tiles]


def assert_new_shapes(c, n_frames, flags=0):
    """the plan of this call runs shapes the former search did not choose; returns (info, tiles)"""
    info, tiles = c.plan_tiles(W, H, n_frames, flags=flags)
    _, former = c.plan_tiles(W, H, n_frames, flags=flags | VJ_PLAN_TILES_FORMER_SHAPES)
    changed = [t.scale_idx for t, s0, s1 in zip(tiles, shapes(former), shapes(tiles)) if s0 != s1 and t.lds_class >= 0]
    print(f"{n_frames} frames: tile scales with a new shape or class: {changed}; blocks {list(info.class_lds)[:info.n_classes]}")
    assert changed
    t0 = tiles[0]
    assert t0.lds_class >= 0 and t0.nx % t0.tile_w and t0.ny % t0.tile_h, "partial tiles at both edges"
    return info, tiles


def assert_launch_lds(r, info):
    """the dynamic LDS of every tile launch is its class's block of the plan"""
    tile = [l for l in r.launches if l["kind"] == "tile"]
    assert tile
    for l in tile:
        print(f"tile launch class {l['lds_class']}: {l['lds_bytes']} B of LDS, scales {l['scales']}")
        assert l["lds_bytes"] == info.class_lds[l["lds_class"]], (l["lds_class"], l["lds_bytes"], list(info.class_lds))


@pytest.fixture
def fresh(monkeypatch):
    """make(VJ_SQ32=..., VJ_TILE_GROUP=...) -> a fresh environment (both are read when one is created); closed afterwards."""
    made = []

    def make(**envvars):
        for k in ("VJ_SQ32", "VJ_TILE_GROUP"):
            if k in envvars:
                monkeypatch.setenv(k, str(envvars[k]))
            else:
                monkeypatch.delenv(k, raising=False)
        e = Environment(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


@pytest.mark.parametrize("n", [8, 33])
def test_frontalface_alt_batches(fresh, oracle, cascades, n):
    """8 and 33 distinct frames: scale groups, the >= 8 and >= 32 frame defaults, the band-major queue pass."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(n)
    info, _ = assert_new_shapes(c, n)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    r, _ = check_against_oracle(fresh(), c, frames, want, f"{n} frames")
    assert_launch_lds(r, info)


def test_tile_end_at_the_first_pass_boundary(env, oracle, cascades):
    """tile_end 0: the tiles leave at the first pass boundary and hand every survivor to the queue pass."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    assert_new_shapes(c, 8)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    with tunables(env, ("tile_end", 0)):
        r, _ = check_against_oracle(env, c, frames, want, "tile_end 0")
    tile = [l for l in r.launches if l["kind"] == "tile"]
    queue = [l for l in r.launches if l["kind"] == "queue"]
    assert tile and queue and max(l["stage_end"] for l in tile) == min(l["stage_begin"] for l in queue)


@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
def test_tree_cascades(fresh, oracle, cascades, casc):
    """Two-node trees (the wave-split finish knows their shape) and the stage tree (prefix on tiles; a crowded tile hands
    its windows to the chains' queues): they share the planner, and their budget never held the phantom tables, so it is the
    intermediate sizes that give them new shapes."""
    c, _ = cascades(casc)
    frames = frames_of(5, ("faces", "blocks"), 1200)
    info, _ = assert_new_shapes(c, 5)
    want = oracle_runs(oracle, cascades, casc, frames, "fb")
    r, _ = check_against_oracle(fresh(), c, frames, want, casc)
    assert_launch_lds(r, info)


ROIS = [(0, 0, 0, 320, 240), (0, 16, 24, 200, 170), (1, 61, 30, 151, 149), (1, 3, 5, 317, 231)]


def test_region_tiles(fresh, oracle, cascades):
    """vj_detect_rois: the regions' small scales run on cascade_tile_roi_pass in every scale's OWN shape, with the class-0
    block of the plan; then vj_detect_chain, whose second half is the same pass on device-built regions."""
    eye, eye_a = cascades("eye")
    face, _ = cascades("frontalface_alt2")
    frames = np.stack([synth.frame("faces", 5, 240, 320), synth.frame("blocks", 8, 240, 320)])
    info, tiles = eye.plan_tiles(320, 240, 1 << 20)
    _, former = eye.plan_tiles(320, 240, 1 << 20, flags=VJ_PLAN_TILES_FORMER_SHAPES)
    own0 = [(t.tile_w, t.tile_h) for t in tiles if t.lds_class == 0]
    assert own0 and own0 != [(t.tile_w, t.tile_h) for t in former if t.lds_class == 0]
    assert all(t.pitch * t.rows * 4 + info.header_bytes <= info.class_lds[0] for t in tiles if t.lds_class == 0)
    want = [oracle.detect(eye_a, np.ascontiguousarray(frames[f][y:y + h, x:x + w])) for f, x, y, w, h in ROIS]
    e = fresh()
    for roi_tiles in (512, 64):
        e.configure("roi_tiles", roi_tiles)
        r = e.detect_rois(eye, frames, ROIS, default_params(flags=VJ_FLAG_COUNTERS))
        r2 = e.detect_rois(eye, frames, ROIS)
        for i, (ro, _) in enumerate(want):
            assert rows_of(r.rects[r.rects["frame"] == i]) == rows_of(ro), (roi_tiles, ROIS[i])
        assert np.array_equal(r.rects, r2.rects), roi_tiles
        assert r.stage_entered == [sum(v) for v in zip(*[st["stage_entered"] for _, st in want])], roi_tiles
        assert r.windows == sum(st["windows"] for _, st in want), roi_tiles
    e.configure("defaults", "")
    got = e.detect_chain(face, eye, frames)
    e.configure("roi_tiles", 0)      # the same regions without region tiles
    ref = e.detect_chain(face, eye, frames)
    assert np.array_equal(got[0].rects, ref[0].rects) and np.array_equal(got[1].rects, ref[1].rects)
    cand = got[0].rects
    assert len(cand), "the drawn faces give the chain candidates"
    for k in range(min(len(cand), 6)):   # the first regions against the oracle on their crops
        q = cand[k]
        crop = np.ascontiguousarray(frames[q["frame"]][q["y"]:q["y"] + q["h"], q["x"]:q["x"] + q["w"]])
        assert rows_of(got[1].rects[got[1].rects["frame"] == k]) == rows_of(oracle.detect(eye_a, crop)[0]), k


@pytest.mark.parametrize("envvar,plan_flags", [("VJ_SQ32", 0), ("VJ_TILE_GROUP", VJ_PLAN_TILES_NO_GROUPS)])
def test_diagnostic_switches(fresh, oracle, cascades, envvar, plan_flags):
    """VJ_SQ32=0: 64-bit squared-sum corners on every scale; VJ_TILE_GROUP=1: one tile per scale, every scale in its own shape."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(8)
    info, _ = assert_new_shapes(c, 8, plan_flags)
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "mix")
    r, _ = check_against_oracle(fresh(**{envvar: 0 if envvar == "VJ_SQ32" else 1}), c, frames, want, f"{envvar} off")
    assert_launch_lds(r, info)


def test_candidate_heavy_content(fresh, oracle, cascades):
    """Blocks and drawn faces only: tiles of up to 2048 windows carry more survivors into the re-packs, the wave-split finish
    and the tail than the former shapes held."""
    c, _ = cascades("frontalface_alt")
    frames = frames_of(6, ("blocks", "faces"), 1300)
    info, tiles = assert_new_shapes(c, 6)
    assert max(t.tile_w * t.tile_h for t in tiles if t.lds_class >= 0) == 2048
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "heavy")
    r, entered = check_against_oracle(fresh(), c, frames, want, "blocks / faces")
    assert_launch_lds(r, info)
    deep = [sum(l["stage_entered"][s] for l in r.launches if l["kind"] == "tile") for s in range(c.info.n_stages)]
    print("windows entering each stage inside tile launches:", deep)
    assert deep[3] > 0 and deep[-1] > 0, "survivors reach the finish stages and the last stage inside the tiles"
