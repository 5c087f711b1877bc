"""The tile kernel's wave-independent tail (tile_wave_tail): below tile_ws_min windows the wave-split finish deals the
tile's survivors to its eight waves, and each wave runs its own to the end of the cascade without a workgroup barrier.
Against the C oracle frame by frame: rectangles, per-stage counts and the stump / rectangle counts of counted runs, at
hand-over thresholds that give tails of one window, fewer than, exactly and more than one per wave, and large ones."""
import numpy as np
import pytest

from clfacedetection_amd import VJ_FLAG_COUNTERS, Environment, default_params, synth

pytestmark = pytest.mark.gpu

WS_MIN = (0, 1, 7, 8, 9, 48, 64, 256)
# drawn faces keep windows alive into the late stages (and into the in-order replay band); noise keeps many alive early
KINDS = (("faces", 41), ("noise", 42), ("faces", 43))
_FRAMES, _ORACLE = {}, {}


def frames(h, w):
    if (h, w) not in _FRAMES:
        _FRAMES[(h, w)] = np.stack([synth.frame(k, s, h, w) for k, s in KINDS])
    return _FRAMES[(h, w)]


def oracle_runs(oracle, cascades, name, f):
    key = (name, f.shape)
    if key not in _ORACLE:
        _, a = cascades(name)
        _ORACLE[key] = [oracle.detect(a, f[i]) for i in range(len(f))]
    return _ORACLE[key]


def assert_oracle(r, runs, what):
    for i, (ro, _) in enumerate(runs):
        mine = r.rects[r.rects["frame"] == i]
        assert len(mine) == len(ro) and all(np.array_equal(mine[k], ro[k]) for k in ("scale_idx", "x", "y", "w", "h")), \
            (what, i)
    entered = [sum(v) for v in zip(*[st["stage_entered"] for _, st in runs])]
    assert r.stage_entered == entered[:len(r.stage_entered)], what
    assert r.stump_evals == sum(st["stump_evals"] for _, st in runs), what
    assert r.gather_bytes == sum(st["gather_bytes"] for _, st in runs), what


@pytest.fixture
def fresh(monkeypatch):
    """A fresh environment per test (VJ_TILE_GROUP is read when one is created)."""
    made = []

    def make(group=None):
        if group is not None:
            monkeypatch.setenv("VJ_TILE_GROUP", str(group))
        e = Environment(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_default"])
def test_tail_thresholds_match_the_oracle(fresh, oracle, cascades, casc):
    """Every hand-over threshold, both LDS tile classes, with counters and without."""
    c, _ = cascades(casc)
    f = frames(1080, 1920)
    runs = oracle_runs(oracle, cascades, casc, f)
    e = fresh()
    for ws_min in WS_MIN:
        e.configure("tile_ws_min", ws_min)
        r = e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS))
        assert {l["lds_class"] for l in r.launches if l["kind"] == "tile"} == {0, 1}, ws_min
        assert_oracle(r, runs, ws_min)
        assert np.array_equal(e.detect(c, f).rects, r.rects), ws_min


@pytest.mark.parametrize("group", [1, 4])
def test_tail_with_tile_groups(fresh, oracle, cascades, group):
    """One scale per tile and groups of four step-2 scales on one tile: each member runs its own tail."""
    c, _ = cascades("frontalface_alt")
    f = frames(1080, 1920)
    runs = oracle_runs(oracle, cascades, "frontalface_alt", f)
    e = fresh(group)
    for ws_min in (1, 9, 48, 256):
        e.configure("tile_ws_min", ws_min)
        assert_oracle(e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS)), runs, (group, ws_min))


def test_tail_on_smaller_frames(fresh, oracle, cascades):
    """A frame size whose tiles are cut by the grid edge (partly filled tiles, fewer windows per tail)."""
    c, _ = cascades("frontalface_alt")
    f = frames(479, 641)
    runs = oracle_runs(oracle, cascades, "frontalface_alt", f)
    e = fresh()
    for ws_min in (7, 8, 64):
        e.configure("tile_ws_min", ws_min)
        assert_oracle(e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS)), runs, ws_min)


def test_tail_in_region_tiles(fresh, oracle, cascades):
    """The region pass's tiles share the tail: large regions on LDS tiles equal the oracle on each sub-image."""
    c, a = cascades("frontalface_alt")
    f = frames(1080, 1920)
    rois = [(0, 100, 50, 700, 500), (1, 0, 0, 960, 540), (2, 900, 400, 640, 480)]
    e = fresh()
    e.configure("roi_tiles", 512)
    for ws_min in (1, 9, 256):
        e.configure("tile_ws_min", ws_min)
        r = e.detect_rois(c, f, rois)
        for i, (fr, x, y, w, h) in enumerate(rois):
            ro, _ = oracle.detect(a, np.ascontiguousarray(f[fr][y:y + h, x:x + w]))
            mine = r.rects[r.rects["frame"] == i]
            assert len(mine) == len(ro) and all(np.array_equal(mine[k], ro[k]) for k in ("scale_idx", "x", "y", "w", "h")), \
                (ws_min, i)


@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
def test_tree_cascades_untouched(fresh, oracle, cascades, casc):
    """Two-node trees and the stage tree take the wave-split finish and the tree paths, never the stump tail."""
    c, _ = cascades(casc)
    f = frames(1080, 1920)
    e = fresh()
    e.configure("tile_ws_min", 48)
    assert_oracle(e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS)), oracle_runs(oracle, cascades, casc, f), casc)
