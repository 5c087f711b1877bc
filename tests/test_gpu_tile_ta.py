"""The two global-load changes of the tile kernel that take work off the texture-address unit, against the C oracle frame
by frame (rectangles and, in counted runs, per-stage counts):

  * the wave-independent tail (tile_wave_tail) loads its stump records from a block-transposed copy of the tile tables —
    stages of one to four blocks, every last block padded;
  * the variance's squared-sum corners are read as dwords where the window area keeps the sum below 2^32
    (ScaleDev::sq32), and as 64-bit words otherwise — VJ_SQ32=0, read when an environment is created, keeps every scale
    on the 64-bit form, which no shipped cascade reaches by itself on a tile scale.

Only where two sets of loads read from and how wide they are differs: every result is the oracle's."""
import numpy as np
import pytest

from cases import check_against_oracle, rows_of
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_TILTED_AS_UPRIGHT, Environment, default_params, synth

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle_runs(oracle, cascades, name, frames, tag):
    """[(rects, stats)] per frame, computed once per module."""
    if (name, tag) not in _ORACLE:
        _, a = cascades(name)
        _ORACLE[name, tag] = [oracle.detect(a, f) for f in frames]
    return _ORACLE[name, tag]


@pytest.fixture
def fresh(monkeypatch):
    """make(sq32) -> a fresh environment (VJ_SQ32 is read when one is created); closed after the test."""
    made = []

    def make(sq32=None):
        if sq32 is None:
            monkeypatch.delenv("VJ_SQ32", raising=False)
        else:
            monkeypatch.setenv("VJ_SQ32", str(sq32))
        e = Environment(0)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


# ----------------------------------------------------------------------------- 1. tail blocks
# frontalface_alt's stages reach 213 stumps: up to four blocks, and no stage fills its last block.  The seeds were chosen
# with the oracle: the drawn face of ("faces", 5) keeps 30 windows alive through the last stage, all of them at the small
# scales that a 160 x 120 frame runs on tiles, and fewer than the default hand-over threshold in the whole frame pair —
# so whichever tile ran them there was below tile_ws_min, i.e. in the tail.
TAIL_FRAMES = (("faces", 5), ("blocks", 8))
TAIL_WS_MIN = (48, 256)    # the default and the largest value the key takes


@pytest.mark.parametrize("ws_min", TAIL_WS_MIN)
def test_tail_blocks(fresh, oracle, cascades, ws_min):
    c, a = cascades("frontalface_alt")
    frames = np.stack([synth.frame(k, s, 120, 160) for k, s in TAIL_FRAMES])
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "tail")
    e = fresh()
    assert int(e.query("tile_ws_min")) == TAIL_WS_MIN[0]
    e.configure("tile_ws_min", ws_min)
    r, entered = check_against_oracle(e, c, frames, want, f"tail blocks, tile_ws_min={ws_min}")
    big = [s for s, n in enumerate(a.stage_n_trees) if n > 128]
    assert big and a.stage_n_trees[big[-1]] == 213
    in_tiles = [sum(l["stage_entered"][s] for l in r.launches if l["kind"] == "tile") for s in range(c.info.n_stages)]
    print(f"tile_ws_min={ws_min}: windows entering stages {big} inside tile launches: {[in_tiles[s] for s in big]}, "
          f"in all launches: {[entered[s] for s in big]}")
    # the wave-split finish only runs a stage for a tile that still holds >= tile_ws_min windows: fewer than that in ALL
    # tile launches together means every one of them ran that stage in the tail
    assert any(0 < in_tiles[s] < ws_min for s in big), (big, [in_tiles[s] for s in big])
    assert 0 < in_tiles[big[-1]] < ws_min, in_tiles[big[-1]]


# ----------------------------------------------------------------------------- 2. trees take other paths
@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
def test_tree_cascades_unchanged(fresh, oracle, cascades, casc):
    """Two-node trees (wave-split finish to the end) and the stage tree (chains inside the tile) never read the tail table."""
    c, _ = cascades(casc)
    frames = np.stack([synth.frame("faces", 5, 120, 160)])
    want = oracle_runs(oracle, cascades, casc, frames, "trees")
    r, _ = check_against_oracle(fresh(), c, frames, want, casc)
    assert any(l["kind"] == "tile" for l in r.launches), casc


# ----------------------------------------------------------------------------- 3. / 4. squared sums at their maximum
def flat_frames():
    return np.stack([np.full((96, 128), 255, np.uint8), np.zeros((96, 128), np.uint8)])


@pytest.mark.parametrize("casc", ["frontalface_default", "mcs_upperbody", "mcs_eyepair_big"])   # 24 x 24, 22 x 20, 45 x 11
def test_squared_sums_at_their_maximum(fresh, oracle, cascades, casc):
    """An all-255 frame: every window's squared sum is 65025 * area, the largest a window of its size can have (and the
    variance is exactly 0); an all-0 frame: the smallest.  All scales; dword corners, then the 64-bit fallback forced
    (VJ_SQ32=0): both equal the oracle, and each other."""
    c, a = cascades(casc)
    assert (a.win_w, a.win_h) in ((24, 24), (22, 20), (45, 11))
    frames = flat_frames()
    want = oracle_runs(oracle, cascades, casc, frames, "flat")
    out = {}
    for sq32 in (None, 0):
        e = fresh(sq32)
        if a.node_tilted.any():   # (every shipped non-square cascade has tilted features, which this profile reads as upright
            # ones exactly as the reference and the oracle do: the flag says so)
            r = e.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS | VJ_FLAG_TILTED_AS_UPRIGHT))
            for i, (ro, _) in enumerate(want):
                assert rows_of(r.rects[r.rects["frame"] == i]) == rows_of(ro), (casc, sq32, i)
            assert r.stage_entered == [sum(v) for v in zip(*[st["stage_entered"] for _, st in want])], (casc, sq32)
            assert r.windows == sum(st["windows"] for _, st in want), (casc, sq32)
            r2 = e.detect(c, frames, default_params(flags=VJ_FLAG_TILTED_AS_UPRIGHT))
            assert np.array_equal(r2.rects, r.rects), (casc, sq32)
        else:
            r, _ = check_against_oracle(e, c, frames, want, f"{casc} VJ_SQ32={sq32}")
        tile_scales = sorted({k for l in r.launches if l["kind"] == "tile" for k in l["scales"]})
        print(f"{casc} VJ_SQ32={sq32}: tile scales {tile_scales}, windows {r.windows}")
        assert tile_scales, "no scale of this frame ran on tiles"
        out[sq32] = r
    assert np.array_equal(out[None].rects, out[0].rects)
    assert out[None].stage_entered == out[0].stage_entered and out[None].windows == out[0].windows


@pytest.mark.parametrize("sq32", [None, 0])
def test_fallback_on_content(fresh, oracle, cascades, sq32):
    """The same switch on frames with content (drawn face, blocks): variances that are not 0."""
    c, _ = cascades("frontalface_alt")
    frames = np.stack([synth.frame(k, s, 120, 160) for k, s in TAIL_FRAMES])
    want = oracle_runs(oracle, cascades, "frontalface_alt", frames, "tail")
    check_against_oracle(fresh(sq32), c, frames, want, f"VJ_SQ32={sq32}")


# ----------------------------------------------------------------------------- 5. the region tile pass
ROIS = [(0, 0, 0, 320, 240), (0, 16, 24, 200, 170), (0, 61, 30, 151, 149)]


@pytest.mark.parametrize("sq32", [None, 0])
def test_region_tile_pass(fresh, oracle, cascades, sq32):
    """vj_detect_rois, three regions of different sizes on one frame: their small scales run on cascade_tile_roi_pass (with the
    default threshold and with one that sends every grid of >= 64 windows to tiles), the result is the oracle's on each crop."""
    eye, eye_a = cascades("eye")
    frames = np.stack([synth.frame("faces", 5, 240, 320)])
    want = [oracle.detect(eye_a, np.ascontiguousarray(frames[f][y:y + h, x:x + w])) for f, x, y, w, h in ROIS]
    e = fresh(sq32)
    for roi_tiles in (512, 64, 0):
        e.configure("roi_tiles", roi_tiles)
        r = e.detect_rois(eye, frames, ROIS, default_params(flags=VJ_FLAG_COUNTERS))
        r2 = e.detect_rois(eye, frames, ROIS)
        for i, (ro, _) in enumerate(want):
            assert rows_of(r.rects[r.rects["frame"] == i]) == rows_of(ro), (roi_tiles, ROIS[i])
        assert np.array_equal(r.rects, r2.rects), roi_tiles
        assert r.stage_entered == [sum(v) for v in zip(*[st["stage_entered"] for _, st in want])], roi_tiles
        assert r.windows == sum(st["windows"] for _, st in want), roi_tiles
