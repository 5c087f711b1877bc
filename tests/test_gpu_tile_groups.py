"""Scale groups of the LDS-tile kernel (VJ_TILE_GROUP, read when an environment is created): consecutive step-2 tile
scales share one staged tile.  Only LDS addresses move, so rectangles and every counter equal the one-tile-per-scale
plan (VJ_TILE_GROUP=1) for every group size, and the oracle."""
import numpy as np
import pytest

from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_SKIP_LIST, Environment, default_params, synth

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 4, 8)
_FRAMES = {}


def frames(n, h, w, seed0=1):
    key = (n, h, w, seed0)
    if key not in _FRAMES:
        _FRAMES[key] = synth.batch(n, h, w, seed0=seed0)
    return _FRAMES[key]


def run_groups(monkeypatch, calls):
    """calls(env) -> list of DetectResult, in a fresh environment per group size; returns {G: results}."""
    out = {}
    for g in GROUPS:
        monkeypatch.setenv("VJ_TILE_GROUP", str(g))
        e = Environment(0)
        try:
            out[g] = calls(e)
        finally:
            e.close()
    monkeypatch.delenv("VJ_TILE_GROUP")
    return out


def assert_same(out):
    base = out[1]
    for g, rs in out.items():
        for i, (r, b) in enumerate(zip(rs, base)):
            assert np.array_equal(r.rects, b.rects), (g, i)
            assert r.stage_entered == b.stage_entered and r.windows == b.windows and r.stump_evals == b.stump_evals, (g, i)


@pytest.mark.parametrize("n,h,w", [(64, 1080, 1920), (8, 1080, 1920), (1, 1080, 1920), (3, 479, 641), (2, 1081, 1917)])
def test_group_sizes_agree(monkeypatch, cascades, n, h, w):
    """Batches of distinct frames (the bench's mix), at the three batch-size classes of the chain balance and at odd sizes:
    with counters and without, every group size gives the rectangles and counters of the one-tile-per-scale plan."""
    c, _ = cascades("frontalface_alt")
    f = frames(n, h, w)
    out = run_groups(monkeypatch, lambda e: [e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS)), e.detect(c, f)])
    assert_same(out)
    for g, (rc, rp) in out.items():
        assert np.array_equal(rc.rects, rp.rects), g
    if n == 64:
        assert len(out[1][0].rects) > 0


def test_group_members_whose_rows_moved_to_the_gather_chain(monkeypatch, cascades):
    """A scale mask whose tile_split moves rows of grouped scales to the global-gather chain: a group tile skips the rows a
    member handed over, and that member's gather units start where they do without groups."""
    c, _ = cascades("frontalface_alt")
    f = frames(16, 1080, 1920, seed0=7)

    def calls(e):
        res = []
        for split in ("1.5", "3.5", "0"):
            e.configure("tile_split", split)
            res.append(e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS, scales=range(0, 6))))
        e.configure("tile_split", "reset")
        return res
    out = run_groups(monkeypatch, calls)
    assert_same(out)
    assert out[1][0].rects.size == out[1][2].rects.size


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_default"])
def test_skip_bits_and_second_cascade(monkeypatch, cascades, casc):
    """VJ_FLAG_SKIP_LIST (the tile kernel reads each member's own skip bits) and frontalface_default (a different reach)."""
    c, _ = cascades(casc)
    f = frames(4, 720, 1280, seed0=3)
    out = run_groups(monkeypatch, lambda e: [e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS | VJ_FLAG_SKIP_LIST)),
                                             e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS))])
    assert_same(out)


def test_groups_match_the_oracle(monkeypatch, oracle, cascades):
    """Two 1080p frames with the largest group against the CPU oracle: rectangles and per-stage counts."""
    c, a = cascades("frontalface_alt")
    f = frames(2, 1080, 1920, seed0=11)
    monkeypatch.setenv("VJ_TILE_GROUP", "8")
    e = Environment(0)
    try:
        r = e.detect(c, f, default_params(flags=VJ_FLAG_COUNTERS))
    finally:
        e.close()
    entered = [0] * c.info.n_stages
    for i in range(len(f)):
        ro, st = oracle.detect(a, f[i])
        mine = r.rects[r.rects["frame"] == i]
        assert len(mine) == len(ro) and all(np.array_equal(mine[k], ro[k]) for k in ("scale_idx", "x", "y", "w", "h")), i
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
    assert r.stage_entered == entered
