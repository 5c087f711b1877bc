"""The gather chain's linear kernels at 4, 5, 6 and 8 waves per workgroup (gather_waves): above four the waves divide the same
16 KiB of LDS into shorter queues (512 entries up to 4 waves, 384 at 5, 320 at 6, 256 at 7 and 8: csrc/vj_gather_queue.hpp), the
plan cuts its first-pass units to that capacity, and the stump-parallel tail's scratch has to fit the shorter queue.  Results
never depend on the wave count: every call is compared with the C oracle frame by frame — rectangles, and the per-stage counts
of a counted run — and with the same call at gather_waves 4.

Frames of 320 x 240 and 640 x 480 (drawn faces, noise, blocks); 1, 3 and 9 frames: nine take the band-major queue pass, three the
chunked one, one frame the single-frame defaults.  The last test fills a wave's queue at 256 entries, so that the band-major pass
sweeps what it holds before it loads a group's next run: survivor_cascade() with a prefix of three accept-all stages on
dot_frame() content and a pass boundary at stage 3 — every window of the grid pass enters stage 3 (asserted on the CPU with the
oracle, then from the counted run), and the plan has gather scales at least 64 windows wide, whose horizontally adjacent units
(32 x 8 windows each at 256 entries, same band, same scale, consecutive in the unit list) share a group: q_group_units = 4 counts
units of 512 windows, two units of 256 at eight waves — 512 windows for a queue of 256; q_group_units 8 and 16 make groups of
four and eight such units."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cases import cascade_to_product, dot_frame, first_difference, rows_of, survivor_cascade, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, Environment, default_params, synth

gpu = pytest.mark.gpu

SIZES = {"320x240": (240, 320), "640x480": (480, 640)}       # (height, width)
COUNTS = (1, 3, 9)
WAVES = (4, 5, 6, 8)
N_SET = 9
KINDS = ("faces", "noise", "blocks")                          # (a frame of drawn faces first: every prefix has detections)
ALL_GATHER = (("tile_min_windows", 65536), ("tile_accept_windows", 65536))   # no scale qualifies for LDS tiles
FILL_CAP = 256                                                # entries of a wave's queue at 8 waves
_CACHE = {}


def frames_of(size):
    if ("frames", size) not in _CACHE:
        h, w = SIZES[size]
        _CACHE["frames", size] = synth.batch(N_SET, h, w, seed0=8100 + h, kinds=KINDS)
    return _CACHE["frames", size]


def oracle_of(oracle, cascades, casc, size):
    """[(rects, stats)] of the oracle for the nine frames, computed once per (cascade, size)."""
    if ("oracle", casc, size) not in _CACHE:
        _, a = cascades(casc)
        with ThreadPoolExecutor(N_SET) as ex:        # (the C entry point releases the GIL)
            _CACHE["oracle", casc, size] = list(ex.map(lambda f: oracle.detect(a, f), frames_of(size)))
    return _CACHE["oracle", casc, size]


def check(e, c, frames, want, label, counted=True):
    """A counted and a timed vj_detect against the oracle's per-frame results; returns the counted result."""
    r = e.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS))
    entered, windows = [0] * c.info.n_stages, 0
    for i, (ro, st) in enumerate(want):
        mine = rows_of(r.rects[r.rects["frame"] == i])
        assert mine == rows_of(ro), f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: {first_difference(r.stage_entered, entered)}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"
    r2 = e.detect(c, frames)
    assert np.array_equal(r2.rects, r.rects), f"{label}: the timed kernels' rectangles differ from the counted ones"
    return r


@gpu
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("size", list(SIZES))
def test_wave_counts_against_the_oracle_and_four_waves(env, oracle, cascades, size, n):
    c, _ = cascades("frontalface_alt")
    frames, want = frames_of(size)[:n], oracle_of(oracle, cascades, "frontalface_alt", size)[:n]
    assert sum(len(ro) for ro, _ in want) > 0 and sum(st["stage_entered"][3] for _, st in want) > 0, "the frames let nothing through"
    for extra in ((), ALL_GATHER):
        for conc in (1, 0):
            base = None
            for waves in WAVES:
                label = f"{size} n={n} gather_waves={waves} concurrent={conc} {dict(extra)}"
                with tunables(env, ("gather_waves", waves), ("concurrent", conc), *extra):
                    r = check(env, c, frames, want, label)
                kinds = [l["kind"] for l in r.launches]
                assert "grid" in kinds, f"{label}: {kinds}"
                if extra:
                    assert "tile" not in kinds, f"{label}: {kinds}"
                if n >= 3:      # (a single frame may finish in the grid pass's tail)
                    assert any(l["kind"] == "queue" and sum(l["stage_entered"]) > 0 for l in r.launches), f"{label}: no queue pass ran"
                if base is None:
                    base = r
                assert np.array_equal(r.rects, base.rects), f"{label}: rectangles differ from gather_waves=4"
                assert r.stage_entered == base.stage_entered, label


@gpu
@pytest.mark.parametrize("tail", [0, 24, 48])
def test_stump_parallel_tail_at_eight_waves(env, oracle, cascades, tail):
    """sp_tail_max 48 at eight waves is clamped to the 24 windows whose scratch a queue of 256 entries holds (48 entries and
    48 x 9 verdict words would reach 1792 bytes into the next wave's queue); 0 turns the tail off."""
    c, _ = cascades("frontalface_alt")
    for n in (1, 9):
        frames, want = frames_of("640x480")[:n], oracle_of(oracle, cascades, "frontalface_alt", "640x480")[:n]
        for extra in ((), ALL_GATHER):
            with tunables(env, ("gather_waves", 8), ("sp_tail_max", tail), *extra):
                assert env.query("sp_tail_max") == str(tail)
                check(env, c, frames, want, f"sp_tail_max={tail} n={n} {dict(extra)}")


@gpu
@pytest.mark.parametrize("waves", [6, 8])
def test_sub_batches(env, oracle, cascades, waves):
    """Five frames in sub-batches of two: the call's plan, and two-frame launches inside it."""
    c, _ = cascades("frontalface_alt")
    frames, want = frames_of("640x480")[:5], oracle_of(oracle, cascades, "frontalface_alt", "640x480")[:5]
    with tunables(env, ("gather_waves", waves), ("max_subbatch", 2)):
        check(env, c, frames, want, f"sub-batches gather_waves={waves}")
    frames, want = frames_of("640x480"), oracle_of(oracle, cascades, "frontalface_alt", "640x480")
    with tunables(env, ("gather_waves", waves), ("max_subbatch", 2)):     # nine frames: the plan of a batch, launches of two
        check(env, c, frames, want, f"sub-batches of a batch gather_waves={waves}")


@gpu
@pytest.mark.parametrize("waves_at_create,waves_at_submit", [(8, 8), (-1, 8), (8, -1), (6, 5)])
def test_stream_with_two_batches_in_flight(oracle, cascades, waves_at_create, waves_at_submit):
    """vj_stream: two different batches submitted before the first is collected.  The stream's plan is cut when it is created; a
    wave count configured afterwards must not run more waves than that plan's units fit (created at the defaults, 512-window
    units: at most four waves whatever is configured later)."""
    c, _ = cascades("frontalface_alt")
    size = "640x480"
    frames, want = frames_of(size), oracle_of(oracle, cascades, "frontalface_alt", size)
    h, w = SIZES[size]
    batches = (np.arange(9), np.array([8, 2, 5, 1, 7, 0, 3, 6]))
    e = Environment(0)
    try:
        e.configure("gather_waves", waves_at_create)
        s = e.stream(c, w, h, N_SET, default_params())
        try:
            e.configure("gather_waves", waves_at_submit)
            for _ in range(2):          # (the second round reuses both lanes)
                for b in batches:
                    s.submit(frames[b])
                for b in batches:
                    r = s.collect()
                    for i, k in enumerate(b):
                        mine = rows_of(r.rects[r.rects["frame"] == i])
                        assert mine == rows_of(want[k][0]), f"stream {waves_at_create}/{waves_at_submit}: frame {k}: {len(mine)} rectangles, the oracle {len(want[k][0])}"
        finally:
            s.close()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("casc", ["frontalface_alt2", "frontalface_alt_tree"])
def test_trees_and_the_stage_tree_at_eight_waves(env, oracle, cascades, casc):
    """frontalface_alt2 (two-node trees) runs the linear kernels at eight waves; frontalface_alt_tree keeps the stage-tree layout
    (three waves, 512-entry queues) whatever gather_waves says."""
    c, _ = cascades(casc)
    for n in (3, 9):
        frames, want = frames_of("640x480")[:n], oracle_of(oracle, cascades, casc, "640x480")[:n]
        with tunables(env, ("gather_waves", 4)):
            base = check(env, c, frames, want, f"{casc} n={n} gather_waves=4")
        for extra in ((), ALL_GATHER):
            with tunables(env, ("gather_waves", 8), *extra):
                r = check(env, c, frames, want, f"{casc} n={n} gather_waves=8 {dict(extra)}")
            assert np.array_equal(r.rects, base.rects) and r.stage_entered == base.stage_entered, (casc, n)


# ----------------------------------------------------------------------------- a wave's queue filled at 256 entries
def fill_case():
    if "fill" not in _CACHE:
        a = survivor_cascade("stumps", n_pass=3)
        h, w = SIZES["640x480"]
        _CACHE["fill"] = (cascade_to_product(a), a, [dot_frame(8300 + i, h, w, n_dots=(h * w) // 4000) for i in range(N_SET)])
    return _CACHE["fill"]


def fill_oracle(oracle):
    if "fill_oracle" not in _CACHE:
        _, a, frames = fill_case()
        with ThreadPoolExecutor(N_SET) as ex:
            _CACHE["fill_oracle"] = list(ex.map(lambda f: oracle.detect(a, f, cap=1 << 21), frames))
    return _CACHE["fill_oracle"]


def test_fill_content_sends_every_window_into_stage_3(oracle):
    """(CPU.)  The oracle on the chosen content: every window of every frame enters stage 3, few leave it; and the nine-frame plan
    has gather scales at least 64 windows wide with 8 rows or more left to the gather chain: two full units of 32 x 8 = 256
    windows side by side in one band, one group, 512 windows entering stage 3 for a queue of 256."""
    c, _, _ = fill_case()
    for _, st in fill_oracle(oracle):
        assert st["stage_entered"][3] == st["stage_entered"][0] == st["windows"] > 0
    assert 0 < sum(len(ro) for ro, _ in fill_oracle(oracle)) < sum(st["windows"] for _, st in fill_oracle(oracle)) // 20
    h, w = SIZES["640x480"]
    for split in (-1.0, 99.0):       # the shipped balance, and every scale a gather scale
        _, tiles = c.plan_tiles(w, h, N_SET, tile_split=split)
        wide = [t for t in tiles if t.nx >= 64 and t.ny - (t.tile_row_end if t.lds_class >= 0 else 0) >= 8]
        assert wide, [(t.nx, t.ny, t.tile_row_end) for t in tiles]


@gpu
def test_band_major_pass_sweeps_a_full_queue_first(env, oracle):
    c, _, frames = fill_case()
    want = fill_oracle(oracle)
    base = None
    for waves in (4, 8):
        for extra in ((), ALL_GATHER, (("q_group_units", 8),), (("q_group_units", 16),)):
            label = f"fill gather_waves={waves} {dict(extra)}"
            with tunables(env, ("gather_waves", waves), ("pass_split", "3"), *extra):
                r = check(env, c, frames, want, label)
            assert [p[:2] for p in r.passes] == [(0, 3), (3, 4)], f"{label}: {r.passes}"
            grid = [l for l in r.launches if l["kind"] == "grid"]
            queue = [l for l in r.launches if l["kind"] == "queue"]
            assert len(grid) == 1 and len(queue) >= 1, f"{label}: {[l['kind'] for l in r.launches]}"
            # every window the grid pass enumerates reaches the queue pass that follows it: a group of two or more full units holds
            # more than FILL_CAP
            assert grid[0]["stage_entered"][0] == grid[0]["stage_entered"][2] > 2 * FILL_CAP * len(frames), label
            assert queue[0]["stage_entered"][3] >= grid[0]["stage_entered"][0], label
            if extra == ALL_GATHER:
                assert not any(l["kind"] == "tile" for l in r.launches) and len(queue) == 1, label
                assert queue[0]["stage_entered"][3] == grid[0]["stage_entered"][0] == r.windows, label
            if base is None:
                base = r
            assert np.array_equal(r.rects, base.rects) and r.stage_entered == base.stage_entered, label
