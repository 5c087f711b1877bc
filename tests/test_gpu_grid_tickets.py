"""The grid pass hands its (frame, unit) list out by ticket (cascade_pass<FROM_GRID>, csrc/vj_grid_parts.hpp):
eight contiguous parts with a counter each, a wave draws one unit per ticket and steals from the next part when its own is
used up.  Every unit must be processed exactly once whatever the grid: per frame the rectangles are the oracle's, and with
VJ_FLAG_COUNTERS the windows entering every stage are the oracle's too — that is what catches a unit without a detection that
was processed twice or never.  Frame counts that leave parts empty (1, 3), fill them evenly (8) and unevenly (9); one and
eight workgroups per CU, one and four waves per workgroup, the chains overlapped and in series; every scale a gather scale
(many units per frame) and the default split; a linear cascade, one of two-node trees (TREES) and a stage tree (GENERAL
prefix + chains); the grid pass as the only pass (LAST); tickets re-zeroed between calls, per sub-batch and per stream lane."""
import pytest

from cases import tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, default_params, synth

pytestmark = pytest.mark.gpu

VJ_LAUNCH_GRID, VJ_LAUNCH_TILE = "grid", "tile"          # DetectResult.launches names the kinds (api.LAUNCH_KINDS)
KINDS = ("noise", "faces", "blocks", "smooth")
SIZES = ((240, 320), (480, 640))
CASCADES = ("frontalface_alt", "frontalface_alt2", "frontalface_alt_tree")
N_FRAMES = (1, 3, 8, 9)
_FRAMES, _WANT = {}, {}
# every scale on the gather chain, many units per frame: a class is searched up to tile_min_windows windows per tile and a scale
# whose best tile holds fewer than tile_accept_windows stays off the tiles — no tile holds 65536
ALL_GATHER = [("tile_min_windows", 65536), ("tile_accept_windows", 65536)]


def frames_of(h, w, n, seed0=4100):
    """n distinct frames of a size (frame i is the same in every batch of that size)."""
    if (h, w, seed0) not in _FRAMES:
        _FRAMES[(h, w, seed0)] = synth.batch(max(N_FRAMES), h, w, seed0=seed0, kinds=KINDS)
    return _FRAMES[(h, w, seed0)][:n]


def oracle_of(oracle, cascades, casc, h, w, i, seed0=4100):
    """(rectangles, stage_entered) of frame i, computed once."""
    key = (casc, h, w, i, seed0)
    if key not in _WANT:
        ro, st = oracle.detect(cascades(casc)[1], frames_of(h, w, i + 1, seed0)[i])
        _WANT[key] = (rows(ro), list(st["stage_entered"]))
    return _WANT[key]


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


def check(r, oracle, cascades, casc, h, w, n, label, counted, seed0=4100, first=0):
    entered = None
    for f in range(n):
        want, st = oracle_of(oracle, cascades, casc, h, w, first + f, seed0)
        assert rows(r.rects[r.rects["frame"] == f]) == want, f"{label}: frame {f}"
        entered = st if entered is None else [a + b for a, b in zip(entered, st)]
    assert len(r.rects) == sum(len(oracle_of(oracle, cascades, casc, h, w, first + f, seed0)[0]) for f in range(n)), label
    if counted:
        assert r.stage_entered == entered, f"{label}: windows entering each stage"


def both(env, c, frames):
    """the timed kernels, then the counting ones"""
    return env.detect(c, frames), env.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS))


@pytest.mark.parametrize("n", N_FRAMES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("casc", CASCADES)
def test_every_unit_once_whatever_the_grid(env, oracle, cascades, casc, size, n):
    h, w = size
    c, _ = cascades(casc)
    frames = frames_of(h, w, n)
    for tile_min_windows in (None, 65536):          # 65536 (ALL_GATHER): no tile holds that many windows, so every scale is a gather scale
        for per_cu in (1, 8):
            for waves in (1, 4):
                for concurrent in (0, 1):
                    settings = [("blocks_per_cu", per_cu), ("concurrent_blocks_per_cu", per_cu), ("gather_waves", waves),
                                ("concurrent", concurrent)]
                    if tile_min_windows is not None:
                        settings += ALL_GATHER
                    if per_cu == 8:   # (taken for linear stump cascades of large frames only, refused here: see the last test)
                        settings.append(("one_pass_max_frames", n))
                    label = f"{casc} {w}x{h} n={n} " + " ".join(f"{k}={v}" for k, v in settings)
                    with tunables(env, *settings):
                        timed, counted = both(env, c, frames)
                    if tile_min_windows is not None:   # (at the default a small frame may leave the gather chain nothing)
                        assert any(l["kind"] == VJ_LAUNCH_GRID for l in counted.launches), label
                        assert all(l["kind"] != VJ_LAUNCH_TILE for l in counted.launches), f"{label}: a tile launch"
                    check(timed, oracle, cascades, casc, h, w, n, label + " timed", False)
                    check(counted, oracle, cascades, casc, h, w, n, label + " counted", True)


@pytest.mark.parametrize("casc", CASCADES)
def test_tickets_are_zeroed_again_for_the_next_call(env, oracle, cascades, casc):
    """Two calls in a row on one environment — with different frame counts, so that a ticket left over from the first call
    would hand out a unit of a frame the second does not have, or skip one it has."""
    h, w = SIZES[0]
    c, _ = cascades(casc)
    with tunables(env, *ALL_GATHER):
        for n in (9, 3, 3, 8):
            timed, counted = both(env, c, frames_of(h, w, n))
            check(timed, oracle, cascades, casc, h, w, n, f"{casc} n={n} timed", False)
            check(counted, oracle, cascades, casc, h, w, n, f"{casc} n={n} counted", True)


@pytest.mark.parametrize("casc", CASCADES)
def test_sub_batches_draw_from_zeroed_tickets(env, oracle, cascades, casc):
    """max_subbatch 2 with 5 frames: three cascade runs behind one call, each with a grid launch of its own."""
    h, w = SIZES[0]
    c, _ = cascades(casc)
    for thresholds in ([], ALL_GATHER):
        with tunables(env, ("max_subbatch", 2), *thresholds):
            timed, counted = both(env, c, frames_of(h, w, 5))
        check(timed, oracle, cascades, casc, h, w, 5, f"{casc} sub-batches timed", False)
        check(counted, oracle, cascades, casc, h, w, 5, f"{casc} sub-batches counted", True)


@pytest.mark.parametrize("casc", CASCADES)
def test_stream_lanes_have_their_own_tickets(env, oracle, cascades, casc):
    """A vj_stream with two different batches in flight: each lane's grid pass draws from the counters of its own block."""
    h, w = SIZES[0]
    c, _ = cascades(casc)
    a, b = frames_of(h, w, 8), frames_of(h, w, 3, seed0=4300)
    for flags, counted in ((0, False), (VJ_FLAG_COUNTERS, True)):
        with tunables(env, *ALL_GATHER):
            st = env.stream(c, w, h, 8, default_params(flags=flags))
            try:
                st.submit(a)
                st.submit(b)
                ra, rb = st.collect(), st.collect()
                st.submit(b)
                st.submit(a)
                rb2, ra2 = st.collect(), st.collect()
            finally:
                st.close()
        for r, n, seed0, name in ((ra, 8, 4100, "first"), (rb, 3, 4300, "second"), (rb2, 3, 4300, "third"), (ra2, 8, 4100, "fourth")):
            check(r, oracle, cascades, casc, h, w, n, f"{casc} stream, {name} batch", counted, seed0)


def test_grid_pass_as_the_only_pass(env, oracle, cascades):
    """one_pass_max_frames >= the frame count on frames of more than 800000 pixels (smaller ones keep their passes): the grid
    pass runs the whole cascade, so the ticketed loop feeds the detection list directly (LAST)."""
    h, w = 768, 1056
    casc = "frontalface_alt"
    c, _ = cascades(casc)
    frames = frames_of(h, w, 2, seed0=4500)
    for per_cu, waves in ((1, 4), (8, 1)):
        with tunables(env, ("one_pass_max_frames", 2), ("blocks_per_cu", per_cu), ("concurrent_blocks_per_cu", per_cu), ("gather_waves", waves)):
            timed, counted = both(env, c, frames)
        grid = [l for l in counted.launches if l["kind"] == VJ_LAUNCH_GRID]
        assert len(grid) == 1 and grid[0]["stage_begin"] == 0 and grid[0]["stage_end"] == c.info.n_stages, counted.launches
        check(timed, oracle, cascades, casc, h, w, 2, "one pass timed", False, 4500)
        check(counted, oracle, cascades, casc, h, w, 2, "one pass counted", True, 4500)
