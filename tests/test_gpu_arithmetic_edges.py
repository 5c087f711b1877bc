"""Stage sums, variances and window sums where float rounding decides, on every path, against the C oracle frame by frame.

Several kernels add a stage's leaf values in another order than the reference's running sum — a DPP butterfly per block of
up to 64 stumps (tile_wave_tail), K even ranges (tile_wave_split, stumps and two-node trees), the stump-parallel tails of the
gather chain, the f64 forms of the OpenCV profile — and trust that sum only when it clears the stage threshold by more than
sp_delta; otherwise they replay the verdict bits in stump order.  The cells of cases.ORDER_CELLS put EVERY window inside that
band and make each of those orders change at least 50 verdicts (tests/test_arithmetic_cases_cpu.py proves it on the CPU), so
a replay that walks the wrong bits, a range that starts from the wrong stump, a band that is too narrow or a > for >= gives
other rectangles and counts than the oracle.  cases.TIE_CELLS put sums exactly ON the threshold (and the threshold one float
above them) with every other window decided by the fast path.  near_flat_frames() make Q / area - mean * mean cancel to a small
negative, zero or positive value; bright_frame() takes window sums past 2^31, where VJ_FLAG_SIGNED_MEAN changes the result.

Which finish a tile took (wave-split with K = 2, 4 or 8, the wave-independent tail, the dense sweep) is not visible in a
result; what is visible — the launch kinds and the stages each launch entered — is asserted, and tile_ws_min / tile_ws_max /
tile_sp_begin are set to each side of the windows a tile holds after the thinning stage (1 in 16 of up to 2048).  With the
decisive stage at index 3, tile_sp_begin 5 and 64 are one setting: the finish is never taken and the dense sweep decides.
That K = 2, 4 and 8 all occur rests on the spread of tile populations over scales and frame edges (about 128 windows in a
full tile, fewer in the partial ones); mutants of the replays (the comparison, the band, the order inside a block), each
built once outside the tree, are what showed that the windows reach them."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cases import (ARITH_FRAMES, BRIGHT_CASCADES, BRIGHT_MIN, NEAR_FLAT_CELLS, ORDER_CELLS, ORDER_PREFIX, TIE_CELLS, arith_frames,
                   bright_frame, cascade_to_product, check_against_oracle, geometry_cascade, near_flat_frames, order_cascade, rows_of,
                   tie_cascade, tunables)
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_SIGNED_MEAN, Environment, default_params
from test_gpu_feature_geometry import CV_SETTINGS

pytestmark = pytest.mark.gpu

# (id, builder arguments, frame size, first frame seed, decisive stages, two-node trees)
CELLS = [(cid, ("order", form, n, cs), size, fs, [ORDER_PREFIX] + ([ORDER_PREFIX + 1] if form == "two_stage" else []), form == "trees")
         for cid, form, n, cs, size, fs in ORDER_CELLS] + \
        [(cid, ("tie", strict, cs), size, fs, [ORDER_PREFIX], False) for cid, strict, cs, size, fs in TIE_CELLS]
CELL_IDS = [c[0] for c in CELLS]
BATCHES = (1, ARITH_FRAMES)
GATHER_ONLY = ("tile_max_dwords_per_window", 0)
TILE_SETTINGS = [(("tile_ws_min", 0),), (("tile_ws_min", 1),), (("tile_ws_min", 9),), (("tile_ws_min", 256),),   # all wave-split .. all tail
                 (("tile_ws_max", 0),), (("tile_sp_begin", 5),), (("tile_sp_begin", 64),)]
GATHER_SETTINGS = [(k, v) for k, vals in (("sp_tail_max", (0, 16)), ("wide_tail", (0, 1)), ("gather_pairs", (0, 1, 2)), ("gather_waves", (1, 4)))
                   for v in vals]
HANDOFFS = ((("pass_split", "1"), ("tile_end", 1), ("tile_min_lanes", 0), ("tile_sp_begin", 64)),
            (("pass_split", "1"), ("tile_end", 64), ("tile_min_lanes", 64)),
            (("pass_split", "1"), ("tile_end", 1), ("tile_min_lanes", 0), ("q_band_px", 0)))
_CASC, _ORACLE = {}, {}
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module", autouse=True)
def report_oracle_share():
    """Prints the module's wall time and the seconds of it spent inside the oracle (shown with -s)."""
    t = time.perf_counter()
    yield
    print(f"\ntest_gpu_arithmetic_edges: {time.perf_counter() - t:.1f} s, of which {ORACLE_SECONDS[0]:.1f} s in the oracle")


def cascade(spec):
    """(oracle CascadeArrays, product Cascade)."""
    if spec not in _CASC:
        a = order_cascade(*spec[1:]) if spec[0] == "order" else tie_cascade(*spec[1:])
        _CASC[spec] = (a, cascade_to_product(a))
    return _CASC[spec]


def oracle_of(oracle, key, a, frames, profile, **kw):
    """[(rects, stats)] of the oracle per frame, computed once per module and timed."""
    key = (key, profile, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        fn = oracle.detect if profile == "clod" else oracle.detect_opencvlike
        t = time.perf_counter()
        with ThreadPoolExecutor(8) as ex:
            _ORACLE[key] = list(ex.map(lambda f: fn(a, f, **kw), frames))
        ORACLE_SECONDS[0] += time.perf_counter() - t
    return _ORACLE[key]


def check_cv(env, c, frames, want, label):
    """A counted and an uncounted vj_detect_opencv against the oracle's per-frame results."""
    r = env.detect_opencv(c, frames, flags=VJ_FLAG_COUNTERS)
    entered, windows = [0] * c.info.n_stages, 0
    for i, (ro, st) in enumerate(want):
        mine = sorted(rows_of(r.rects[r.rects["frame"] == i]))
        assert mine == sorted(rows_of(ro)), f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: stages entered {r.stage_entered}, the oracle {entered}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"
    r2 = env.detect_opencv(c, frames)
    assert np.array_equal(r2.rects, r.rects), f"{label}: the uncounted call's rectangles differ from the counted ones"
    return r


def entered_by(r, kind, stage):
    return sum(l["stage_entered"][stage] for l in r.launches if l["kind"] == kind)


def kinds_of(r):
    return sorted({l["kind"] for l in r.launches})


# ------------------------------------------------------------------------------------------------ clod profile
@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_clod_paths_match_the_oracle(env, oracle, cell):
    cid, spec, size, fseed, stages, trees = cell
    a, c = cascade(spec)
    frames = arith_frames(size, fseed)
    want = oracle_of(oracle, cid, a, frames, "clod")
    for n in BATCHES:
        fr, w = frames[:n], want[:n]
        label = f"{cid} n={n}"
        r, entered = check_against_oracle(env, c, fr, w, f"{label} default")
        assert all(entered[s] > 0 for s in stages), f"{label}: a decisive stage is never entered: {entered}"
        # the tiles run the decisive stages themselves (tile_end 64, tile_min_lanes 0): that is where the finishes are
        assert "tile" in kinds_of(r) and all(entered_by(r, "tile", s) > 0 for s in stages), f"{label}: {kinds_of(r)}"
        for settings in TILE_SETTINGS:
            with tunables(env, *settings):
                r, _ = check_against_oracle(env, c, fr, w, f"{label} {settings}")
                assert all(entered_by(r, "tile", s) > 0 for s in stages), f"{label} {settings}: the tiles left before the decisive stage"
        with tunables(env, GATHER_ONLY):
            r, _ = check_against_oracle(env, c, fr, w, f"{label} gather chain")
            assert "tile" not in kinds_of(r), kinds_of(r)
        for setting in GATHER_SETTINGS:
            with tunables(env, GATHER_ONLY, setting):
                r, _ = check_against_oracle(env, c, fr, w, f"{label} gather chain {setting}")
                assert "tile" not in kinds_of(r), kinds_of(r)
            with tunables(env, setting):
                check_against_oracle(env, c, fr, w, f"{label} {setting}")
        for settings in HANDOFFS:
            with tunables(env, *settings):
                r, _ = check_against_oracle(env, c, fr, w, f"{label} {settings}")
                assert "tile" in kinds_of(r), f"{label} {settings}: {kinds_of(r)}"
                if settings[1] == ("tile_end", 1):   # the queue pass decides the decisive stages
                    assert "queue" in kinds_of(r) and all(entered_by(r, "tile", s) == 0 and entered_by(r, "queue", s) > 0 for s in stages), f"{label} {settings}"


def test_clod_tile_groups(monkeypatch, oracle):
    """VJ_TILE_GROUP 1 and 4 in a fresh environment: step-2 scales alone on their tiles, or four of them sharing one."""
    for g in (1, 4):
        monkeypatch.setenv("VJ_TILE_GROUP", str(g))
        e = Environment(0)
        try:
            for cid, spec, size, fseed, stages, trees in CELLS:
                a, c = cascade(spec)
                frames = arith_frames(size, fseed)
                want = oracle_of(oracle, cid, a, frames, "clod")
                for n in BATCHES:
                    r, _ = check_against_oracle(e, c, frames[:n], want[:n], f"{cid} n={n} VJ_TILE_GROUP={g}")
                    assert all(entered_by(r, "tile", s) > 0 for s in stages)
        finally:
            e.close()
    monkeypatch.delenv("VJ_TILE_GROUP")


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_regions_match_the_oracle(env, oracle, cell):
    """vj_detect_rois on large regions, on LDS tiles (roi_tiles 512, the default) and without (0), against the oracle on
    each sub-image."""
    cid, spec, size, fseed, stages, trees = cell
    a, c = cascade(spec)
    frames = arith_frames(size, fseed, 3)
    h, w = size
    rois = [(0, 0, 0, w, h), (1, 0, 0, w, h), (2, w // 5, h // 6, 3 * w // 4, 3 * h // 4), (0, 1, 3, w - 1, h - 3), (1, w // 3, 0, 2 * w // 3, h)]
    t = time.perf_counter()
    want = [oracle.detect(a, np.ascontiguousarray(frames[f][y:y + rh, x:x + rw])) for f, x, y, rw, rh in rois]
    ORACLE_SECONDS[0] += time.perf_counter() - t
    entered = [sum(st["stage_entered"][s] for _, st in want) for s in range(a.n_stages)]
    for value in (512, 0):
        with tunables(env, ("roi_tiles", value)):
            r = env.detect_rois(c, frames, rois, default_params(flags=VJ_FLAG_COUNTERS))
            r2 = env.detect_rois(c, frames, rois)
        for i, (ro, _) in enumerate(want):
            assert rows_of(r.rects[r.rects["frame"] == i]) == rows_of(ro), f"{cid} roi_tiles {value} region {rois[i]}"
        assert r.stage_entered == entered, f"{cid} roi_tiles {value}: stages entered {r.stage_entered}, the oracle {entered}"
        assert np.array_equal(r2.rects, r.rects), f"{cid} roi_tiles {value}: the uncounted call differs"


# ------------------------------------------------------------------------------------------------ OpenCV profile
TILES = (("cv_tile_min_windows0", 64), ("cv_tile_min_windows", 64))
CV_EXTRA = [(("cv_tail_max", 0),), (("cv_tail_max", 20),), TILES + (("cv_tail_max", 0),), TILES + (("cv_tail_max", 20),)]


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_opencv_paths_match_the_oracle(env, oracle, cell):
    cid, spec, size, fseed, stages, trees = cell
    a, c = cascade(spec)
    frames = arith_frames(size, fseed)
    want = oracle_of(oracle, cid, a, frames, "cv")
    settings = CV_SETTINGS + CV_EXTRA + ([(("cv_tree2", 0),), TILES + (("cv_tree2", 0),)] if trees else [])
    for n in BATCHES:
        for s in settings:
            with tunables(env, *s):
                r = check_cv(env, c, frames[:n], want[:n], f"cv {cid} n={n} {s}")
        assert all(r.stage_entered[s] > 0 for s in stages)


# ------------------------------------------------------------------------------------------------ nearly flat windows
@pytest.mark.parametrize("cell", NEAR_FLAT_CELLS, ids=[c[0] for c in NEAR_FLAT_CELLS])
def test_near_flat_frames(env, oracle, cascades, cell):
    """Tile kernel from LDS, grid kernel (gather chain only), region pass and the OpenCV profile's f64 on frames whose
    variance expression cancels to a small negative, zero or positive value."""
    cid, name, size, n_off = cell
    if isinstance(name, tuple):
        a = geometry_cascade(name[1][0], name[1][1], name[2])
        c = cascade_to_product(a)
    else:
        c, a = cascades(name)
    frames = near_flat_frames(size, n_off)
    want = oracle_of(oracle, "flat_" + cid, a, frames, "clod")
    for n in (1, len(frames)):
        check_against_oracle(env, c, frames[:n], want[:n], f"near flat {cid} n={n} default")
        with tunables(env, GATHER_ONLY):
            r, _ = check_against_oracle(env, c, frames[:n], want[:n], f"near flat {cid} n={n} gather chain")
            assert "tile" not in kinds_of(r)
    want_cv = oracle_of(oracle, "flat_" + cid, a, frames, "cv")
    for s in ((), TILES, (("cv_tiles", 0),)):
        with tunables(env, *s):
            check_cv(env, c, frames, want_cv, f"near flat {cid} cv {s}")
    rois = [(i, 0, 0, size[1], size[0]) for i in range(len(frames))] + [(0, 7, 5, size[1] - 20, size[0] - 9)]
    want_r = [want[f] if i < len(frames) else oracle.detect(a, np.ascontiguousarray(frames[f][y:y + rh, x:x + rw]))
              for i, (f, x, y, rw, rh) in enumerate(rois)]
    # (no window of these frames is a detection of the shipped cascades: what a wrong norm factor moves is the per-stage counts)
    entered = [sum(st["stage_entered"][s] for _, st in want_r) for s in range(a.n_stages)]
    assert sum(entered[1:]) > 0
    for value in (512, 0):
        with tunables(env, ("roi_tiles", value)):
            r = env.detect_rois(c, frames, rois, default_params(flags=VJ_FLAG_COUNTERS))
            r2 = env.detect_rois(c, frames, rois)
        for i, (ro, _) in enumerate(want_r):
            assert rows_of(r.rects[r.rects["frame"] == i]) == rows_of(ro), f"near flat {cid} roi_tiles {value} region {rois[i]}"
        assert r.stage_entered == entered, f"near flat {cid} roi_tiles {value}: stages entered {r.stage_entered}, the oracle {entered}"
        assert np.array_equal(r2.rects, r.rects), f"near flat {cid} roi_tiles {value}: the uncounted call differs"


# ------------------------------------------------------------------------------------------------ sums past 2^31
@pytest.mark.parametrize("name", BRIGHT_CASCADES)
def test_bright_frame_with_and_without_signed_mean(env, oracle, cascades, name):
    """The five largest scales of a 4608 x 4608 frame of 230..255: the sum integral wraps 2^32 and the windows hold more than
    2^31.  With and without VJ_FLAG_SIGNED_MEAN the oracle's rectangles and counts, which differ from each other; the OpenCV
    profile (whose mean is always the signed one) on the same frame."""
    c, a = cascades(name)
    img = bright_frame(1)
    size = (BRIGHT_MIN, BRIGHT_MIN)
    got = {}
    for signed in (False, True):
        (ro, st), = oracle_of(oracle, "bright_" + name, a, [img], "clod", min_size=size, signed_mean=signed)
        for extra in ((), (GATHER_ONLY,)):
            with tunables(env, *extra):
                flags = VJ_FLAG_SIGNED_MEAN if signed else 0
                r = env.detect(c, img, default_params(flags=flags | VJ_FLAG_COUNTERS, min_w=size[0], min_h=size[1]))
                label = f"bright {name} signed_mean={signed} {extra}"
                assert rows_of(r.rects) == rows_of(ro), f"{label}: {len(r.rects)} rectangles, the oracle {len(ro)}"
                assert r.stage_entered == st["stage_entered"], f"{label}: {r.stage_entered}, the oracle {st['stage_entered']}"
                assert r.windows == st["windows"], label
                r2 = env.detect(c, img, default_params(flags=flags, min_w=size[0], min_h=size[1]))
                assert np.array_equal(r2.rects, r.rects), label
        got[signed] = (rows_of(r.rects), r.stage_entered)
    assert got[False] != got[True], "VJ_FLAG_SIGNED_MEAN changed nothing"
    want = oracle_of(oracle, "bright_" + name, a, [img], "cv", min_size=size)
    r = env.detect_opencv(c, img, min_size=size, flags=VJ_FLAG_COUNTERS)
    assert sorted(rows_of(r.rects)) == sorted(rows_of(want[0][0])) and r.stage_entered == want[0][1]["stage_entered"]
    assert r.windows == want[0][1]["windows"]
