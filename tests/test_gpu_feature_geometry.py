"""Feature rectangles on the edges of the window (tests/cases.py, geometry_cascade): flush with each border and corner, the
full window, 1-pixel strips, w = 0 / h = 0, two and three rectangles, negative weights, tilted rectangles on each of the
four tilted bounds, the smallest tilted one, two-node trees mixing upright and tilted nodes; windows 20x20, 24x24, 45x11,
14x28 and 7x5.  The tile footprints (reach_x / reach_y, the re-based corner offsets, the tilted image behind the sum image)
are what such features test: every path of both profiles is forced in turn and gives the oracle's rectangles and counters.

The frames are sized so that at a scale where a rounded rectangle overhangs its rounded window by one pixel, the last
window column and row end one pixel before the frame's edge: the overhanging read is the frame's last integral column and
row.  Both facts, and that every stage is entered on every frame, are asserted, so that no test passes vacuously."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from cases import GEOMETRY_KINDS, GEOMETRY_WINDOWS, cascade_to_product, geometry_cascade, overhangs, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_TILTED_AS_UPRIGHT, Environment, default_params, synth

pytestmark = pytest.mark.gpu

# (height, width) per window: at one scale of each profile the last window column / row ends one pixel before the edge
# while a feature overhangs the window by one pixel there (test_frame_sizes_put_the_overhang_on_the_edge)
EDGE_SIZES = {(20, 20): (94, 93), (24, 24): (118, 110), (45, 11): (58, 195), (14, 28): (128, 70), (7, 5): (44, 42)}
N_FRAMES = 8                                     # q_band_min_frames: the band-major queue pass takes batches of 8 or more
KINDS = ("noise", "blocks", "smooth")
WIN_IDS = [f"{w}x{h}" for w, h in GEOMETRY_WINDOWS]
CELLS = [pytest.param(win, kind, id=f"{win[0]}x{win[1]}-{kind}") for win in GEOMETRY_WINDOWS for kind in GEOMETRY_KINDS]

_CASC, _FRAMES, _ORACLE = {}, {}, {}


def cascade(win, kind):
    """(oracle CascadeArrays, product Cascade)."""
    if (win, kind) not in _CASC:
        a = geometry_cascade(win[0], win[1], kind)
        _CASC[(win, kind)] = (a, cascade_to_product(a))
    return _CASC[(win, kind)]


def frames(win, size=None, n=N_FRAMES):
    h, w = size or EDGE_SIZES[win]
    key = (h, w, n)
    if key not in _FRAMES:
        _FRAMES[key] = synth.batch(n, h, w, seed0=7000 + h * 3 + w, kinds=KINDS)
    return _FRAMES[key]


def clod_flags(kind, counters=True):
    """The clod profile reads tilted rectangles as upright ones only when asked to (the reference's reading)."""
    return (VJ_FLAG_COUNTERS if counters else 0) | (VJ_FLAG_TILTED_AS_UPRIGHT if kind != "upright" else 0)


def rows(rects):
    return [tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects]


def oracle_of(oracle, win, kind, fr, profile):
    """[(rects, stats)] of the oracle for every frame of `fr` (computed once per module); asserts that every stage of the
    cascade is entered on every frame."""
    key = (win, kind, fr.shape, fr.ctypes.data, profile)
    if key not in _ORACLE:
        a, _ = cascade(win, kind)
        fn = oracle.detect if profile == "clod" else oracle.detect_opencvlike
        with ThreadPoolExecutor(8) as ex:
            res = list(ex.map(lambda i: fn(a, fr[i]), range(len(fr))))
        for i, (_, st) in enumerate(res):
            assert all(v > 0 for v in st["stage_entered"]), \
                f"{profile} {win} {kind} frame {i} {fr.shape[1:]}: a stage is never entered: {st['stage_entered']}"
        _ORACLE[key] = res
    return _ORACLE[key]


def compare(r, want, n_stages, label, sort=False):
    entered, windows = [0] * n_stages, 0
    for i, (ro, st) in enumerate(want):
        mine, theirs = rows(r.rects[r.rects["frame"] == i]), rows(ro)
        if sort:
            mine, theirs = sorted(mine), sorted(theirs)
        assert mine == theirs, f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(theirs)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: stages entered {r.stage_entered}, the oracle {entered}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"


def launch_kinds(r):
    return sorted({l["kind"] for l in r.launches})


def check_clod(env, oracle, win, kind, fr, label):
    """A counted and a timed vj_detect of `fr` against the oracle; returns the counted result."""
    a, c = cascade(win, kind)
    r = env.detect(c, fr, default_params(flags=clod_flags(kind)))
    compare(r, oracle_of(oracle, win, kind, fr, "clod"), c.info.n_stages, label)
    r2 = env.detect(c, fr, default_params(flags=clod_flags(kind, counters=False)))
    assert np.array_equal(r2.rects, r.rects), f"{label}: the timed kernels' rectangles differ from the counted ones"
    return r


def check_cv(env, oracle, win, kind, fr, label):
    a, c = cascade(win, kind)
    r = env.detect_opencv(c, fr, flags=VJ_FLAG_COUNTERS)
    compare(r, oracle_of(oracle, win, kind, fr, "cv"), c.info.n_stages, label, sort=True)
    r2 = env.detect_opencv(c, fr)
    assert np.array_equal(r2.rects, r.rects), f"{label}: the uncounted call's rectangles differ from the counted ones"
    return r


# ------------------------------------------------------------------------------------------------ the premises
def _cv_round(v):
    return int(np.rint(v))


@pytest.mark.parametrize("win,kind", CELLS)
def test_frame_sizes_put_the_overhang_on_the_edge(win, kind):
    """At the edge sizes, for x and for y, some scale of each profile has (a) a weighted rectangle whose rounded far edge
    passes the rounded window by one pixel — round(x s) + round(w s) == round(win s) + 1, in the clod plan's f32 rounding
    and in the OpenCV profile's cvRound of f64 products — and (b) a last window that ends one pixel before the frame's edge."""
    a, c = cascade(win, kind)
    h, w = EDGE_SIZES[win]
    scales = [s for s in c.plan_scales(w, h) if s.accepted and s.nx > 0 and s.ny > 0]
    ov = overhangs(a, scales)
    assert ov["x"] and ov["y"], f"no one-pixel overhang in the clod plan: {ov}"
    last = lambda n, step: int(np.rint(np.float64(np.float32(n - 1) * np.float32(step))))   # lrint of the f32 product
    assert any(last(s.nx, s.step) + s.win_w == w - 1 for s in scales if s.scale_idx in {k for k, _, _ in ov["x"]})
    assert any(last(s.ny, s.step) + s.win_h == h - 1 for s in scales if s.scale_idx in {k for k, _, _ in ov["y"]})
    # OpenCV profile (cvHaarDetectObjects' loop, as the oracle restates it)
    r, wt = a.node_rect.reshape(-1, 3, 4), a.node_weight.reshape(-1, 3)
    used = [(n, q) for n in range(a.n_nodes) for q in range(3) if wt[n, q] != 0]
    hit_x = hit_y = False
    factor, n_f = 1.0, 0
    while factor * a.win_w < w - 10 and factor * a.win_h < h - 10:
        n_f, factor = n_f + 1, factor * 1.1
    factor = 1.0
    for _ in range(n_f):
        ys = max(2.0, factor)
        ww, wh = _cv_round(a.win_w * factor), _cv_round(a.win_h * factor)
        end_x, end_y = _cv_round((w - ww) / ys), _cv_round((h - wh) / ys)
        ox = any(_cv_round(r[n, q, 0] * factor) + _cv_round(r[n, q, 2] * factor) == ww + 1 for n, q in used)
        oy = any(_cv_round(r[n, q, 1] * factor) + _cv_round(r[n, q, 3] * factor) == wh + 1 for n, q in used)
        hit_x |= ox and end_x > 0 and _cv_round((end_x - 1) * ys) + ww == w - 1
        hit_y |= oy and end_y > 0 and _cv_round((end_y - 1) * ys) + wh == h - 1
        factor *= 1.1
    assert hit_x and hit_y, (hit_x, hit_y)


# ------------------------------------------------------------------------------------------------ clod profile
@pytest.mark.parametrize("win,kind", CELLS)
def test_clod_paths_match_the_oracle(env, oracle, win, kind):
    """vj_detect on eight distinct edge-size frames: the default plan, every scale on the global-gather chain
    (tile_max_dwords_per_window 0: no tile), and tiles that hand their windows to the queue pass at stage 1 — band-major
    for eight frames — or when fewer than tile_min_lanes windows are left."""
    fr = frames(win)
    label = f"clod {win[0]}x{win[1]} {kind} {fr.shape[1]}x{fr.shape[2]}"
    r = check_clod(env, oracle, win, kind, fr, f"{label} default")
    assert "tile" in launch_kinds(r), f"{label}: the default plan staged no tile: {launch_kinds(r)}"
    with tunables(env, ("tile_max_dwords_per_window", 0)):
        r = check_clod(env, oracle, win, kind, fr, f"{label} gather chain")
        assert "tile" not in launch_kinds(r), launch_kinds(r)
    for settings in ((("pass_split", "1"), ("tile_end", 1), ("tile_min_lanes", 0), ("tile_sp_begin", 64)),
                     (("pass_split", "1"), ("tile_end", 64), ("tile_min_lanes", 64)),
                     (("pass_split", "1"), ("tile_end", 1), ("tile_min_lanes", 0), ("q_band_px", 0))):
        with tunables(env, *settings):
            r = check_clod(env, oracle, win, kind, fr, f"{label} {settings}")
            kinds = launch_kinds(r)
            assert "tile" in kinds and "queue" in kinds, f"{label} {settings}: {kinds}"
            if settings[1] == ("tile_end", 1):
                tiles = [l for l in r.launches if l["kind"] == "tile"]
                assert not any(l["stage_entered"][1] for l in tiles), f"{label} {settings}: the tiles entered stage 1"
    # odd sizes: one frame each, the window count no multiple of anything
    check_clod(env, oracle, win, kind, frames(win, (EDGE_SIZES[win][0] + 37, EDGE_SIZES[win][1] + 52), n=2),
               f"{label} odd size")


@pytest.mark.parametrize("win", GEOMETRY_WINDOWS, ids=WIN_IDS)
def test_clod_tile_groups(monkeypatch, oracle, win):
    """VJ_TILE_GROUP 1 and 4 (step-2 scales sharing one staged tile, the group's pitch the largest member's): the oracle's
    rectangles and counters for every kind."""
    fr = frames(win)
    for g in (1, 4):
        monkeypatch.setenv("VJ_TILE_GROUP", str(g))
        e = Environment(0)
        try:
            for kind in GEOMETRY_KINDS:
                r = check_clod(e, oracle, win, kind, fr, f"clod {win} {kind} VJ_TILE_GROUP={g}")
                assert "tile" in launch_kinds(r)
        finally:
            e.close()
    monkeypatch.delenv("VJ_TILE_GROUP")


@pytest.mark.parametrize("win", [(20, 20), (7, 5), (45, 11)], ids=["20x20", "7x5", "45x11"])
def test_clod_regions_on_the_frame_edges(env, oracle, win):
    """vj_detect_rois with regions flush with each edge of the frame and one that is the whole frame, against the oracle
    on each sub-image."""
    fr = frames(win)
    h, w = fr.shape[1:]
    rh, rw = 2 * h // 3 + 1, 2 * w // 3 + 1
    rois = [(0, 0, 0, w, h), (1, w - rw, h - rh, rw, rh), (2, 0, h - rh, rw, rh), (3, w - rw, 0, rw, rh), (4, 0, 0, rw, rh),
            (7, w - rw, 3, rw, h - 3)]
    for kind in GEOMETRY_KINDS:
        a, c = cascade(win, kind)
        for setting in (None, ("roi_tiles", 0)):
            with tunables(env, *([setting] if setting else [])):
                r = env.detect_rois(c, fr, rois, default_params(flags=clod_flags(kind)))
            for i, (f, x, y, rw_, rh_) in enumerate(rois):
                ro, st = oracle.detect(a, np.ascontiguousarray(fr[f][y:y + rh_, x:x + rw_]))
                assert rows(r.rects[r.rects["frame"] == i]) == rows(ro), f"{win} {kind} {setting} roi {rois[i]}"


def test_clod_chain(env, oracle):
    """vj_detect_chain: the 24x24 upright geometry cascade's raw candidates as the regions of each 7x5 and 20x20 cascade;
    equal to vj_detect + vj_detect_rois, and to the oracle on sub-images."""
    first_a, first = cascade((24, 24), "upright")
    fr = frames((24, 24))
    for win in ((7, 5), (20, 20)):
        for kind in GEOMETRY_KINDS:
            a, c = cascade(win, kind)
            p2 = default_params(flags=clod_flags(kind))
            r1, r2 = env.detect_chain(first, c, fr, default_params(), p2)
            assert len(r1.rects) > 0
            rois = [(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects]
            host = env.detect_rois(c, fr, rois, p2)
            key = lambda rr: sorted(tuple(int(r[k]) for k in ("frame", "scale_idx", "y", "x", "w", "h")) for r in rr)
            assert key(r2.rects) == key(host.rects), f"{win} {kind}"
            assert r2.stage_entered == host.stage_entered and r2.windows == host.windows, f"{win} {kind}"
            edge = [i for i, (f, x, y, w, h) in enumerate(rois) if x + w == fr.shape[2] or y + h == fr.shape[1]]
            for i in (edge[:6] + list(range(0, len(rois), max(1, len(rois) // 6))))[:12]:
                f, x, y, w, h = rois[i]
                ro, _ = oracle.detect(a, np.ascontiguousarray(fr[f][y:y + h, x:x + w]))
                assert rows(r2.rects[r2.rects["frame"] == i]) == rows(ro), f"{win} {kind} roi {rois[i]}"


# ------------------------------------------------------------------------------------------------ OpenCV profile
# the edge-size frames are small: a tile needs only 64 windows in TILES, so that every scale that can take one does
TILES = (("cv_tile_min_windows0", 64), ("cv_tile_min_windows", 64))
CV_SETTINGS = [(), TILES, (("cv_tiles", 0),), TILES + (("cv_tiles_tilted", 0),), TILES + (("cv_tile_ws_max", 0),),
               TILES + (("cv_tile_ws_max", 64),), (("cv_row_band_px", 0),), TILES + (("cv_row_band_px", 0),)]


@pytest.mark.parametrize("win,kind", CELLS)
def test_opencv_paths_match_the_oracle(env, oracle, win, kind):
    """vj_detect_opencv on eight distinct edge-size frames with every tile / row setting (and cv_tree2 0 for the trees):
    the oracle's rectangles, visited windows and per-stage counts."""
    fr = frames(win)
    label = f"cv {win[0]}x{win[1]} {kind} {fr.shape[1]}x{fr.shape[2]}"
    settings = CV_SETTINGS + ([(("cv_tree2", 0),), TILES + (("cv_tree2", 0),)] if kind == "tree" else [])
    for s in settings:
        with tunables(env, *s):
            check_cv(env, oracle, win, kind, fr, f"{label} {s}")
    check_cv(env, oracle, win, kind, frames(win, (EDGE_SIZES[win][0] + 37, EDGE_SIZES[win][1] + 52), n=2), f"{label} odd size")


@pytest.mark.parametrize("win", GEOMETRY_WINDOWS, ids=WIN_IDS)
def test_opencv_grouping(env, oracle, win):
    """min_neighbors 1: the grouped rectangles are cv::groupRectangles of the oracle's raw candidates."""
    fr = frames(win)[0]
    for kind in GEOMETRY_KINDS:
        a, c = cascade(win, kind)
        ro, _ = oracle_of(oracle, win, kind, frames(win), "cv")[0]
        want, _ = oracle.group_rectangles(np.stack([ro[k] for k in ("x", "y", "w", "h")], 1), 1)
        got = env.detect_opencv(c, fr, min_neighbors=1)
        assert len(want) > 0
        assert sorted(tuple(int(r[k]) for k in ("x", "y", "w", "h")) for r in got.rects) == \
            sorted(tuple(int(v) for v in t) for t in want), f"{win} {kind}"


# ------------------------------------------------------------------------------------------------ 1080p, BGR
@pytest.mark.parametrize("kind", GEOMETRY_KINDS)
def test_one_1080p_frame_in_both_profiles(env, oracle, kind):
    win = (20, 20)
    fr = frames(win, (1080, 1920), n=1)
    r = check_clod(env, oracle, win, kind, fr, f"clod 1080p {kind}")
    assert "tile" in launch_kinds(r)
    check_cv(env, oracle, win, kind, fr, f"cv 1080p {kind}")


def test_bgr_input(env, oracle):
    """BGR frames, converted on the device: the oracle on the oracle's gray conversion, in both profiles."""
    win = (14, 28)
    h, w = EDGE_SIZES[win]
    rng = np.random.default_rng(28)
    bgr = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(3)]
    gray = np.stack([oracle.bgr2gray(b) for b in bgr])
    for kind in GEOMETRY_KINDS:
        a, c = cascade(win, kind)
        r = env.detect(c, bgr, default_params(flags=clod_flags(kind)), color=True)
        compare(r, [oracle.detect(a, g) for g in gray], c.info.n_stages, f"clod BGR {kind}")
        r = env.detect_opencv(c, bgr, flags=VJ_FLAG_COUNTERS, color=True)
        compare(r, [oracle.detect_opencvlike(a, g) for g in gray], c.info.n_stages, f"cv BGR {kind}", sort=True)
