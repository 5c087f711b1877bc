"""CV_HAAR_FIND_BIGGEST_OBJECT on the device: vj_detect_opencv(VJ_FLAG_CV_FIND_BIGGEST) against the test restatement
(tests/find_biggest_oracle.c) — the one rectangle per frame with its neighbors, and the counters (windows, stage_entered), which pin
the scanROI's ranges and the break points.  The frames and their premises are checked in tests/test_find_biggest_cpu.py."""
import numpy as np
import pytest

import find_biggest_oracle as fo
import scale_image_oracle as so
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH,
                                 VJ_FLAG_CV_SCALE_IMAGE, cvHaarDetectObjects)

pytestmark = pytest.mark.gpu
FB = VJ_FLAG_CV_FIND_BIGGEST


def got_rows(r):
    return [tuple(int(x[k]) for k in ("frame", "x", "y", "w", "h")) + (int(x["weight"]),) for x in r.rects]


def _check(env, c, a, frames, flags=FB, **kw):
    """The batch through the library, every frame through the restatement: rectangles, windows and stage_entered must be equal."""
    r = env.detect_opencv(c, frames, flags=flags | VJ_FLAG_COUNTERS, **kw)
    want, windows, entered = [], 0, np.zeros(a.n_stages, np.int64)
    for f in range(len(frames)):
        res, st = fo.detect_biggest(a, frames[f], min_size=kw.get("min_size", (0, 0)), scale_factor=kw.get("scale_factor", 1.1),
                                    min_neighbors=kw.get("min_neighbors", 0), rough=bool(flags & VJ_FLAG_CV_ROUGH_SEARCH))
        if res is not None:
            want.append((f,) + tuple(res))
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
    print(f"find-biggest: {len(frames)} frames, rects {got_rows(r)} / {want}, windows {r.windows} / {windows}")
    assert got_rows(r) == want
    assert all(int(x["scale_idx"]) == -1 for x in r.rects)
    assert r.windows == windows and r.stage_entered == entered.tolist()
    assert r.launches == [] and r.n_cascade_launches >= 1      # no per-launch records; the true launch count
    return r, want


@pytest.mark.parametrize("casc", list(fo.CASES))
def test_matches_restatement(env, cascades, casc):
    """Stumps (nine distinct frames, two of them faceless), two-node trees, a stage tree, tilted features; batch and single frames."""
    c, a = cascades(casc)
    frames = fo.frames_for(casc)
    r, want = _check(env, c, a, frames, min_neighbors=3)
    assert len(want) == len(frames) - (2 if casc == "frontalface_alt" else 0)
    # the batch's result is the frames' own results, concatenated
    single = []
    for f in range(len(frames)):
        r1, _ = _check(env, c, a, frames[f:f + 1], min_neighbors=3)
        single += [(f,) + row[1:] for row in got_rows(r1)]
    assert single == got_rows(r)
    # uncounted calls run other kernel instantiations
    r0 = env.detect_opencv(c, frames, flags=FB, min_neighbors=3)
    assert np.array_equal(r0.rects, r.rects)


@pytest.mark.parametrize("min_neighbors", [0, 3, fo.HIGH_NEIGHBORS])
def test_min_neighbors(env, cascades, min_neighbors):
    c, a = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")
    _, want = _check(env, c, a, frames, min_neighbors=min_neighbors)
    if min_neighbors == fo.HIGH_NEIGHBORS:      # some frame with a face never groups, some does
        assert 0 < len(want) < len(frames) - 2


def test_rough_search(env, cascades):
    c, a = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")
    r, _ = _check(env, c, a, frames, flags=FB | VJ_FLAG_CV_ROUGH_SEARCH, min_neighbors=3)
    base, _ = _check(env, c, a, frames, min_neighbors=3)
    assert r.windows < base.windows


@pytest.mark.parametrize("scale_factor", [1.25, 2.0])
def test_scale_factors(env, cascades, scale_factor):
    c, a = cascades("frontalface_alt")
    _check(env, c, a, fo.frames_for("frontalface_alt"), min_neighbors=3, scale_factor=scale_factor)
    _, want = _check(env, c, a, so.face_grid_frame(so.GRID_SEED)[None], min_neighbors=3, scale_factor=scale_factor)
    assert len(want) == 1


@pytest.mark.parametrize("min_size", [fo.MIN_SIZE_CASE, fo.MIN_SIZE_BREAK])
def test_min_size(env, cascades, min_size):
    c, a = cascades("frontalface_alt")
    _, want = _check(env, c, a, fo.frames_for("frontalface_alt"), min_neighbors=3, min_size=min_size)
    assert (len(want) == 0) == (min_size == fo.MIN_SIZE_BREAK)


def test_large_frame_roi_scales_in_tile_range(env, cascades):
    """480 x 640 with a face of about 300 pixels: the scanROI's scales are ones the plain path puts on LDS tiles."""
    c, a = cascades("frontalface_alt")
    frame = fo.big_face_frame()
    _, want = _check(env, c, a, frame[None], min_neighbors=3)
    assert len(want) == 1 and want[0][3] > 250
    assert env.cv_plan_info(c, 640, 480, 1).n_tile_scales > 0


def test_bgr_input(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")[:4]
    bgr = np.repeat(frames[..., None], 3, axis=3)
    bgr[..., 1] = frames[:, ::-1]
    r = env.detect_opencv(c, list(bgr), flags=FB | VJ_FLAG_COUNTERS, min_neighbors=3, color=True)
    want, windows, entered = [], 0, np.zeros(a.n_stages, np.int64)
    for f in range(len(bgr)):
        res, st = fo.detect_biggest(a, oracle.bgr2gray(bgr[f]), min_neighbors=3)
        if res is not None:
            want.append((f,) + tuple(res))
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
    assert got_rows(r) == want and all(int(x["scale_idx"]) == -1 for x in r.rects)
    assert r.windows == windows and r.stage_entered == entered.tolist()
    assert len(want) >= 1


@pytest.mark.parametrize("scale_factor,min_neighbors", fo.LAST_SCALE_CASES)
def test_first_hit_after_the_last_scale(env, cascades, scale_factor, min_neighbors):
    """The first group forms only after the last scale of the walk: the grouping step runs there too, and the pushed maxRect is one of
    the result's neighbors.  Alone, and in a batch next to a frame that finds nothing."""
    c, a = cascades("frontalface_alt")
    frame = fo.last_scale_frame()
    from clfacedetection_amd import synth
    _, want = _check(env, c, a, frame[None], min_neighbors=min_neighbors, scale_factor=scale_factor)
    assert len(want) == 1
    batch = np.stack([synth.frame("smooth", 3, *frame.shape), frame, frame[::-1].copy()])
    _, want3 = _check(env, c, a, batch, min_neighbors=min_neighbors, scale_factor=scale_factor)
    assert (1,) + want[0][1:] in want3


def test_tunables_do_not_change_results(env, cascades):
    c, a = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")
    base, _ = _check(env, c, a, frames, min_neighbors=3)
    for settings in ([("max_subbatch", "3")], [("concurrent", "0")], [("det_cap", "4")], [("max_subbatch", "3"), ("det_cap", "2")]):
        with tunables(env, *settings):
            r, _ = _check(env, c, a, frames, min_neighbors=3)
        assert np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered, settings


def test_canny_and_scale_image_bits_change_nothing(env, cascades):
    c, a = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")[:4]
    base, _ = _check(env, c, a, frames, min_neighbors=3)
    for extra in (VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_CV_CANNY_PRUNING | VJ_FLAG_CV_SCALE_IMAGE):
        r, _ = _check(env, c, a, frames, flags=FB | extra, min_neighbors=3)
        assert np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered


def test_rough_search_alone_is_the_plain_path(env, cascades):
    c, _ = cascades("frontalface_alt")
    frames = fo.frames_for("frontalface_alt")
    for mn in (0, 3):
        plain = env.detect_opencv(c, frames, flags=VJ_FLAG_COUNTERS, min_neighbors=mn)
        rough = env.detect_opencv(c, frames, flags=VJ_FLAG_COUNTERS | VJ_FLAG_CV_ROUGH_SEARCH, min_neighbors=mn)
        assert len(plain.rects) > 9
        assert np.array_equal(rough.rects, plain.rects) and rough.windows == plain.windows and rough.stage_entered == plain.stage_entered


def test_through_cvHaarDetectObjects(env, cascades):
    c, a = cascades("frontalface_alt")
    img = fo.frames_for("frontalface_alt")[0]
    res, _ = fo.detect_biggest(a, img, min_neighbors=3)
    r = cvHaarDetectObjects(img, c, env, 1.1, 3, vj_flags=FB)
    assert got_rows(r) == [(0,) + tuple(res)]
