"""CV_HAAR_DO_CANNY_PRUNING on the CPU: the test restatement (tests/canny_oracle.c) against the oracle and against
hand-derived known answers of the Canny specification."""
import numpy as np
import pytest

import canny_oracle as co
from cases import MODE_CASES, make_frame
from clfacedetection_amd import (CV_HAAR_DO_CANNY_PRUNING, CV_HAAR_DO_ROUGH_SEARCH, CV_HAAR_FIND_BIGGEST_OBJECT,
                                 CV_HAAR_SCALE_IMAGE, VJ_FLAG_CV_CANNY_PRUNING, VjError, cvHaarDetectObjects)


@pytest.mark.parametrize("case", MODE_CASES, ids=[c[0] for c in MODE_CASES])
def test_restatement_without_pruning_is_the_oracle(case, oracle, cascades):
    cid, name, gen, seed, h, w = case
    _, arrays = cascades(name)
    g = make_frame(gen, seed, h, w, oracle)
    r0, s0 = oracle.detect_opencvlike(arrays, g)
    r1, s1 = co.detect_opencvlike(arrays, g, prune=False)
    assert np.array_equal(r0, r1)
    assert s0 == s1


def _cols(e):
    return sorted(np.flatnonzero(e.any(axis=0)).tolist())


def test_canny_constant_frame():
    assert not co.canny(np.full((20, 30), 77, np.uint8)).any()


def test_canny_step_200():
    f = np.zeros((16, 16), np.uint8)
    f[:, 7:] = 200
    e = co.canny(f)
    assert _cols(e) == [6] and (e[:, 6] == 255).all()


@pytest.mark.parametrize("v,cols", [(12, []), (13, [6])])   # m = 4 v: 48 is weak only, 52 is strong
def test_canny_step_threshold(v, cols):
    f = np.zeros((16, 16), np.uint8)
    f[:, 7:] = v
    e = co.canny(f)
    assert _cols(e) == cols
    if cols:
        assert (e[:, 6] == 255).all() and int(e.sum()) == 255 * 16


def test_canny_single_pixel():
    f = np.zeros((9, 9), np.uint8)
    f[4, 4] = 25                       # m = 2 v = 50 at all eight neighbours: not > 50
    assert not co.canny(f).any()
    f[4, 4] = 26
    e = co.canny(f)
    expect = np.zeros((9, 9), np.uint8)
    expect[3:6, 3:6] = 255
    expect[4, 4] = 0
    assert np.array_equal(e, expect)


def serpentine(h, w, strong, v=6, pitch=8, bw=3):
    """A band of gray v (max |dx| + |dy| <= 8 v = 48: weak everywhere) snaking over the frame; `strong`: one pixel of 60 at the
    start of the band, the far end of the path."""
    f = np.zeros((h, w), np.uint8)
    cols = list(range(4, w - 4 - bw, pitch))
    for i, c in enumerate(cols):
        f[4:h - 4, c:c + bw] = v
        if i + 1 < len(cols):
            r = h - 4 - bw if i % 2 == 0 else 4
            f[r:r + bw, c:cols[i + 1] + bw] = v
    if strong:
        f[h // 2, 4] = 60
    return f


def _components(mask):
    """8-connected components of a boolean mask (flood fill; no scipy here)."""
    lab = np.zeros(mask.shape, np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if lab[y0, x0]:
            continue
        n += 1
        stack = [(y0, x0)]
        lab[y0, x0] = n
        while stack:
            y, x = stack.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < mask.shape[0] and 0 <= xx < mask.shape[1] and mask[yy, xx] and not lab[yy, xx]:
                        lab[yy, xx] = n
                        stack.append((yy, xx))
    return n


def test_hysteresis_follows_a_long_weak_path():
    e = co.canny(serpentine(64, 200, strong=True))
    assert _components(e > 0) == 1
    assert e[:, :8].any() and e[:, -16:].any()     # from the strong pixel to the far end of the band
    assert int((e > 0).sum()) > 2000


def test_hysteresis_without_a_strong_pixel():
    assert not co.canny(serpentine(64, 200, strong=False)).any()


def test_pruning_changes_the_walk_on_flat_content(oracle, cascades):
    _, arrays = cascades("frontalface_alt")
    g = co.patches_frame(4, 240, 320)
    r0, s0 = co.detect_opencvlike(arrays, g, prune=False)
    r1, s1 = co.detect_opencvlike(arrays, g, prune=True)
    assert s1["stage_entered"][0] < s1["windows"] // 2
    assert s1["stage_entered"][0] < s0["stage_entered"][0]
    g = co.soft_face_frame()
    assert not co.canny(g).any()
    r0, _ = co.detect_opencvlike(arrays, g, prune=False)
    r1, s1 = co.detect_opencvlike(arrays, g, prune=True)
    assert len(r0) > 0 and len(r1) == 0 and s1["stage_entered"][0] == 0


def test_black_edge_frame_exercises_the_sq_clause(cascades):
    """Windows whose pruning rectangle is black but ends on an edge column: s >= 100, sq = 0.  Without the sq < 20 half of the test
    more windows would be evaluated."""
    _, arrays = cascades("frontalface_alt")
    g = co.black_edge_frame()
    _, with_sq = co.detect_opencvlike(arrays, g)
    _, without_sq = co.detect_opencvlike(arrays, g, sq_clause=False)
    assert with_sq["windows"] == without_sq["windows"]
    assert with_sq["stage_entered"][0] < without_sq["stage_entered"][0]


def test_flag_values():
    assert (CV_HAAR_DO_CANNY_PRUNING, CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT, CV_HAAR_DO_ROUGH_SEARCH) == (1, 2, 4, 8)
    assert VJ_FLAG_CV_CANNY_PRUNING == 1 << 6


@pytest.mark.parametrize("flags", [CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT, CV_HAAR_DO_ROUGH_SEARCH,
                                   CV_HAAR_DO_CANNY_PRUNING | CV_HAAR_SCALE_IMAGE])
def test_other_haar_flags_are_refused(flags):
    with pytest.raises(VjError, match="CV_HAAR_DO_CANNY_PRUNING"):
        cvHaarDetectObjects(np.zeros((40, 40), np.uint8), None, None, flags=flags)
