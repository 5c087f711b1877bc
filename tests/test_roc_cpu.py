"""cvHaarDetectObjectsForROC without a GPU: the premises of the GPU cases (tests/test_gpu_roc.py), the ROC restatement
(tests/roc_oracle.c) against the existing scale-image restatement, and vj_group_rectangles_levels — host code of libvjhip, which
loads without a device — against the restatement of groupRectangles' level overload."""
import os

import numpy as np
import pytest

import heavy_cases as hc
import roc_oracle as ro
import scale_image_oracle as so
from clfacedetection_amd import group_rectangles_levels
from clfacedetection_amd.api import DATA_DIR, RECT_DTYPE
from oracle.oracle import load_vjc

_RAW = {}


def arrays(casc):
    return load_vjc(os.path.join(DATA_DIR, f"haarcascade_{casc}.vjc"))


def raw(casc, seed):
    """(cascade arrays, rects, levels, weights) of the oracle on one case frame; computed once."""
    if (casc, seed) not in _RAW:
        a = arrays(casc)
        _RAW[(casc, seed)] = (a,) + ro.detect_roc(a, so.faces_frame(seed, ro.FRAME_H, ro.FRAME_W))[:3]
    return _RAW[(casc, seed)]


@pytest.mark.parametrize("casc", list(ro.PREMISE_SEEDS))
def test_premises_linear(casc):
    seen = set()
    for seed in ro.PREMISE_SEEDS[casc]:
        a, r, lv, lw = raw(casc, seed)
        n = a.n_stages
        assert set(lv.tolist()) <= {n - 3, n - 2, n - 1, n}
        assert (lv < n).sum() >= 5 and (lv == n).sum() >= 10, (seed, np.unique(lv, return_counts=True))
        seen |= set(lv[lv < n].tolist())
    assert seen == {n - 3, n - 2, n - 1}, seen


def test_premises_stage_tree():
    for seed in ro.CASES["frontalface_alt_tree"]:
        a, r, lv, lw = raw("frontalface_alt_tree", seed)
        assert len(lv) >= 10 and (lv == a.n_stages).all()     # a stage tree returns 0 on every reject: nothing else is reported


def test_default_seed_search():
    """frontalface_default: the first seed from 3 upwards whose frame shows level 22 is the one the cases list."""
    a = arrays("frontalface_default")
    for seed in range(3, 40):
        lv = raw("frontalface_default", seed)[2]
        if (lv == a.n_stages - 3).any():
            break
    assert seed == ro.CASES["frontalface_default"][2] == ro.PREMISE_SEEDS["frontalface_default"][2]


def test_premise_wide_frame_rows_overflow_the_queue():
    f = hc.frame_of(ro.WIDE_SPEC)
    for form in ro.WIDE_FORMS:
        a = ro.wide_cascade(form)
        assert a.n_stages == 4
        v, _ = so.level_verdicts(a, f, 2)
        assert ((v != 0).sum(1) > ro.CV_QCAP - 64).any()      # stage-0 survivors of one row of level 0


@pytest.mark.parametrize("casc", list(ro.CASES))
def test_roc_against_scale_image_restatement(casc):
    """The entries at level n are exactly the plain call's rectangles; every entry's level is what level_verdicts says of its
    window (on the level's own image: checked on level 0, where the image is the frame)."""
    for seed in ro.CASES[casc][:3]:
        a, r, lv, lw = raw(casc, seed)
        n = a.n_stages
        plain, _ = so.detect_scale_image(a, so.faces_frame(seed, ro.FRAME_H, ro.FRAME_W))
        assert sorted(map(tuple, r[lv == n].tolist())) == sorted(map(tuple, plain.tolist()))
        key = [(int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r]
        assert key == sorted(key) and len(set(key)) == len(key)
        v, _ = so.level_verdicts(a, so.faces_frame(seed, ro.FRAME_H, ro.FRAME_W), 2)
        want = {}
        for iy in range(v.shape[0]):
            for ix in range(v.shape[1]):
                res = -n if v[iy, ix] > 0 else int(v[iy, ix])
                if n + res < 4:
                    want[(2 * ix, 2 * iy)] = -res
        got = {(int(x["x"]), int(x["y"])): int(l) for x, l in zip(r, lv) if x["scale_idx"] == 0}
        assert got == want


def _lib_group(r, lv, lw, thr, frame=0):
    rects = np.zeros(len(r), RECT_DTYPE)
    for k in ("x", "y", "w", "h"):
        rects[k] = r[k]
    rects["frame"] = frame
    return group_rectangles_levels(rects, lv, lw, thr)


def _same(got, want):
    g, glv, glw = got
    w, wlv, wlw = want
    assert [tuple(int(x[k]) for k in "xywh") for x in g] == [tuple(map(int, x)) for x in w]
    assert glv.tolist() == wlv.tolist() and np.array_equal(glw.view(np.uint64), wlw.view(np.uint64))


def test_group_levels_on_oracle_lists():
    """Without vj_group_rectangles_levels this fails.  The raw lists of every case frame at thresholds 0, 1, 3 and n_stages - 2;
    the last one drops the classes whose best level is a near-miss (on these frames: classes of frontalface_default, _alt2 and
    mcs_mouth; every class of frontalface_alt holds a pass) and keeps the others."""
    dropped = kept = 0
    for casc, seeds in ro.CASES.items():
        for seed in seeds:
            a, r, lv, lw = raw(casc, seed)
            xywh = np.array([[x["x"], x["y"], x["w"], x["h"]] for x in r], np.int32)
            n_out = {}
            for thr in (0, 1, 3, a.n_stages - 2):
                got = _lib_group(r, lv, lw, thr)
                _same(got, ro.group_levels(xywh, lv, lw, thr))
                n_out[thr] = len(got[0])
                if thr > 0:
                    assert (got[0]["scale_idx"] == -1).all() and (got[0]["weight"] == 0).all()
                    assert (got[1] > thr).all()
                else:
                    assert len(got[0]) == len(r) and (got[1] == 1).all()      # (:147-156: nothing grouped, the levels set to 1)
            dropped += n_out[1] - n_out[a.n_stages - 2]
            kept += n_out[a.n_stages - 2]
    assert dropped > 0 and kept > 0


def test_group_levels_small_lists():
    r1 = np.zeros(1, RECT_DTYPE)
    r1["w"] = r1["h"] = 20
    e = group_rectangles_levels(r1[:0], [], [], 3)
    assert len(e[0]) == len(e[1]) == len(e[2]) == 0
    g = group_rectangles_levels(r1, [22], [1.5], 3)                     # one rectangle: kept by its level, not its member count
    assert len(g[0]) == 1 and g[1].tolist() == [22] and g[2].tolist() == [1.5]
    assert len(group_rectangles_levels(r1, [3], [1.5], 3)[0]) == 0
    r = np.zeros(4, RECT_DTYPE)
    r["w"] = r["h"] = 30
    r["x"] = [10, 11, 12, 11]
    xywh = np.array([[x["x"], x["y"], x["w"], x["h"]] for x in r], np.int32)
    for lv, lw in (([21, 21, 21, 21], [0.25, 3.5, -1.0, 2.0]),           # equal levels, differing weights: the greatest
                   ([20, 21, 21, 19], [9.0, -2.0, -0.5, 7.0]),           # the greatest weight AT the greatest level
                   ([21, 21, 21, 21], [-4.0, -0.125, -3.0, -8.0]),       # all negative: the first replaces DBL_MIN, then the greatest
                   ([0, 0, 0, 0], [-4.0, -1.0, -3.0, -8.0])):            # no level above 0: DBL_MIN would stay (the class is dropped)
        for thr in (1, 20):
            _same(group_rectangles_levels(r, lv, lw, thr), ro.group_levels(xywh, lv, lw, thr))
    g = group_rectangles_levels(r, [21, 21, 21, 21], [-4.0, -0.125, -3.0, -8.0], 1)
    assert g[1].tolist() == [21] and g[2].tolist() == [-0.125]
    two = np.concatenate([r, r])                                          # two frames: grouped one by one
    two["frame"][4:] = 1
    g = group_rectangles_levels(two, [21] * 4 + [5] * 4, [1.0] * 8, 10)
    assert g[0]["frame"].tolist() == [0] and g[1].tolist() == [21]
