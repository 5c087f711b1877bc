"""cvHaarDetectObjectsForROC on the device: vj_detect_opencv_roc against the test restatement (tests/roc_oracle.c).  Comparisons
are exact — rectangles, scale_idx and levels equal, weights equal as bit patterns: the sums are the ones the verdicts depend on.
The frames and their premises (every near-miss level occurs, at least 5 near-misses a frame) are checked in tests/test_roc_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import heavy_cases as hc
import roc_oracle as ro
import scale_image_oracle as so
from cases import cascade_to_product, tunables
from clfacedetection_amd import (CV_HAAR_SCALE_IMAGE, VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST,
                                 VJ_FLAG_CV_SCALE_IMAGE, DeviceFrames, VjError, cvHaarDetectObjectsForROC)
from clfacedetection_amd.api import RECT_DTYPE, CvRocParams, _RocResult

pytestmark = pytest.mark.gpu
SI = VJ_FLAG_CV_SCALE_IMAGE
VJ_ERR_UNSUPPORTED = 4
_ORACLE = {}


def oracle_raw(a, frame, **kw):
    """The restatement's raw lists of one frame, computed once per (cascade, frame, parameters)."""
    key = (a.name, a.n_stages, frame.shape, hash(frame.tobytes()), tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = ro.detect_roc(a, frame, **kw)
    return _ORACLE[key]


def table(rects, levels, weights, frame=None):
    """Rows (scale_idx, y, x, w, h, level, weight bits) in list order."""
    sel = slice(None) if frame is None else rects["frame"] == frame
    r, lv, lw = rects[sel], np.asarray(levels)[sel], np.asarray(weights, np.float64)[sel]
    return [(int(x["scale_idx"]), int(x["y"]), int(x["x"]), int(x["w"]), int(x["h"]), int(l), int(b))
            for x, l, b in zip(r, lv, lw.view(np.uint64))]


def check(env, c, a, frames, flags=SI, color=False, gray=None, **kw):
    """One raw call against the restatement, frame by frame; returns the result."""
    r = env.detect_opencv_roc(c, frames, flags=flags, color=color, **kw)
    assert r.reject_levels.dtype == np.int32 and r.level_weights.dtype == np.float64
    assert len(r.rects) == len(r.reject_levels) == len(r.level_weights)
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)                                             # sorted by (frame, scale_idx, y, x)
    assert (r.rects["weight"] == 0).all()
    n = len(frames) if not isinstance(frames, DeviceFrames) else len(gray)
    for f in range(n):
        ro_r, ro_lv, ro_lw, _ = oracle_raw(a, frames[f] if gray is None else gray[f], **kw)
        assert table(r.rects, r.reject_levels, r.level_weights, f) == table(ro_r, ro_lv, ro_lw), f"frame {f}"   # (the oracle's order is the sorted one)
    return r


def same(r, base):
    assert np.array_equal(r.rects, base.rects) and np.array_equal(r.reject_levels, base.reject_levels)
    assert np.array_equal(r.level_weights.view(np.uint64), base.level_weights.view(np.uint64))


@pytest.mark.parametrize("casc", list(ro.CASES))
def test_raw_lists_match_restatement(env, cascades, casc):
    """Stumps (f64 two_rects stages among them), two-node trees, tilted features and a stage tree; counted and uncounted calls take
    different stage-tree forms (the lockstep sweep; the prefix and the chain sweep)."""
    c, a = cascades(casc)
    frames = ro.case_frames(casc)
    r = check(env, c, a, frames)
    n = a.n_stages
    if casc != "frontalface_alt_tree":
        assert set(r.reject_levels.tolist()) == {n - 3, n - 2, n - 1, n}
    else:
        assert set(r.reject_levels.tolist()) == {n}
    same(check(env, c, a, frames, flags=SI | VJ_FLAG_COUNTERS), r)
    check(env, c, a, frames[:1])


SETTINGS = ([("cv_tail_max", "0")], [("cv_tree_chains", "0")], [("cv_tree2", "0")], [("cv_tiles", "0")], [("cv_tiles", "1")],
            [("cv_tiles_tilted", "0")], [("cv_row_blocks", "1")], [("max_subbatch", "2")], [("concurrent", "0")])


@pytest.mark.parametrize("casc", list(ro.CASES))
def test_tunables_do_not_change_results(env, cascades, casc):
    c, a = cascades(casc)
    frames = ro.case_frames(casc)[:3]
    for count in (0, VJ_FLAG_COUNTERS):
        base = check(env, c, a, frames, flags=SI | count)
        for settings in SETTINGS:
            with tunables(env, *settings):
                r = env.detect_opencv_roc(c, frames, flags=SI | count)
            same(r, base)
            assert r.windows == base.windows and r.stage_entered == base.stage_entered, settings


@pytest.mark.parametrize("casc", list(ro.CASES))
def test_counters_equal_the_plain_call(env, cascades, casc):
    c, _ = cascades(casc)
    frames = ro.case_frames(casc)[:3]
    r = env.detect_opencv_roc(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    p = env.detect_opencv(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    assert r.windows == p.windows > 0 and r.stage_entered == p.stage_entered and r.stump_evals == p.stump_evals > 0


@pytest.mark.parametrize("form", ro.WIDE_FORMS)
def test_mid_row_queue_flush(env, form):
    """A 64 x 1400 frame whose rows of level 0 hold 690 stage-0 survivors each: the wave's queue is flushed inside the row (the
    premise is asserted here on the CPU, as in tests/test_roc_cpu.py).  Every grid position is reported, level 3 or 4."""
    a = ro.wide_cascade(form)
    f = hc.frame_of(ro.WIDE_SPEC)
    v, _ = so.level_verdicts(a, f, 2)
    assert ((v != 0).sum(1) > ro.CV_QCAP - 64).any()
    c = cascade_to_product(a)
    for count in (0, VJ_FLAG_COUNTERS):
        r = check(env, c, a, f[None], flags=SI | count)
        assert set(r.reject_levels.tolist()) == {3, 4}
    assert r.windows == len(r.rects)


def test_many_reports_and_regrow(env, cascades):
    """The first 4 stages of frontalface_alt: every stage-0 survivor is reported (levels 1-4), from a detection buffer of one
    record, so that the call has to grow it.  The first 3 stages alone are refused."""
    _, full = cascades("frontalface_alt")
    a4 = ro.first_stages(full, 4)
    c4 = cascade_to_product(a4)
    frame = so.faces_frame(1, ro.FRAME_H, ro.FRAME_W)
    with tunables(env, ("det_cap", "1")):
        r = check(env, c4, a4, frame[None], flags=SI | VJ_FLAG_COUNTERS)
        again = check(env, c4, a4, frame[None])
    same(again, r)
    assert set(r.reject_levels.tolist()) == {1, 2, 3, 4}
    assert len(r.rects) == r.stage_entered[1] > 1000                       # every stage-0 survivor
    c3 = cascade_to_product(ro.first_stages(full, 3))
    with pytest.raises(VjError) as ei:
        env.detect_opencv_roc(c3, frame)
    assert ei.value.code == VJ_ERR_UNSUPPORTED


def test_parameters(env, cascades):
    c, a = cascades("frontalface_alt")
    f7 = so.faces_frame(7, ro.FRAME_H, ro.FRAME_W)[None]
    check(env, c, a, so.faces_frame(1, ro.FRAME_H, ro.FRAME_W)[None], scale_factor=1.25)
    whole = check(env, c, a, f7)
    r = check(env, c, a, f7, min_size=(40, 40))                            # leading levels are skipped and keep their scale_idx
    assert len(r.rects) > 0 and r.rects["scale_idx"].min() > 0
    n_all = oracle_raw(a, f7[0])[3]
    rmax = check(env, c, a, f7, max_size=(60, 60), flags=SI | VJ_FLAG_COUNTERS)   # the loop ends early
    n_max = oracle_raw(a, f7[0], max_size=(60, 60))[3]
    assert 0 < n_max < n_all and len(rmax.rects) > 0 and rmax.rects["w"].max() <= 60
    assert rmax.windows < env.detect_opencv_roc(c, f7, flags=SI | VJ_FLAG_COUNTERS).windows
    both = check(env, c, a, f7, min_size=(40, 40), max_size=(60, 60))
    assert len(both.rects) > 0 and both.rects["w"].min() >= 40 and both.rects["w"].max() <= 60
    same(check(env, c, a, f7, max_size=(0, 60)), whole)                    # a zero member: the frame
    same(check(env, c, a, f7, max_size=(ro.FRAME_W, ro.FRAME_H)), whole)   # another max that cuts nothing, after one that did
    same(check(env, c, a, f7, max_size=(60, 60)), rmax)
    g = check(env, c, a, so.face_grid_frame(so.GRID_SEED)[None], scale_factor=2.0)   # levels with ystep 1
    assert len(g.rects) > 0


@pytest.mark.parametrize("casc", ["frontalface_alt", "mcs_mouth", "frontalface_alt_tree"])
def test_grouping(env, cascades, casc):
    c, a = cascades(casc)
    frames = ro.case_frames(casc)[:3]
    for thr in (3, a.n_stages - 2):
        g = env.detect_opencv_roc(c, frames, min_neighbors=thr)
        assert (g.rects["weight"] == 0).all() and (g.rects["scale_idx"] == -1).all()
        assert list(g.rects["frame"]) == sorted(g.rects["frame"])
        total = 0
        for f in range(len(frames)):
            r, lv, lw, _ = oracle_raw(a, frames[f])                        # the oracle's own list is in sorted order
            want, wlv, wlw = ro.group_levels(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in r], np.int32), lv, lw, thr)
            sel = g.rects["frame"] == f
            assert [tuple(int(x[k]) for k in "xywh") for x in g.rects[sel]] == [tuple(map(int, x)) for x in want]
            assert g.reject_levels[sel].tolist() == wlv.tolist()
            assert np.array_equal(g.level_weights[sel].view(np.uint64), wlw.view(np.uint64))
            total += len(want)
        assert total > 0


def test_bgr_strided_and_device_frames(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames = ro.case_frames("frontalface_alt")[:3]
    bgr = np.repeat(frames[..., None], 3, axis=3)
    bgr[..., 1] = frames[:, ::-1]
    gray = [oracle.bgr2gray(b) for b in bgr]
    base = check(env, c, a, list(bgr), color=True, gray=gray)
    big = np.zeros((3, ro.FRAME_H, ro.FRAME_W + 100, 3), np.uint8)          # strided host views
    big[:, :, 50:50 + ro.FRAME_W] = bgr
    same(check(env, c, a, [b[:, 50:50 + ro.FRAME_W] for b in big], color=True, gray=gray), base)
    import torch
    t = torch.from_numpy(bgr.copy()).cuda()
    same(check(env, c, a, DeviceFrames.from_torch(t), gray=gray), base)
    tg = torch.from_numpy(frames.copy()).cuda()
    check(env, c, a, DeviceFrames.from_torch(tg), gray=list(frames))


def test_refusals_and_ignored_flags(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    frames = ro.case_frames("frontalface_alt")[:2]
    imgs, n, keep = env._images(frames, False)
    for flags in (0, VJ_FLAG_COUNTERS, SI | VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_CANNY_PRUNING):
        p = CvRocParams(0, 0, 0, 0, 1.1, 0, flags)
        res = _RocResult()
        res.r.count = 7                                                    # `out` comes back empty
        assert lib.vj_detect_opencv_roc(env._h, c._h, imgs, n, C.byref(p), C.byref(res)) == VJ_ERR_UNSUPPORTED
        assert res.r.count == 0 and not res.r.rects and not res.reject_levels and not res.level_weights
        with pytest.raises(VjError) as ei:
            env.detect_opencv_roc(c, frames, flags=flags)
        assert ei.value.code == VJ_ERR_UNSUPPORTED
    base = check(env, c, a, frames)
    same(check(env, c, a, frames, flags=SI | VJ_FLAG_CV_CANNY_PRUNING), base)


def test_c_abi_and_python_entry_points(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    img = so.faces_frame(7, ro.FRAME_H, ro.FRAME_W)
    r0, lv0, lw0, _ = oracle_raw(a, img)
    imgs, n, keep = env._images(img, False)
    p = CvRocParams()
    lib.vj_cv_roc_params_default(C.byref(p))
    assert (p.min_w, p.min_h, p.max_w, p.max_h, p.scale_factor, p.min_neighbors, p.flags) == (0, 0, 0, 0, 1.1, 0, SI)
    assert C.sizeof(CvRocParams) == 32
    p.flags |= VJ_FLAG_COUNTERS
    res = _RocResult()
    assert lib.vj_detect_opencv_roc(env._h, c._h, imgs, n, C.byref(p), C.byref(res)) == 0
    try:
        m = int(res.r.count)
        rects = np.frombuffer((C.c_char * (m * RECT_DTYPE.itemsize)).from_address(res.r.rects), RECT_DTYPE).copy()
        lv = np.ctypeslib.as_array((C.c_int32 * m).from_address(res.reject_levels)).copy()
        lw = np.ctypeslib.as_array((C.c_double * m).from_address(res.level_weights)).copy()
        assert table(rects, lv, lw) == table(r0, lv0, lw0) and int(res.r.counters.windows) > 0
    finally:
        lib.vj_roc_result_free(C.byref(res))
    assert res.r.count == 0 and not res.r.rects and not res.reject_levels and not res.level_weights
    lib.vj_roc_result_free(C.byref(res))                                   # (idempotent)
    r = cvHaarDetectObjectsForROC(img, c, env, 1.1, 0)                     # flags = CV_HAAR_SCALE_IMAGE by default
    assert table(r.rects, r.reject_levels, r.level_weights) == table(r0, lv0, lw0)
    g = cvHaarDetectObjectsForROC(img, c, env, flags=CV_HAAR_SCALE_IMAGE)  # min_neighbors = 3 by default
    want = ro.group_levels(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in r0], np.int32), lv0, lw0, 3)
    assert len(want[0]) > 0 and [tuple(int(x[k]) for k in "xywh") for x in g.rects] == [tuple(map(int, x)) for x in want[0]]
    assert g.reject_levels.tolist() == want[1].tolist()
    with pytest.raises(VjError):
        cvHaarDetectObjectsForROC(img, c, env, flags=0)


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_alt_tree"])
def test_plain_call_before_and_after(env, cascades, casc):
    """The plan caches must not mix: a plain scale-image call gives the same result before and after a ROC call."""
    c, a = cascades(casc)
    frames = ro.case_frames(casc)[:3]
    before = env.detect_opencv(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    roc = check(env, c, a, frames, max_size=(80, 80))
    check(env, c, a, frames)
    after = env.detect_opencv(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    assert np.array_equal(before.rects, after.rects) and before.windows == after.windows and before.stage_entered == after.stage_entered
    n = a.n_stages
    full = check(env, c, a, frames)
    passes = full.rects[full.reject_levels == n]
    assert np.array_equal(passes, before.rects)                            # and the ROC call's passes are the plain call's rectangles
    assert len(roc.rects) < len(full.rects)
