"""vj_detect_opencv_rois and vj_detect_opencv_chain on the device against the oracle on numpy crops (Oracle.detect_opencvlike,
Oracle.group_rectangles): rectangle for rectangle and counter for counter.  The cases and their premises — rectangles on three
scales, at least 10 per case, a region whose result is not the frame's restricted to it — are tests/cv_rois_cases.py and
tests/test_cv_rois_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import cv_rois_cases as cc
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_SCALE_IMAGE,
                                 DeviceFrames)
from clfacedetection_amd.api import CvParams, VjError, _Result

pytestmark = pytest.mark.gpu


def _check_rois(env, oracle, c, a, frames, rois, count=True, at_least=10, **kw):
    """Every region's rectangles equal the oracle's on the crop; counters are the sums over the regions.  at_least: the case's
    premise of 10 rectangles holds for its batch (tests/test_cv_rois_cpu.py); one frame of it alone must still give some."""
    r = env.detect_opencv_rois(c, frames, rois, flags=VJ_FLAG_COUNTERS if count else 0, **kw)
    res = cc.oracle_rois(oracle, a, frames, rois, **kw)
    windows, entered, evals, total = 0, np.zeros(a.n_stages, np.int64), 0, 0
    for i, (ro, st) in enumerate(res):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro), f"region {i} {tuple(rois[i])}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        evals += st["stump_evals"]
        total += len(ro)
    assert len(r.rects) == total and total >= at_least
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)                                   # sorted by (frame, scale_idx, y, x)
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if all(int(n) == 1 for n in a.tree_n_nodes):
            assert r.stump_evals == evals
        else:   # multi-node trees: the library counts every node of an entered stage, the oracle the nodes a walk visits
            nodes = [int(sum(a.tree_n_nodes[a.stage_first_tree[s]:a.stage_first_tree[s] + a.stage_n_trees[s]])) for s in range(a.n_stages)]
            assert r.stump_evals == sum(int(entered[s]) * nodes[s] for s in range(a.n_stages)) >= evals
    return r


def _per_region(env, c, frames, rois, color=False, **kw):
    """What the parent commit offers: one detect_opencv call per region on a sub-image view."""
    out = []
    for roi in rois:
        f, x, y, w, h = (int(v) for v in roi)
        if isinstance(frames, DeviceFrames):
            view = DeviceFrames(frames.ptr + f * frames.stride * frames.height + y * frames.stride + x * frames.channels, 1, h, w,
                                frames.stride, frames.channels)
        else:
            view = frames[f][y:y + h, x:x + w]
        out.append(env.detect_opencv(c, view, color=color, **kw))
    return out


def _same_as_per_region(r, parts):
    n = 0
    for i, part in enumerate(parts):
        mine = r.rects[r.rects["frame"] == i]
        assert len(mine) == len(part.rects), f"region {i}"
        for k in ("x", "y", "w", "h", "scale_idx", "weight"):
            assert np.array_equal(mine[k], part.rects[k]), f"region {i}: {k}"   # the same rectangles in the same order
        n += len(mine)
    assert n == len(r.rects)
    return n


@pytest.mark.parametrize("name", list(cc.CASES))
def test_fast_path_matches_the_oracle_on_crops(env, oracle, cascades, name):
    casc, seeds, kw = cc.CASES[name]
    c, a = cascades(casc)
    frames, rois = cc.case_frames(name), cc.case_rois(name)
    base = _check_rois(env, oracle, c, a, frames, rois, **kw)
    r = _check_rois(env, oracle, c, a, frames, rois, count=False, **kw)
    assert np.array_equal(r.rects, base.rects)
    one = rois[rois[:, 0] == 0]                                  # a batch of one frame
    _check_rois(env, oracle, c, a, frames[:1], one, at_least=3, **kw)
    _check_rois(env, oracle, c, a, frames[:1], one, count=False, at_least=3, **kw)
    with tunables(env, ("max_subbatch", "2")):                   # the batch split into sub-batches
        r = _check_rois(env, oracle, c, a, frames, rois, **kw)
    assert np.array_equal(r.rects, base.rects) and r.windows == base.windows


@pytest.mark.parametrize("name", ["stumps", "tilted", "eye"])
def test_grouped_per_region(env, oracle, cascades, name):
    casc, seeds, kw = cc.CASES[name]
    c, a = cascades(casc)
    frames, rois = cc.case_frames(name), cc.case_rois(name)
    g = env.detect_opencv_rois(c, frames, rois, min_neighbors=3, **kw)
    groups = 0
    for i, (ro, _) in enumerate(cc.oracle_rois(oracle, a, frames, rois, **kw)):
        ro = ro[np.lexsort((ro["x"], ro["y"], ro["scale_idx"]))]   # the library groups its sorted list; the grouping is order-sensitive
        want, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in ro], np.int32).reshape(-1, 4), 3)
        mine = g.rects[g.rects["frame"] == i]
        assert [(int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in mine] == list(map(tuple, want.tolist())), f"region {i}"
        assert [int(x["weight"]) for x in mine] == weights.tolist() and np.all(mine["scale_idx"] == -1)
        groups += len(want)
    assert groups >= 1 and len(g.rects) == groups


@pytest.mark.parametrize("name", ["stumps", "tilted"])
def test_equals_per_region_calls_gray_bgr_and_device(env, oracle, cascades, name):
    import torch
    casc, seeds, kw = cc.CASES[name]
    c, a = cascades(casc)
    frames, rois = cc.case_frames(name), cc.case_rois(name)
    for mn in (0, 3):
        r = env.detect_opencv_rois(c, frames, rois, min_neighbors=mn, **kw)                       # gray host frames
        assert _same_as_per_region(r, _per_region(env, c, frames, rois, min_neighbors=mn, **kw)) >= 1
    bgr = np.repeat(frames[..., None], 3, axis=3)                                                 # BGR host frames
    bgr[..., 1] = frames[:, ::-1]
    bgr[..., 2] = frames[:, :, ::-1]
    r = env.detect_opencv_rois(c, list(bgr), rois, color=True, **kw)
    assert _same_as_per_region(r, _per_region(env, c, list(bgr), rois, color=True, **kw)) >= 10
    gray = np.stack([oracle.bgr2gray(b) for b in bgr])
    for i, (ro, _) in enumerate(cc.oracle_rois(oracle, a, gray, rois, **kw)):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)
    n, h, w = frames.shape                                                                        # DeviceFrames, row stride above the width
    stride = w + 40
    t = torch.zeros((n, h, stride), dtype=torch.uint8).cuda()
    t[:, :, :w] = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    dev = DeviceFrames(t.data_ptr(), n, h, w, stride, 1)
    r = env.detect_opencv_rois(c, dev, rois, **kw)
    assert _same_as_per_region(r, _per_region(env, c, dev, rois, **kw)) >= 10
    for i, (ro, _) in enumerate(cc.oracle_rois(oracle, a, frames, rois, **kw)):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)


@pytest.mark.parametrize("flag,mn", [(VJ_FLAG_CV_CANNY_PRUNING, 0), (VJ_FLAG_CV_SCALE_IMAGE, 0), (VJ_FLAG_CV_FIND_BIGGEST, 2),
                                     (VJ_FLAG_CV_CANNY_PRUNING | VJ_FLAG_COUNTERS, 3)])
def test_fallback_flags_equal_per_region_calls(env, cascades, flag, mn):
    c, a = cascades("frontalface_alt")
    frames, rois = cc.case_frames("stumps"), cc.case_rois("stumps")
    r = env.detect_opencv_rois(c, frames, rois, flags=flag, min_neighbors=mn)
    parts = _per_region(env, c, frames, rois, flags=flag, min_neighbors=mn)
    assert _same_as_per_region(r, parts) >= 3
    if flag & VJ_FLAG_COUNTERS:
        assert r.windows == sum(p.windows for p in parts) and r.stage_entered == np.sum([p.stage_entered for p in parts], axis=0).tolist()


def test_frames_of_differing_sizes_take_the_fallback(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames = [cc.faces_frame(1), cc.faces_frame(2, 150, 200), cc.faces_frame(3)]
    rois = np.array([(0, 37, 21, 155, 133), (1, 11, 9, 160, 131), (2, 0, 0, 240, 180), (1, 0, 0, 200, 150), (0, 5, 3, 29, 29)], np.int32)
    r = env.detect_opencv_rois(c, frames, rois, flags=VJ_FLAG_COUNTERS)
    windows = 0
    for i, roi in enumerate(rois):
        ro, st = oracle.detect_opencvlike(a, np.ascontiguousarray(cc.crop(frames, roi)))
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)
        windows += st["windows"]
    assert r.windows == windows and len(r.rects) >= 10
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)


def test_argument_handling(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    frames = cc.case_frames("stumps")
    r = env.detect_opencv_rois(c, frames, np.zeros((0, 5), np.int32), flags=VJ_FLAG_COUNTERS)    # zero regions: VJ_OK, nothing
    assert len(r.rects) == 0 and r.windows == 0
    small = np.array([(0, 5, 3, 29, 29), (2, 199, 150, 31, 22)], np.int32)                        # too small for any scale
    r = env.detect_opencv_rois(c, frames, small, flags=VJ_FLAG_COUNTERS)
    assert len(r.rects) == 0 and r.windows == 0
    for bad in [(0, 200, 0, 41, 50), (0, 0, 150, 50, 31), (0, -1, 0, 50, 50), (0, 0, -1, 50, 50), (3, 0, 0, 50, 50), (-1, 0, 0, 50, 50),
                (0, 10, 10, 0, 50), (0, 10, 10, 50, -3)]:
        for flags in (0, VJ_FLAG_CV_SCALE_IMAGE):
            with pytest.raises(VjError) as ei:
                env.detect_opencv_rois(c, frames, np.array([(0, 0, 0, 100, 100), bad], np.int32), flags=flags)
            assert ei.value.code == 1, bad                                                          # VJ_ERR_ARG
    with pytest.raises(VjError) as ei:
        env.detect_opencv_rois(c, frames, np.array([(0, 0, 0, 100, 100)], np.int32), scale_factor=1.0)
    assert ei.value.code == 1
    # the C entry points: null arguments
    p = CvParams(0, 0, 1.1, 0, 0)
    res, res2 = _Result(), _Result()
    imgs, n, keep = env._images(frames, False)
    assert lib.vj_detect_opencv_rois(env._h, c._h, imgs, n, None, 1, C.byref(p), C.byref(res)) == 1
    assert lib.vj_detect_opencv_rois(env._h, c._h, imgs, n, None, 0, C.byref(p), C.byref(res)) == 0 and res.count == 0
    assert lib.vj_detect_opencv_chain(env._h, c._h, None, imgs, n, C.byref(p), C.byref(p), C.byref(res), C.byref(res2)) == 1
    assert lib.vj_detect_opencv_chain(env._h, c._h, c._h, imgs, 0, C.byref(p), C.byref(p), C.byref(res), C.byref(res2)) == 0


def _same_result(x, y):
    assert np.array_equal(x.rects, y.rects)


@pytest.mark.parametrize("name", list(cc.CHAIN_CASES))
def test_chain(env, oracle, cascades, name):
    first, second, seeds, mn = cc.CHAIN_CASES[name]
    c1, a1 = cascades(first)
    c2, a2 = cascades(second)
    frames = cc.chain_frames(name)
    r1, r2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=mn, flags=VJ_FLAG_COUNTERS, flags_second=VJ_FLAG_COUNTERS)
    base = env.detect_opencv(c1, frames, min_neighbors=mn, flags=VJ_FLAG_COUNTERS)               # out_first is detect_opencv's
    _same_result(r1, base)
    assert r1.windows == base.windows and r1.stage_entered == base.stage_entered
    regions = np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)
    want = env.detect_opencv_rois(c2, frames, regions, flags=VJ_FLAG_COUNTERS)                    # out_second is detect_opencv_rois' on them
    _same_result(r2, want)
    assert r2.windows == want.windows and r2.stage_entered == want.stage_entered
    o_regions, o_res = cc.oracle_chain(oracle, a1, a2, frames, mn)                                # and both are the oracle's
    assert np.array_equal(regions, o_regions) and len(regions) >= 5
    for i, (ro, _) in enumerate(o_res):
        assert cc.rows(r2.rects[r2.rects["frame"] == i]) == cc.rows(ro), f"region {i}"
    assert r2.windows == sum(st["windows"] for _, st in o_res)
    assert len(r2.rects) == sum(len(ro) for ro, _ in o_res) >= 3
    with tunables(env, ("max_subbatch", "1")):                                                    # sub-batches: the same
        s1, s2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=mn)
    _same_result(s1, r1)
    _same_result(s2, r2)
    g1, g2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=mn, min_neighbors_second=2)    # the second cascade grouped per region
    _same_result(g1, r1)
    _same_result(g2, env.detect_opencv_rois(c2, frames, regions, min_neighbors=2))


def test_chain_with_a_fallback_flag_and_device_frames(env, cascades):
    import torch
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = cc.chain_frames("alt2_lefteye_grouped")
    r1, r2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=3)
    t = torch.from_numpy(frames.copy()).cuda()
    torch.cuda.synchronize()
    d1, d2 = env.detect_opencv_chain(c1, c2, DeviceFrames.from_torch(t), min_neighbors=3)
    _same_result(d1, r1)
    _same_result(d2, r2)
    assert len(r2.rects) >= 10
    f1, f2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=3, flags_second=VJ_FLAG_CV_SCALE_IMAGE)   # the two public calls
    _same_result(f1, r1)
    regions = np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)
    _same_result(f2, env.detect_opencv_rois(c2, frames, regions, flags=VJ_FLAG_CV_SCALE_IMAGE))

