"""vj_detect_opencv_rois with VJ_FLAG_CV_SCALE_IMAGE on the device: every region's level images on canvases, one pass per canvas
(route 2 of vj_cv_rois_info), against the scale-image oracle on numpy crops (scale_image_oracle.detect_scale_image)
— rectangle for rectangle, counter for counter — and against one detect_opencv call per region.  The cases and their premises —
rectangles on six factor numbers, the 2 x 2 mean levels, step-1 levels, a region whose result is not the frame's restricted to it —
are tests/cv_rois_cases.py and tests/test_cv_rois_scale_image_cpu.py."""
import functools

import numpy as np
import pytest

import cv_rois_cases as cc
import scale_image_oracle as so
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH,
                                 VJ_FLAG_CV_SCALE_IMAGE, DeviceFrames)
from clfacedetection_amd.api import VjError
from test_cv_rois_scale_image_cpu import _arrays, oracle_crops
from test_gpu_cv_rois import _per_region, _same_as_per_region

pytestmark = pytest.mark.gpu

SI = VJ_FLAG_CV_SCALE_IMAGE
CASES = dict(cc.CASES, stumps_sf2=("frontalface_alt", cc.CASES["stumps"][1], {"scale_factor": 2.0}))   # the 2 x 2 mean levels


def _frames(name):
    return np.stack([cc.faces_frame(s) for s in CASES[name][1]])


def _rois(name):
    return np.array([(f, *r) for r in cc.REGIONS for f in range(len(CASES[name][1]))], np.int32)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's (rectangles, stats) per region of the case: computed once, shared, never written to."""
    casc, seeds, kw = CASES[name]
    return oracle_crops(_arrays(casc), _frames(name), _rois(name), **kw)


def _check(env, c, a, name, count=True):
    """Every region's rectangles equal the oracle's on the crop; the counters are the sums over the regions (the multi-node rule of
    test_gpu_cv_rois._check_rois for stump_evals)."""
    casc, seeds, kw = CASES[name]
    frames, rois, res = _frames(name), _rois(name), _oracle(name)
    r = env.detect_opencv_rois(c, frames, rois, flags=SI | (VJ_FLAG_COUNTERS if count else 0), **kw)
    info = env.cv_rois_info()
    windows, entered, evals, total, levels = 0, np.zeros(a.n_stages, np.int64), 0, 0, 0
    for i, (ro, st) in enumerate(res):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro), f"region {i} {tuple(rois[i])}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        evals += st["stump_evals"]
        total += len(ro)
        levels += st["n_levels"]
    assert len(r.rects) == total
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)                                   # sorted by (frame, scale_idx, y, x)
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if all(int(n) == 1 for n in a.tree_n_nodes):
            assert r.stump_evals == evals
        else:   # multi-node trees: the library counts every node of an entered stage, the oracle the nodes a walk visits
            nodes = [int(sum(a.tree_n_nodes[a.stage_first_tree[s]:a.stage_first_tree[s] + a.stage_n_trees[s]])) for s in range(a.n_stages)]
            assert r.stump_evals == sum(int(entered[s]) * nodes[s] for s in range(a.n_stages)) >= evals
    assert info.route == 2 and info.regions == len(rois) and info.level_images == levels and info.windows == windows
    assert info.canvases >= 1 and info.canvas_w >= a.win_w and info.canvas_h >= a.win_h and info.pyramid_ms > 0
    return r, info


@pytest.mark.parametrize("name", list(CASES))
def test_level_canvases_match_the_oracle_on_crops(env, cascades, name):
    c, a = cascades(CASES[name][0])
    base, info = _check(env, c, a, name)
    assert len(base.rects) >= (1 if name == "eye" else 10)
    r, _ = _check(env, c, a, name, count=False)
    assert np.array_equal(r.rects, base.rects)
    with tunables(env, ("max_subbatch", "2")):                   # the frames split into sub-batches, so the canvases too
        r, split = _check(env, c, a, name)
    assert np.array_equal(r.rects, base.rects) and r.windows == base.windows
    # (a canvas never spans two sub-batches of frames: three frames make two; the case of two frames stays one sub-batch)
    assert split.canvases >= (2 if len(CASES[name][1]) > 2 else 1) and split.level_images == info.level_images


@pytest.mark.parametrize("name", ["stumps", "tilted"])
def test_grouped_per_region(env, oracle, cascades, name):
    c, a = cascades(CASES[name][0])
    casc, seeds, kw = CASES[name]
    g = env.detect_opencv_rois(c, _frames(name), _rois(name), min_neighbors=3, flags=SI, **kw)
    assert env.cv_rois_info().route == 2
    groups = 0
    for i, (ro, _) in enumerate(_oracle(name)):
        ro = ro[np.lexsort((ro["x"], ro["y"], ro["scale_idx"]))]   # the library groups its sorted list; the grouping is order-sensitive
        want, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in ro], np.int32).reshape(-1, 4), 3)
        mine = g.rects[g.rects["frame"] == i]
        assert [(int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in mine] == list(map(tuple, want.tolist())), f"region {i}"
        assert [int(x["weight"]) for x in mine] == weights.tolist() and np.all(mine["scale_idx"] == -1)
        groups += len(want)
    assert groups >= 1 and len(g.rects) == groups


@pytest.mark.parametrize("name", ["stumps", "tilted"])
def test_equals_per_region_calls_gray_bgr_and_device(env, oracle, cascades, name):
    """Regions touching every frame edge, at odd origins: a tap clamped to the frame instead of the crop reads the neighbour pixel
    and changes a level image's border."""
    import torch
    c, a = cascades(CASES[name][0])
    casc, seeds, kw = CASES[name]
    frames, rois = _frames(name), _rois(name)
    for mn in (0, 3):
        r = env.detect_opencv_rois(c, frames, rois, min_neighbors=mn, flags=SI, **kw)               # gray host frames
        assert env.cv_rois_info().route == 2
        assert _same_as_per_region(r, _per_region(env, c, frames, rois, min_neighbors=mn, flags=SI, **kw)) >= 1
    bgr = np.repeat(frames[..., None], 3, axis=3)                                                 # BGR host frames
    bgr[..., 1] = frames[:, ::-1]
    bgr[..., 2] = frames[:, :, ::-1]
    r = env.detect_opencv_rois(c, list(bgr), rois, color=True, flags=SI, **kw)
    assert env.cv_rois_info().route == 2
    assert _same_as_per_region(r, _per_region(env, c, list(bgr), rois, color=True, flags=SI, **kw)) >= 10
    gray = np.stack([oracle.bgr2gray(b) for b in bgr])
    for i, (ro, _) in enumerate(oracle_crops(a, gray, rois, **kw)):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)
    n, h, w = frames.shape                                                                        # DeviceFrames, row stride above the width
    stride = w + 40
    t = torch.full((n, h, stride), 255, dtype=torch.uint8).cuda()                                 # (what lies beyond the width is not the frame)
    t[:, :, :w] = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    dev = DeviceFrames(t.data_ptr(), n, h, w, stride, 1)
    r = env.detect_opencv_rois(c, dev, rois, flags=SI, **kw)
    assert env.cv_rois_info().route == 2
    assert _same_as_per_region(r, _per_region(env, c, dev, rois, flags=SI, **kw)) >= 10
    for i, (ro, _) in enumerate(_oracle(name)):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)


def test_routes(env, cascades):
    c, a = cascades("frontalface_alt")
    frames, rois = _frames("stumps"), _rois("stumps")
    base = env.detect_opencv_rois(c, frames, rois, flags=SI | VJ_FLAG_COUNTERS)
    assert env.cv_rois_info().route == 2 and len(base.rects) >= 10
    for extra in (VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_ROUGH_SEARCH):                              # not read next to scale-image
        r = env.detect_opencv_rois(c, frames, rois, flags=SI | VJ_FLAG_COUNTERS | extra)
        assert env.cv_rois_info().route == 2
        assert np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered
    r = env.detect_opencv_rois(c, frames, rois, flags=SI | VJ_FLAG_CV_FIND_BIGGEST, min_neighbors=2)   # clears scale-image: the old route
    assert env.cv_rois_info().route == 3
    assert _same_as_per_region(r, _per_region(env, c, frames, rois, flags=SI | VJ_FLAG_CV_FIND_BIGGEST, min_neighbors=2)) >= 3
    mixed = [cc.faces_frame(1), cc.faces_frame(2, 150, 200), cc.faces_frame(3)]                   # frames of differing sizes
    mrois = np.array([(0, 37, 21, 155, 133), (1, 11, 9, 160, 131), (2, 0, 0, 240, 180), (1, 0, 0, 200, 150), (0, 5, 3, 29, 29)], np.int32)
    r = env.detect_opencv_rois(c, mixed, mrois, flags=SI)
    assert env.cv_rois_info().route == 3
    for i, roi in enumerate(mrois):
        ro, _ = so.detect_scale_image(a, np.ascontiguousarray(cc.crop(mixed, roi)))
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(ro)
    assert len(r.rects) >= 10
    many = np.array([(f, 2 * k, k, 131, 97) for f in range(3) for k in range(11)], np.int32)      # 33 regions of ONE size: more than
    r = env.detect_opencv_rois(c, frames, many, flags=SI)                                         # 32 per size keep the per-size route
    assert env.cv_rois_info().route == 3
    assert _same_as_per_region(r, _per_region(env, c, frames, many, flags=SI)) >= 10
    r2 = env.detect_opencv_rois(c, frames, many[:32], flags=SI)                                   # 32 of them: level canvases, the same
    assert env.cv_rois_info().route == 2
    assert np.array_equal(r2.rects, r.rects[r.rects["frame"] < 32])
    env.detect_opencv_rois(c, frames, rois)                                                       # flags 0
    info = env.cv_rois_info()
    assert info.route == 1 and info.canvases == 0 and info.level_images == 0 and info.windows > 0


def test_argument_handling(env, lib, cascades):
    import ctypes as C
    from clfacedetection_amd.api import CvRoisInfo
    c, a = cascades("frontalface_alt")
    frames = _frames("stumps")
    r = env.detect_opencv_rois(c, frames, np.zeros((0, 5), np.int32), flags=SI | VJ_FLAG_COUNTERS)    # zero regions: VJ_OK, nothing
    assert len(r.rects) == 0 and r.windows == 0 and env.cv_rois_info().regions == 0
    small = np.array([(0, 5, 3, a.win_w - 1, 40), (2, 199, 150, 40, a.win_h - 1)], np.int32)          # smaller than the window: no level
    r = env.detect_opencv_rois(c, frames, small, flags=SI | VJ_FLAG_COUNTERS)
    info = env.cv_rois_info()
    assert len(r.rects) == 0 and r.windows == 0 and info.route == 2 and info.level_images == 0 and info.canvases == 0
    for bad in [(0, 200, 0, 41, 50), (0, 0, 150, 50, 31), (0, -1, 0, 50, 50), (0, 0, -1, 50, 50), (3, 0, 0, 50, 50), (-1, 0, 0, 50, 50),
                (0, 10, 10, 0, 50), (0, 10, 10, 50, -3)]:
        with pytest.raises(VjError) as ei:
            env.detect_opencv_rois(c, frames, np.array([(0, 0, 0, 100, 100), bad], np.int32), flags=SI)
        assert ei.value.code == 1, bad                                                              # VJ_ERR_ARG
    out = CvRoisInfo()
    assert lib.vj_cv_rois_info_get(env._h, None) == 1 and lib.vj_cv_rois_info_get(None, C.byref(out)) == 1


def test_chain_with_a_scale_image_second_cascade(env, cascades):
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = cc.chain_frames("alt2_lefteye_grouped")
    r1, r2 = env.detect_opencv_chain(c1, c2, frames, min_neighbors=3, flags_second=SI)
    assert env.cv_chain_info().handoff == 3                                                       # the two public calls ...
    assert env.cv_rois_info().route == 2                                                          # ... the second on level canvases
    regions = np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)
    want = env.detect_opencv_rois(c2, frames, regions, flags=SI)
    assert env.cv_rois_info().route == 2 and env.cv_rois_info().regions == len(regions) >= 5
    assert np.array_equal(r2.rects, want.rects) and len(r2.rects) >= 1
    assert _same_as_per_region(want, _per_region(env, c2, frames, regions, flags=SI)) >= 1


def test_a_region_too_large_for_a_canvas_takes_the_per_size_route(env, cascades):
    """Route 4: the level images of a 2048 x 1536 region hold more pixels than a canvas (2^24), so that region goes through one
    detect_opencv call while the others share a canvas; the merged result is what per-region calls give, in their order."""
    from clfacedetection_amd import synth
    c, a = cascades("frontalface_alt")
    frames = synth.frame("faces", 3, 1536, 2048)[None]
    rois = np.array([(0, 101, 57, 400, 300), (0, 0, 0, 2048, 1536), (0, 1300, 900, 333, 251), (0, 7, 3, 1200, 900)], np.int32)
    for mn in (0, 3):
        r = env.detect_opencv_rois(c, frames, rois, flags=SI | VJ_FLAG_COUNTERS, min_neighbors=mn)
        info = env.cv_rois_info()
        # (regions are taken in order: the region that fits no canvas ends the one before it, so there is one on either side)
        assert info.route == 4 and info.canvases == 2 and info.regions == 4
        parts = _per_region(env, c, frames, rois, flags=SI | VJ_FLAG_COUNTERS, min_neighbors=mn)
        assert _same_as_per_region(r, parts) >= 3
        assert r.windows == sum(p.windows for p in parts) and r.stage_entered == np.sum([p.stage_entered for p in parts], axis=0).tolist()
        assert r.stump_evals == sum(p.stump_evals for p in parts)
        assert info.windows == sum(p.windows for i, p in enumerate(parts) if i != 1)
