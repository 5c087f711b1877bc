"""CV_HAAR_SCALE_IMAGE on the device: vj_resize_linear and vj_detect_opencv(VJ_FLAG_CV_SCALE_IMAGE) against the test restatement
(tests/scale_image_oracle.c), byte for byte, rectangle for rectangle and counter for counter.  The frames and their premises (at
least 10 raw rectangles on three levels, a result unlike the scale-cascade path's) are checked in tests/test_scale_image_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import scale_image_oracle as so
from cases import make_frame, tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_SCALE_IMAGE, DeviceFrames, cvHaarDetectObjects,
                                 synth)
from clfacedetection_amd.api import RECT_DTYPE, CvParams, _Result

pytestmark = pytest.mark.gpu
SI = VJ_FLAG_CV_SCALE_IMAGE


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("h,w,dh,dw", [(37, 53, 37, 53), (37, 53, 19, 31), (61, 131, 55, 119), (3, 3, 2, 2), (4, 4, 7, 7), (1, 1, 1, 1),
                                       (40, 60, 20, 30), (40, 60, 40, 30), (480, 640, 436, 582), (1080, 1920, 982, 1745),
                                       (1080, 1920, 540, 960), (1200, 2100, 23, 41)])
def test_resize_matches_restatement(env, oracle, kind, h, w, dh, dw):
    g = make_frame(kind, 100 + h + w, h, w, oracle)
    assert np.array_equal(env.resize_linear(g, dw, dh), so.resize_linear(g, dw, dh))


@pytest.mark.parametrize("ch", [3, 4])
def test_resize_color_strided_and_device(env, oracle, ch):
    rng = np.random.default_rng(ch)
    img = synth.frame("blocks", 9, 200, 301)
    bgr = np.stack([img, rng.integers(0, 256, img.shape, dtype=np.uint8), img[::-1]] + [img] * (ch - 3), axis=2)
    want = so.resize_linear(oracle.bgr2gray(bgr), 211, 143)
    assert np.array_equal(env.resize_linear(bgr, 211, 143, color=True), want)
    big = np.zeros((200, 400, ch), np.uint8)          # a strided host view
    big[:, 50:351] = bgr
    assert np.array_equal(env.resize_linear(big[:, 50:351], 211, 143, color=True), want)
    import torch
    t = torch.from_numpy(bgr[None].copy()).cuda()
    assert np.array_equal(env.resize_linear(DeviceFrames.from_torch(t), 211, 143), want)
    gray = synth.frame("noise", 3, 120, 161)          # gray, device-resident with a row stride > width
    tg = torch.zeros((120, 200), dtype=torch.uint8).cuda()
    tg[:, :161] = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(env.resize_linear(DeviceFrames(tg.data_ptr(), 1, 120, 161, 200, 1), 80, 60), so.resize_linear(gray, 80, 60))
    assert np.array_equal(env.resize_linear(DeviceFrames(tg.data_ptr(), 1, 120, 161, 200, 1), 97, 71), so.resize_linear(gray, 97, 71))


def _check_batch(env, c, a, frames, count=True, flags=SI, **kw):
    r = env.detect_opencv(c, frames, flags=flags | (VJ_FLAG_COUNTERS if count else 0), **kw)
    windows, entered, evals = 0, np.zeros(a.n_stages, np.int64), 0
    for f in range(len(frames)):
        ro, st = so.detect_scale_image(a, frames[f], min_size=kw.get("min_size", (0, 0)), scale_factor=kw.get("scale_factor", 1.1))
        assert rows(r.rects[r.rects["frame"] == f]) == rows(ro), f"frame {f}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        evals += st["stump_evals"]
    assert len(r.rects) >= 10 * len(frames)
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if all(int(n) == 1 for n in a.tree_n_nodes):
            assert r.stump_evals == evals
        else:   # multi-node trees: the library counts every node of an entered stage, the restatement the nodes a walk visits
            nodes = [int(sum(a.tree_n_nodes[a.stage_first_tree[s]:a.stage_first_tree[s] + a.stage_n_trees[s]])) for s in range(a.n_stages)]
            assert r.stump_evals == sum(int(entered[s]) * nodes[s] for s in range(a.n_stages)) >= evals
    return r


@pytest.mark.parametrize("casc", list(so.CASES))
def test_detect_matches_restatement(env, cascades, casc):
    """Stumps, two-node trees, a stage tree and a cascade with tilted features; batches of 3 (9 for frontalface_alt) and of 1."""
    c, a = cascades(casc)
    frames = so.case_frames(casc)
    _check_batch(env, c, a, frames)
    _check_batch(env, c, a, frames, count=False)      # uncounted: the stage-tree chain sweep of the row kernel
    _check_batch(env, c, a, frames[:1])
    r = env.detect_opencv(c, frames, flags=SI)         # sorted by (frame, scale_idx, y, x)
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)
    # linear cascades: the large levels run on LDS tiles, batches of 1 and of 3 / 9 alike; the stage tree on the row kernel
    for n in (1, len(frames)):
        info = env.cv_plan_info(c, so.FRAME_W, so.FRAME_H, n, flags=SI)
        assert (info.n_tile_scales >= 3) == (casc != "frontalface_alt_tree"), (n, info.n_tile_scales)
    with tunables(env, ("cv_tiles", "0")):
        assert env.cv_plan_info(c, so.FRAME_W, so.FRAME_H, len(frames), flags=SI).n_tile_scales == 0


def test_detect_scale_factors_and_min_size(env, cascades):
    c, a = cascades("frontalface_alt")
    for seed, kw in so.PARAM_CASES:
        _check_batch(env, c, a, np.stack([so.faces_frame(seed, so.FRAME_H, so.FRAME_W)]), **kw)
    _check_batch(env, c, a, np.stack([so.face_grid_frame(so.GRID_SEED)]), scale_factor=2.0)    # the area level; levels with ystep = 1


def test_sub_batches_bgr_and_grouping(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames = so.case_frames("frontalface_alt")
    base = _check_batch(env, c, a, frames)
    with tunables(env, ("max_subbatch", "2")):
        r = _check_batch(env, c, a, frames)
    assert np.array_equal(r.rects, base.rects)
    bgr = np.repeat(frames[:3, ..., None], 3, axis=3)
    bgr[..., 1] = frames[:3, ::-1]
    r = env.detect_opencv(c, list(bgr), flags=SI, color=True)
    for f in range(3):
        ro, _ = so.detect_scale_image(a, oracle.bgr2gray(bgr[f]))
        assert rows(r.rects[r.rects["frame"] == f]) == rows(ro)
    g = env.detect_opencv(c, frames[0], min_neighbors=3, flags=SI)
    ro, _ = so.detect_scale_image(a, frames[0])
    order = np.lexsort((ro["x"], ro["y"], ro["scale_idx"]))    # the library groups its sorted list; the grouping is order-sensitive
    ro = ro[order]
    want, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in ro], np.int32).reshape(-1, 4), 3)
    assert len(want) > 0
    assert sorted(map(tuple, want.tolist())) == sorted((int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in g.rects)


def test_canny_flag_is_ignored(env, cascades):
    c, a = cascades("frontalface_alt")
    frames = so.case_frames("frontalface_alt")[:3]
    base = env.detect_opencv(c, frames, flags=SI | VJ_FLAG_COUNTERS)
    both = _check_batch(env, c, a, frames, flags=SI | VJ_FLAG_CV_CANNY_PRUNING)
    assert np.array_equal(both.rects, base.rects) and both.windows == base.windows and both.stage_entered == base.stage_entered


def test_tunables_do_not_change_results(env, cascades):
    """The OpenCV-profile tunables the new path reads (the row kernel's, the integral's, sub-batching), and the tile switches it
    must not be moved by."""
    for casc in ("frontalface_alt", "frontalface_alt2", "frontalface_alt_tree", "mcs_mouth"):
        c, _ = cascades(casc)
        frames = so.case_frames(casc)[:3]
        for count in (VJ_FLAG_COUNTERS, 0):
            base = env.detect_opencv(c, frames, flags=SI | count)
            for settings in ([("cv_tiles", "0")], [("cv_tile_min_windows", "256"), ("cv_tile_min_windows0", "256")], [("cv_tile_ws_max", "64")],
                             [("concurrent", "0")], [("cv_row_blocks", "1")], [("cv_tree_chains", "0")], [("cv_tail_max", "0")],
                             [("max_subbatch", "2")], [("cv_row_band_px", "0")], [("cv_row_band_px", "32")], [("integral_rows", "0")],
                             [("cv_tree2", "0")], [("cv_tiles_tilted", "0")]):
                with tunables(env, *settings):
                    r = env.detect_opencv(c, frames, flags=SI | count)
                assert np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered, settings


def test_c_abi_and_python_entry_points(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    img = so.faces_frame(7, so.FRAME_H, so.FRAME_W)
    ro, st = so.detect_scale_image(a, img)
    imgs, n, keep = env._images(img, False)
    p = CvParams(0, 0, 1.1, 0, SI | VJ_FLAG_COUNTERS)
    res = _Result()
    assert lib.vj_detect_opencv(env._h, c._h, imgs, n, C.byref(p), C.byref(res)) == 0
    try:
        got = np.frombuffer((C.c_char * (res.count * RECT_DTYPE.itemsize)).from_address(res.rects), RECT_DTYPE).copy()
        assert rows(got) == rows(ro) and int(res.counters.windows) == st["windows"]
    finally:
        lib.vj_result_free(C.byref(res))
    r = cvHaarDetectObjects(img, c, env, 1.1, 0, vj_flags=SI)     # the forwarded vj_flags reach the branch
    assert rows(r.rects) == rows(ro)
    assert rows(env.detect_opencv(c, img).rects) != rows(ro)      # and without the flag: the scale-cascade path, as before
