"""CV_HAAR_DO_CANNY_PRUNING on the device: vj_canny and vj_detect_opencv(VJ_FLAG_CV_CANNY_PRUNING) against the test restatement
(tests/canny_oracle.c), byte for byte and counter for counter."""
import numpy as np
import pytest

import canny_oracle as co
from cases import make_frame, tunables
from clfacedetection_amd import (CV_HAAR_DO_CANNY_PRUNING, CV_HAAR_FIND_BIGGEST_OBJECT, CV_HAAR_SCALE_IMAGE, VJ_FLAG_COUNTERS,
                                 VJ_FLAG_CV_CANNY_PRUNING, DeviceFrames, VjError, cvHaarDetectObjects, synth)
from test_canny_cpu import serpentine

pytestmark = pytest.mark.gpu
PRUNE = VJ_FLAG_CV_CANNY_PRUNING


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


@pytest.mark.parametrize("kind", ["noise", "smooth", "blocks", "xorshift"])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 37), (37, 1), (2, 2), (3, 3), (17, 29), (61, 131), (480, 640), (1080, 1920)])
def test_canny_matches_restatement(env, oracle, kind, h, w):
    g = make_frame(kind, 100 + h + w, h, w, oracle)
    assert np.array_equal(env.canny(g), co.canny(g))


def test_canny_large_and_patches(env, oracle):
    for g in (make_frame("noise", 5, 4096, 4096, oracle), co.patches_frame(4, 1080, 1920), co.black_edge_frame()):
        assert np.array_equal(env.canny(g), co.canny(g))


def test_canny_serpentine_across_many_tiles(env):
    for strong in (True, False):
        g = serpentine(600, 1500, strong)
        e = env.canny(g)
        assert np.array_equal(e, co.canny(g))
        assert e.any() == strong


@pytest.mark.parametrize("ch", [3, 4])
def test_canny_color_strided_and_device(env, oracle, ch):
    rng = np.random.default_rng(ch)
    img = synth.frame("blocks", 9, 200, 301)
    bgr = np.stack([img, rng.integers(0, 256, img.shape, dtype=np.uint8), img[::-1]] + [img] * (ch - 3), axis=2)
    want = co.canny(oracle.bgr2gray(bgr))
    assert np.array_equal(env.canny(bgr, color=True), want)
    big = np.zeros((200, 400, ch), np.uint8)          # a strided host view
    big[:, 50:351] = bgr
    assert np.array_equal(env.canny(big[:, 50:351], color=True), want)
    import torch
    t = torch.from_numpy(bgr[None].copy()).cuda()
    assert np.array_equal(env.canny(DeviceFrames.from_torch(t)), want)
    gray = synth.frame("noise", 3, 120, 161)          # gray, device-resident with a row stride > width
    tg = torch.zeros((120, 200), dtype=torch.uint8).cuda()
    tg[:, :161] = torch.from_numpy(gray).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(env.canny(DeviceFrames(tg.data_ptr(), 1, 120, 161, 200, 1)), co.canny(gray))


def _check_batch(env, c, a, frames, count=True, **kw):
    r = env.detect_opencv(c, frames, flags=PRUNE | (VJ_FLAG_COUNTERS if count else 0), **kw)
    windows, entered, evals = 0, np.zeros(a.n_stages, np.int64), 0
    for f in range(len(frames)):
        ro, st = co.detect_opencvlike(a, frames[f], min_size=kw.get("min_size", (0, 0)), scale_factor=kw.get("scale_factor", 1.1))
        assert rows(r.rects[r.rects["frame"] == f]) == rows(ro), f"frame {f}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        evals += st["stump_evals"]
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if all(int(n) == 1 for n in a.tree_n_nodes):   # (multi-node trees: the library counts every node of an entered stage)
            assert r.stump_evals == evals
    return r


def _mixed_batch(oracle, n, h, w, seed):
    out = []
    for i in range(n):
        k = i % 4
        out.append(co.patches_frame(seed + i, h, w) if k == 0 else co.soft_face_frame(h, w) if k == 1 and i < 4 else
                   make_frame(("noise", "smooth", "blocks")[i % 3], seed + i, h, w, oracle))
    return np.stack(out)


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_default", "frontalface_alt2", "frontalface_alt_tree", "eye",
                                  "mcs_nose"])
def test_detect_pruned_matches_restatement(env, oracle, cascades, casc):
    c, a = cascades(casc)
    frames = _mixed_batch(oracle, 8, 180, 240, 40)
    _check_batch(env, c, a, frames)
    _check_batch(env, c, a, frames, count=False)      # uncounted: the stage-tree chain sweep of the row kernel


def test_detect_pruned_min_size_scale_bgr_grouping(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames = _mixed_batch(oracle, 8, 240, 320, 70)
    _check_batch(env, c, a, frames, min_size=(40, 40), scale_factor=1.2)
    bgr = np.repeat(frames[..., None], 3, axis=3)
    bgr[..., 1] = frames[:, ::-1]
    r = env.detect_opencv(c, list(bgr), flags=PRUNE, color=True)
    for f in range(len(frames)):
        ro, _ = co.detect_opencvlike(a, oracle.bgr2gray(bgr[f]))
        assert rows(r.rects[r.rects["frame"] == f]) == rows(ro)
    g = env.detect_opencv(c, frames[0], min_neighbors=3, flags=PRUNE)
    ro, _ = co.detect_opencvlike(a, frames[0])
    want, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in ro], np.int32).reshape(-1, 4), 3)
    assert sorted(map(tuple, want.tolist())) == sorted((int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in g.rects)


def test_pruning_bites(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    r = _check_batch(env, c, a, np.stack([co.patches_frame(4, 240, 320)]))
    assert r.stage_entered[0] < r.windows // 2
    soft = co.soft_face_frame()
    on = _check_batch(env, c, a, np.stack([soft]))
    off = env.detect_opencv(c, soft, flags=VJ_FLAG_COUNTERS)
    assert len(off.rects) > 0 and len(on.rects) == 0 and on.stage_entered[0] == 0 and on.windows < off.windows
    r = _check_batch(env, c, a, np.stack([co.black_edge_frame()]))    # the sq < 20 clause decides windows of this frame:
    _, without_sq = co.detect_opencvlike(a, co.black_edge_frame(), sq_clause=False)
    assert r.stage_entered[0] < without_sq["stage_entered"][0]


def test_tunables_do_not_change_pruned_results(env, oracle, cascades):
    frames = _mixed_batch(oracle, 8, 180, 240, 90)
    for casc in ("frontalface_alt", "frontalface_alt_tree"):
        c, _ = cascades(casc)
        base = env.detect_opencv(c, frames, flags=PRUNE | VJ_FLAG_COUNTERS)
        for settings in ([("cv_tiles", "0")], [("cv_row_blocks", "1")], [("cv_tree_chains", "0")], [("cv_tail_max", "0")],
                         [("max_subbatch", "3")], [("cv_row_band_px", "0")], [("integral_rows", "0")], [("cv_tree2", "0")]):
            with tunables(env, *settings):
                r = env.detect_opencv(c, frames, flags=PRUNE | VJ_FLAG_COUNTERS)
            assert np.array_equal(r.rects, base.rects) and r.windows == base.windows and r.stage_entered == base.stage_entered, settings


def test_cv_haar_detect_objects_canny_pruning(env, cascades):
    c, _ = cascades("frontalface_alt")
    img = co.patches_frame(4, 240, 320)
    r = cvHaarDetectObjects(img, c, env, 1.1, 0, flags=CV_HAAR_DO_CANNY_PRUNING)
    assert np.array_equal(r.rects, env.detect_opencv(c, img, flags=PRUNE).rects)
    for flags in (CV_HAAR_SCALE_IMAGE, CV_HAAR_FIND_BIGGEST_OBJECT, 8):
        with pytest.raises(VjError):
            cvHaarDetectObjects(img, c, env, flags=flags)
