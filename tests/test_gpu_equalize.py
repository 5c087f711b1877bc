"""VJ_FLAG_EQUALIZE_HIST and vj_equalize_hist on the device.  vj_equalize_hist byte for byte against the numpy
restatement (tests/equalize_oracle.py); the flag against the oracles ON THE EQUALIZED FRAMES, frame by frame, with rectangles, order
and counters — the contract: a call with the flag returns what the same call without it returns for the images vj_equalize_hist
gives.  All comparisons are exact.  The premise (equalization changes what the detector finds in these frames) is checked on the
CPU in tests/test_equalize_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import canny_oracle as co
import cv_rois_cases as cc
import equalize_oracle as eo
import find_biggest_oracle as fo
import mixed_cases as mc
import roc_oracle as ro
import scale_image_oracle as so
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_SCALE_IMAGE,
                                 VJ_FLAG_EQUALIZE_HIST, VJ_FLAG_SKIP_ROW, DeviceFrames, VjError, default_params, synth)
from test_gpu_mixed import _color, _device_frame, _strided_view

pytestmark = pytest.mark.gpu
EQ = VJ_FLAG_EQUALIZE_HIST
CNT = VJ_FLAG_COUNTERS
N = len(mc.SIZES)
NEVER = 2**64 - 1
VJ_ERR_ARG, VJ_ERR_UNSUPPORTED = 1, 4
CASC = "frontalface_alt"


# ------------------------------------------------------------------------------------------------------------ 1. vj_equalize_hist
@pytest.mark.parametrize("h", [1, 2, 5])
def test_small_widths_and_the_mask_of_a_rows_last_dword(env, h):
    rng = np.random.default_rng(h)
    for w in list(range(1, 10)) + [63, 64, 65, 255, 256, 257]:
        flat = np.full((h, w), 200, np.uint8)               # whole waves of one value, and one pixel that is not
        flat[-1, -1] = 7
        for g in (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(100, 104, (h, w), dtype=np.uint8), flat):
            assert np.array_equal(env.equalize_hist(g), eo.equalize(g)), (h, w)


def test_known_answers_on_the_device(env):
    assert env.equalize_hist(np.arange(7, dtype=np.uint8).reshape(1, 7).copy()).tolist() == [[0, 42, 85, 128, 170, 212, 255]]   # the ties go to even
    assert env.equalize_hist(np.array([[10, 20, 30, 40]], np.uint8)).tolist() == [[0, 85, 170, 255]]


@pytest.mark.parametrize("kind", ["constant0", "constant200", "two_valued", "all_values", "smooth", "noise", "blocks"])
def test_contents(env, kind):
    h, w = 480, 640
    if kind.startswith("constant"):
        g = np.full((h, w), int(kind[8:]), np.uint8)
    elif kind == "two_valued":
        g = np.where(np.random.default_rng(1).random((h, w)) < 0.3, 17, 230).astype(np.uint8)
    elif kind == "all_values":
        g = np.random.default_rng(2).permutation(np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
        assert len(np.unique(g)) == 256
    else:
        g = synth.frame(kind, 11, h, w)
    want = eo.equalize(g)
    assert np.array_equal(env.equalize_hist(g), want)
    if kind.startswith("constant"):
        assert np.array_equal(want, g)


def test_more_than_2_pow_24_pixels(env):
    """(float)sum rounds above 2^24 pixels; the lowest bin holds 10 pixels, so total - hist[i] is above 2^24 too."""
    h = w = 4100
    g = np.random.default_rng(3).integers(1, 256, (h, w), dtype=np.uint8)
    g.reshape(-1)[:: h * w // 10][:10] = 0
    assert int((g == 0).sum()) == 10 and g.size - 10 > 2**24
    assert np.array_equal(env.equalize_hist(g), eo.equalize(g))


def test_color_strided_device_and_sources_that_end_with_their_last_row(env, oracle):
    rng = np.random.default_rng(5)
    keep = []
    for i, (h, w, ch) in enumerate([(37, 61, 3), (37, 61, 4), (5, 7, 3), (61, 131, 1), (2, 257, 4), (33, 64, 1)]):
        img = _color(rng, h, w, ch)
        want = eo.equalize(img if ch == 1 else oracle.bgr2gray(img))
        assert np.array_equal(env.equalize_hist(np.ascontiguousarray(img), color=ch > 1), want), (h, w, ch)   # ends with its last row
        v, base = _strided_view(img, 7 if (w * ch) % 2 == 0 else 8)                                      # a strided host view
        assert v.strides[0] % 2 == 1
        assert np.array_equal(env.equalize_hist(v, color=ch > 1), want), (h, w, ch)
        d, t = _device_frame(img, 1 + 2 * (i % 2), 0 if (w * ch) % 2 else 3)                              # an odd address, stride > width
        assert d.ptr % 2 == 1 and d.stride % 2 == 1
        keep.append(t)
        assert np.array_equal(env.equalize_hist(d), want), (h, w, ch)
        d, t = _device_frame(img, 0, 0)                                                                   # tight rows, ends with the last row
        keep.append(t)
        assert np.array_equal(env.equalize_hist(d), want), (h, w, ch)


def test_argument_errors(env, lib):
    g = np.zeros((4, 8), np.uint8)
    out = np.zeros((4, 8), np.uint8)
    im, keep = env._one_image(g)
    f = lib.vj_equalize_hist
    assert f(None, C.byref(im), out.ctypes.data, 8) == VJ_ERR_ARG
    assert f(env._h, None, out.ctypes.data, 8) == VJ_ERR_ARG
    assert f(env._h, C.byref(im), None, 8) == VJ_ERR_ARG
    assert f(env._h, C.byref(im), out.ctypes.data, 7) == VJ_ERR_ARG
    for bad in (type(im)(None, 8, 4, 8, 0, 1), type(im)(im.data, 0, 4, 8, 0, 1), type(im)(im.data, 8, 4, 7, 0, 1), type(im)(im.data, 8, 4, 16, 0, 2)):
        assert f(env._h, C.byref(bad), out.ctypes.data, 8) == VJ_ERR_ARG
    assert f(env._h, C.byref(im), out.ctypes.data, 8) == 0


# ------------------------------------------------------------------------------------------------ 2. the flag: batches of one size
_BATCH = None


def batch3():
    """Three distinct 240 x 180 frames (two of them frames of tests/mixed_cases.py); built once, not modified."""
    global _BATCH
    if _BATCH is None:
        _BATCH = np.stack([cc.faces_frame(s, 180, 240, n_faces=3) for s in (1, 9, 4)])
        _BATCH.setflags(write=False)
        assert len({f.tobytes() for f in _BATCH}) == 3
    return _BATCH


_RES = {}


def per_frame(key, fn, frames):
    """[fn(frame)] for the frames of a list, computed once per key."""
    if key not in _RES:
        _RES[key] = [fn(f) for f in frames]
    return _RES[key]


def _sorted_raw(r):
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)


def _against(r, res, a, count=True, evals=True, least=10):
    """Rectangles per frame, their order, and the counters against per-frame (rectangles, stats) of an oracle."""
    windows, entered, n_evals = 0, np.zeros(a.n_stages, np.int64), 0
    for f, (want, st) in enumerate(res):
        assert mc.rows(r.rects[r.rects["frame"] == f]) == mc.rows(want), f"frame {f}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        n_evals += st["stump_evals"]
    assert len(r.rects) == sum(len(want) for want, _ in res) >= least
    _sorted_raw(r)
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if evals:
            assert r.stump_evals == n_evals


def test_detect_and_detect_opencv(env, oracle, cascades):
    """Fails where the bit is ignored: the oracle's lists differ between the frames and their equalized images."""
    c, a = cascades(CASC)
    fr = batch3()
    eq = eo.equalized(fr)
    clod = per_frame("clod", lambda f: oracle.detect(a, f), eq)
    cv = per_frame("cv", lambda f: oracle.detect_opencvlike(a, f), eq)
    assert all(mc.rows(x[0]) != mc.rows(oracle.detect(a, f)[0]) for x, f in zip(clod, fr))
    assert all(mc.rows(x[0]) != mc.rows(oracle.detect_opencvlike(a, f)[0]) for x, f in zip(cv, fr))
    r = env.detect(c, fr, default_params(flags=CNT | EQ))
    _against(r, clod, a)
    assert r.integral_ms > 0
    assert np.array_equal(env.detect(c, fr, default_params(flags=EQ)).rects, r.rects)     # uncounted kernels
    r = env.detect_opencv(c, fr, flags=CNT | EQ)
    _against(r, cv, a)
    assert np.array_equal(env.detect_opencv(c, fr, flags=EQ).rects, r.rects)
    # one frame, and the frames as BGR on the device (gray = the frame: 1868 + 9617 + 4899 = 16384)
    _against(env.detect_opencv(c, fr[1], flags=CNT | EQ), cv[1:2], a)
    import torch
    t = torch.from_numpy(np.repeat(fr[..., None], 3, axis=3).copy()).cuda()
    _against(env.detect_opencv(c, DeviceFrames.from_torch(t), flags=CNT | EQ), cv, a)
    _against(env.detect(c, DeviceFrames.from_torch(t), default_params(flags=CNT | EQ)), clod, a)


def test_detect_skip_mode_and_grouping(env, oracle, cascades):
    c, a = cascades(CASC)
    fr = batch3()
    eq = eo.equalized(fr)
    skip = per_frame("clod_skip_row", lambda f: oracle.detect(a, f, mode=3), eq)
    _against(env.detect(c, fr, default_params(flags=VJ_FLAG_SKIP_ROW | CNT | EQ)), skip, a, evals=False, least=3)
    g = env.detect(c, fr, default_params(min_neighbors=3, flags=EQ))
    clod = per_frame("clod", lambda f: oracle.detect(a, f), eq)
    groups = 0
    for f, (want, _) in enumerate(clod):   # (the library groups its sorted list: the oracle's order)
        xywh, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in want], np.int32).reshape(-1, 4), 3)
        mine = g.rects[g.rects["frame"] == f]
        assert [(int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in mine] == list(map(tuple, xywh.tolist())), f"frame {f}"
        assert [int(x["weight"]) for x in mine] == weights.tolist()
        groups += len(xywh)
    assert groups >= 3 and len(g.rects) == groups


def test_detect_opencv_modes(env, oracle, cascades):
    c, a = cascades(CASC)
    fr = batch3()
    eq = eo.equalized(fr)
    si = per_frame("si", lambda f: so.detect_scale_image(a, f), eq)
    _against(env.detect_opencv(c, fr, flags=VJ_FLAG_CV_SCALE_IMAGE | CNT | EQ), si, a)
    canny = per_frame("canny", lambda f: co.detect_opencvlike(a, f), eq)
    _against(env.detect_opencv(c, fr, flags=VJ_FLAG_CV_CANNY_PRUNING | CNT | EQ), canny, a, least=3)
    r = env.detect_opencv(c, fr, min_neighbors=3, flags=VJ_FLAG_CV_FIND_BIGGEST | CNT | EQ)
    big = per_frame("big", lambda f: fo.detect_biggest(a, f, min_neighbors=3), eq)
    want = [(f,) + tuple(res) for f, (res, _) in enumerate(big) if res is not None]
    assert [tuple(int(x[k]) for k in ("frame", "x", "y", "w", "h", "weight")) for x in r.rects] == want and len(want) >= 2
    assert r.windows == sum(st["windows"] for _, st in big)
    assert r.stage_entered == np.sum([st["stage_entered"] for _, st in big], axis=0).tolist()


def test_detect_opencv_roc(env, cascades):
    c, a = cascades(CASC)
    fr = batch3()
    eq = eo.equalized(fr)
    res = per_frame("roc", lambda f: ro.detect_roc(a, f), eq)

    def table(rects, levels, weights):
        return [(int(x["scale_idx"]), int(x["y"]), int(x["x"]), int(x["w"]), int(x["h"]), int(l), int(b))
                for x, l, b in zip(rects, levels, np.asarray(weights, np.float64).view(np.uint64))]

    for flags in (VJ_FLAG_CV_SCALE_IMAGE | EQ, VJ_FLAG_CV_SCALE_IMAGE | CNT | EQ):
        r = env.detect_opencv_roc(c, fr, flags=flags)
        _sorted_raw(r)
        for f, (rr, lv, lw, _) in enumerate(res):
            sel = r.rects["frame"] == f
            assert table(r.rects[sel], r.reject_levels[sel], r.level_weights[sel]) == table(rr, lv, lw), f"frame {f}"
        assert len(r.rects) == sum(len(x[0]) for x in res) >= 10


def test_a_batch_larger_than_max_subbatch_and_a_plain_call_afterwards(env, oracle, cascades):
    c, a = cascades(CASC)
    fr = batch3()
    eq = eo.equalized(fr)
    clod = per_frame("clod", lambda f: oracle.detect(a, f), eq)
    cv = per_frame("cv", lambda f: oracle.detect_opencvlike(a, f), eq)
    with tunables(env, ("max_subbatch", "2")):
        _against(env.detect(c, fr, default_params(flags=CNT | EQ)), clod, a)
        _against(env.detect_opencv(c, fr, flags=CNT | EQ), cv, a)
    # without the flag, right after calls with it: the frames as they are
    _against(env.detect(c, fr, default_params(flags=CNT)), per_frame("clod_plain", lambda f: oracle.detect(a, f), fr), a)
    _against(env.detect_opencv(c, fr, flags=CNT), per_frame("cv_plain", lambda f: oracle.detect_opencvlike(a, f), fr), a)


# ---------------------------------------------------------------------------------------------------- 3. the flag: mixed sizes
def _mixed_items():
    """The eleven frames; frame 2 as BGR on the host, frame 6 device-resident at an odd address (their gray images are the frames)."""
    items, keep = list(mc.frames()), []
    items[2] = np.repeat(items[2][..., None], 3, axis=2)
    d, t = _device_frame(items[6], 3, 5)
    items[6] = d
    keep.append(t)
    return items, keep


def _info(env):
    i = env.mixed_info()
    return dict(atlases=i.atlases, own_calls=i.own_calls, on_atlas=i.frames_atlas, own=i.frames_own_calls, oversized=i.frames_oversized)


ROUTES = [(dict(), (), dict(atlases=1, own_calls=0, on_atlas=N, own=0, oversized=0)),
          (dict(own_call_px=1), (), dict(atlases=0, own_calls=N - 1, on_atlas=0, own=N, oversized=0)),
          (dict(own_call_px=NEVER), (("max_subbatch", "4"),), dict(atlases=3, own_calls=0, on_atlas=N, own=0, oversized=0))]


@pytest.mark.parametrize("route", range(len(ROUTES)))
def test_mixed_calls(env, oracle, cascades, route):
    c, a = cascades(CASC)
    kw, settings, info = ROUTES[route]
    items, keep = _mixed_items()
    eq = eo.equalized(mc.frames())
    cv = per_frame("mixed_cv", lambda f: oracle.detect_opencvlike(a, f), eq)
    clod = per_frame("mixed_clod", lambda f: oracle.detect(a, f), eq)
    assert sum(1 for (x, _), (y, _) in zip(cv, mc.oracle_cv(oracle, CASC, a)) if mc.rows(x) != mc.rows(y)) >= 8
    with tunables(env, *settings):
        r = env.detect_opencv_mixed(c, items, flags=CNT | EQ, **kw)
        assert _info(env) == info
        _against(r, cv, a, least=40)
        r = env.detect_mixed(c, items, default_params(flags=CNT | EQ), **kw)
        assert _info(env) == info
        _against(r, clod, a, least=40)
    if route == 0:      # scale-image runs from the atlas too; and a plain call afterwards packs the frames as they are
        si = per_frame("mixed_si", lambda f: so.detect_scale_image(a, f), eq)
        r = env.detect_opencv_mixed(c, items, flags=VJ_FLAG_CV_SCALE_IMAGE | CNT | EQ)
        assert _info(env)["atlases"] == 1
        _against(r, si, a, least=40)
        _against(env.detect_opencv_mixed(c, items, flags=CNT), mc.oracle_cv(oracle, CASC, a), a, least=40)


# -------------------------------------------------------------------------------------------------------------- 4. the refusals
def test_entry_points_that_do_not_equalize_refuse_the_flag(env, lib, cascades):
    c, a = cascades(CASC)
    fr = batch3()
    rois = [(0, 0, 0, 100, 100)]
    windows, scales = [(0, 10, 10, 0)], [1.0]
    calls = [lambda: env.detect_rois(c, fr, rois, default_params(flags=EQ)),
             lambda: env.detect_chain(c, c, fr, default_params(flags=EQ), default_params()),
             lambda: env.detect_chain(c, c, fr, default_params(), default_params(flags=EQ)),
             lambda: env.detect_opencv_rois(c, fr, rois, flags=EQ),
             lambda: env.detect_opencv_chain(c, c, fr, flags=EQ),
             lambda: env.detect_opencv_chain(c, c, fr, flags_second=EQ),
             lambda: env.run_windows(c, fr, windows, scales, flags=EQ),
             lambda: env.stream(c, 240, 180, 2, default_params(flags=EQ))]
    for i, call in enumerate(calls):
        with pytest.raises(VjError) as ei:
            call()
        assert ei.value.code == VJ_ERR_UNSUPPORTED and "VJ_FLAG_EQUALIZE_HIST" in str(ei.value), i
