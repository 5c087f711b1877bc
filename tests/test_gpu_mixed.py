"""vj_detect_mixed, vj_detect_opencv_mixed and vj_pack_frames on the device: a batch of frames of differing sizes gives, frame by
frame, what the oracle (Oracle.detect_opencvlike, Oracle.detect, Oracle.group_rectangles) gives for the frame alone, and what one
detect_opencv / detect call per frame — what a caller had to write before — returns; whichever way the call is routed.  The frames
and their premises are tests/mixed_cases.py and tests/test_mixed_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import mixed_cases as mc
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_FIND_BIGGEST, VJ_FLAG_CV_ROUGH_SEARCH,
                                 VJ_FLAG_CV_SCALE_IMAGE, VJ_FLAG_SIGNED_MEAN, VJ_FLAG_SKIP_ROW, VJ_FLAG_TILTED_AS_UPRIGHT, DeviceFrames,
                                 default_params)
from clfacedetection_amd.api import CvParams, MixedInfo, MixedOpts, Params, VjError, _Image, _Result

pytestmark = pytest.mark.gpu

N = len(mc.SIZES)
NEVER = 2**64 - 1


def _sorted_by_frame(r):
    if np.all(r.rects["scale_idx"] == -1):                      # grouped objects: frame by frame, in groupRectangles' class order
        assert np.all(np.diff(r.rects["frame"]) >= 0)
        return
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)                                   # raw candidates: sorted by (frame, scale_idx, y, x)


def _same_as_per_frame(r, parts):
    """The same rectangles in the same order as one call per frame."""
    n = 0
    for i, part in enumerate(parts):
        mine = r.rects[r.rects["frame"] == i]
        assert len(mine) == len(part.rects), f"frame {i}"
        for k in ("x", "y", "w", "h", "scale_idx", "weight"):
            assert np.array_equal(mine[k], part.rects[k]), f"frame {i}: {k}"
        n += len(mine)
    assert n == len(r.rects)
    _sorted_by_frame(r)
    return n


def _same_counters(r, parts):
    assert r.windows == sum(p.windows for p in parts)
    assert r.stage_entered == np.sum([p.stage_entered for p in parts], axis=0).tolist()
    assert r.stump_evals == sum(p.stump_evals for p in parts)


def _grouped_like_the_oracle(oracle, r, res, mn):
    groups = 0
    for i, (ro, _) in enumerate(res):
        ro = ro[np.lexsort((ro["x"], ro["y"], ro["scale_idx"]))]   # the library groups its sorted list; the grouping is order-sensitive
        want, weights = oracle.group_rectangles(np.array([[x["x"], x["y"], x["w"], x["h"]] for x in ro], np.int32).reshape(-1, 4), mn)
        mine = r.rects[r.rects["frame"] == i]
        assert [(int(x["x"]), int(x["y"]), int(x["w"]), int(x["h"])) for x in mine] == list(map(tuple, want.tolist())), f"frame {i}"
        assert [int(x["weight"]) for x in mine] == weights.tolist() and np.all(mine["scale_idx"] == -1)
        groups += len(want)
    assert groups >= 3 and len(r.rects) == groups


# ---------------------------------------------------------------------------------------------------------------- 1. pack_frames
def _color(rng, h, w, ch):
    return rng.integers(1, 256, (h, w, ch), dtype=np.uint8) if ch > 1 else rng.integers(1, 256, (h, w), dtype=np.uint8)


def _strided_view(img, pad):
    """The same pixels as a view into a larger buffer: rows `pad` bytes further apart than they are long."""
    h, w = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    base = np.zeros((h, w * ch + pad), np.uint8)
    base[:, :w * ch] = img.reshape(h, w * ch)
    v = np.lib.stride_tricks.as_strided(base, shape=(h, w, ch) if ch > 1 else (h, w),
                                        strides=(base.strides[0], ch, 1) if ch > 1 else (base.strides[0], 1), writeable=False)
    assert np.array_equal(v, img)
    return v, base


def _device_frame(img, offset, pad):
    """The same pixels in device memory, `offset` bytes into an allocation that ENDS with the last row's last byte."""
    import torch
    h, w = img.shape[:2]
    ch = img.shape[2] if img.ndim == 3 else 1
    stride = w * ch + pad
    buf = np.zeros(offset + (h - 1) * stride + w * ch, np.uint8)
    for y in range(h):
        buf[offset + y * stride: offset + y * stride + w * ch] = img[y].reshape(-1)
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return DeviceFrames(t.data_ptr() + offset, 1, h, w, stride, ch), t


def test_pack_frames_smallest_shapes(env, oracle):
    rng = np.random.default_rng(7)
    widths = list(range(1, 10)) + [63, 64, 65, 255, 256, 257]
    items, gray, keep = [], [], []
    for i, w in enumerate(widths):
        h, ch = (1, 2, 5)[i % 3], (1, 3, 4)[(i + i // 3) % 3]
        img = _color(rng, h, w, ch)
        gray.append(img if ch == 1 else oracle.bgr2gray(img))
        kind = i % 4
        if kind == 0:                                   # a host array whose last row ends its allocation
            items.append(np.ascontiguousarray(img))
        elif kind == 1:                                 # a host view with stride > w * ch, odd
            v, base = _strided_view(img, 7 if (w * ch) % 2 == 0 else 8)
            assert v.strides[0] % 2 == 1
            items.append(v)
            keep.append(base)
        elif kind == 2:                                 # device memory at an odd byte offset, odd stride
            d, t = _device_frame(img, 1 + 2 * (i % 2), 0 if (w * ch) % 2 else 3)
            assert d.ptr % 2 == 1 and d.stride % 2 == 1
            items.append(d)
            keep.append(t)
        else:                                           # device memory, tight rows, the allocation ends with the last row
            d, t = _device_frame(img, 0, 0)
            items.append(d)
            keep.append(t)
    assert {g.shape[0] for g in gray} == {1, 2, 5} and len({(it.channels if isinstance(it, DeviceFrames) else (it.shape[2] if it.ndim == 3 else 1))
                                                          for it in items}) == 3
    atlas, origins = env.pack_frames(items)
    assert atlas.shape[0] > 0 and np.all(origins >= 0) and np.all(origins[:, 0] % 4 == 0)
    want = np.zeros_like(atlas)                         # what no frame covers, and a slot's pad columns, are 0
    for g, (x, y) in zip(gray, origins):
        assert np.all(want[y:y + g.shape[0], x:x + g.shape[1]] == 0)   # no two frames share a pixel
        want[y:y + g.shape[0], x:x + g.shape[1]] = g
    assert np.array_equal(atlas, want)                  # every frame at its origin, and nothing anywhere else
    # the first atlas of several: frames that are not in it say so
    atlas2, origins2 = env.pack_frames(items, atlas_px=1200)
    inside = origins2[:, 0] >= 0
    assert 0 < inside.sum() < len(items) and np.all(origins2[~inside] == -1) and inside[0]
    want = np.zeros_like(atlas2)
    for g, (x, y), ok in zip(gray, origins2, inside):
        if ok:
            want[y:y + g.shape[0], x:x + g.shape[1]] = g
    assert np.array_equal(atlas2, want)


def test_pack_frames_of_the_cases(env):
    fr = mc.frames()
    atlas, origins = env.pack_frames(fr)
    assert atlas.shape == (640, 448)                    # on the ladder (tests/atlas_asan_driver.cpp plans the same list)
    want = np.zeros_like(atlas)
    for f, (x, y) in zip(fr, origins):
        want[y:y + f.shape[0], x:x + f.shape[1]] = f
    assert np.array_equal(atlas, want)
    with tunables(env, ("max_subbatch", "2")):          # frames per atlas are capped like frames per sub-batch
        _, o2 = env.pack_frames(fr)
    assert (o2[:, 0] >= 0).tolist() == [True, True] + [False] * (N - 2)


# ---------------------------------------------------------------------------------------- 2. OpenCV profile against the oracle
def _check_cv(env, oracle, name, a, r, count, **kw):
    res = mc.oracle_cv(oracle, name, a, **kw)
    windows, entered, evals = 0, np.zeros(a.n_stages, np.int64), 0
    for i, (ro, st) in enumerate(res):
        assert mc.rows(r.rects[r.rects["frame"] == i]) == mc.rows(ro), f"frame {i} {mc.SIZES[i]}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
        evals += st["stump_evals"]
    assert len(r.rects) == sum(len(ro) for ro, _ in res) >= 40
    _sorted_by_frame(r)
    if count:
        assert r.windows == windows and r.stage_entered == entered.tolist()
        if all(int(n) == 1 for n in a.tree_n_nodes):
            assert r.stump_evals == evals
        else:   # multi-node trees: the library counts every node of an entered stage, the oracle the nodes a walk visits
            nodes = [int(sum(a.tree_n_nodes[a.stage_first_tree[s]:a.stage_first_tree[s] + a.stage_n_trees[s]])) for s in range(a.n_stages)]
            assert r.stump_evals == sum(int(entered[s]) * nodes[s] for s in range(a.n_stages)) >= evals


@pytest.mark.parametrize("name", list(mc.EXPECTED))
def test_opencv_profile_matches_the_oracle(env, oracle, cascades, name):
    c, a = cascades(name)
    r = env.detect_opencv_mixed(c, mc.frames(), flags=VJ_FLAG_COUNTERS)
    _check_cv(env, oracle, name, a, r, True)
    assert [int((r.rects["frame"] == i).sum()) for i in range(N)] == mc.EXPECTED[name][0]
    info = env.mixed_info()
    assert (info.atlases, info.frames, info.frames_atlas, info.own_calls, info.frames_oversized) == (1, N, N, 0, 0)
    assert info.windows >= r.windows > 0 and (info.atlas_w, info.atlas_h) == (448, 640) and info.pack_ms > 0   # (grid positions; the walk visits fewer)
    r0 = env.detect_opencv_mixed(c, mc.frames())
    _check_cv(env, oracle, name, a, r0, False)
    assert np.array_equal(r0.rects, r.rects)


# -------------------------------------------------------------------------------------------------------------------- 3. routes
def _info(env):
    i = env.mixed_info()
    return dict(atlases=i.atlases, own_calls=i.own_calls, on_atlas=i.frames_atlas, own=i.frames_own_calls, oversized=i.frames_oversized)


@pytest.mark.parametrize("name", ["frontalface_alt", "mcs_mouth"])
def test_every_route_gives_the_same(env, oracle, cascades, name):
    c, a = cascades(name)
    fr = mc.frames()
    base = env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS)
    _check_cv(env, oracle, name, a, base, True)

    def same(r):
        assert np.array_equal(r.rects, base.rects)
        assert (r.windows, r.stage_entered, r.stump_evals) == (base.windows, base.stage_entered, base.stump_evals)

    # three atlases, and the two 240 x 180 frames too large for an empty one: they share one batched call
    same(env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS, atlas_px=42000, own_call_px=NEVER))
    assert _info(env) == dict(atlases=3, own_calls=1, on_atlas=N - 2, own=0, oversized=2)
    # the two equal frames reach the rule's pixel count: a batched call of their own
    same(env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS, own_call_px=2 * 240 * 180))
    assert _info(env) == dict(atlases=1, own_calls=1, on_atlas=N - 2, own=2, oversized=0)
    # everything per group
    same(env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS, own_call_px=1))
    assert _info(env) == dict(atlases=0, own_calls=N - 1, on_atlas=0, own=N, oversized=0)
    # frames per atlas capped
    with tunables(env, ("max_subbatch", "2")):
        same(env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS))
        assert _info(env) == dict(atlases=(N + 1) // 2, own_calls=0, on_atlas=N, own=0, oversized=0)


# --------------------------------------------------------------------------------------------------------------- 4. mixed input
def _mixed_inputs(oracle):
    """The eleven frames as gray / BGR / BGRA, host / strided host / device-resident -> (items of one call, the same frame by frame with
    the color argument of a per-frame call, their gray images, what must stay alive)."""
    items, gray, keep = [], [], []
    for i, f in enumerate(mc.frames()):
        ch = (1, 3, 4)[i % 3]
        img = f
        if ch > 1:
            img = np.repeat(f[..., None], ch, axis=2)
            img[..., 1] = f[::-1]
            img[..., 2] = f[:, ::-1]
        gray.append(f if ch == 1 else oracle.bgr2gray(img))
        where = (i // 3) % 3
        if where == 0:
            items.append(np.ascontiguousarray(img))
        elif where == 1:
            v, base = _strided_view(img, 13)
            items.append(v)
            keep.append(base)
        else:
            d, t = _device_frame(img, 3, 5)
            items.append(d)
            keep.append(t)
    kinds = {((it.channels if isinstance(it, DeviceFrames) else (it.shape[2] if it.ndim == 3 else 1)), isinstance(it, DeviceFrames)) for it in items}
    assert len(kinds) == 6                              # every channel count both on the host and on the device
    return items, gray, keep


def _per_frame_cv(env, c, items, **kw):
    """What a caller had before: one detect_opencv call per frame."""
    return [env.detect_opencv(c, it, color=(it.channels if isinstance(it, DeviceFrames) else it.ndim == 3 and it.shape[2]) > 1, **kw)
            for it in items]


@pytest.mark.parametrize("name", ["frontalface_alt", "mcs_mouth"])
def test_gray_bgr_bgra_host_and_device_frames_in_one_call(env, oracle, cascades, name):
    c, a = cascades(name)
    items, gray, keep = _mixed_inputs(oracle)
    res = [oracle.detect_opencvlike(a, np.ascontiguousarray(g)) for g in gray]
    for mn in (0, 3):
        r = env.detect_opencv_mixed(c, items, min_neighbors=mn)
        assert _info(env)["atlases"] == 1 and _info(env)["on_atlas"] == N
        assert _same_as_per_frame(r, _per_frame_cv(env, c, items, min_neighbors=mn)) >= 3
        if mn == 0:
            for i, (ro, _) in enumerate(res):
                assert mc.rows(r.rects[r.rects["frame"] == i]) == mc.rows(ro), f"frame {i}"
            assert len(r.rects) >= 40
        else:
            _grouped_like_the_oracle(oracle, r, res, mn)


# --------------------------------------------------------------------------------------------------------------------- 5. flags
@pytest.mark.parametrize("flags,mn,atlases", [(VJ_FLAG_CV_SCALE_IMAGE, 0, 1), (VJ_FLAG_CV_SCALE_IMAGE | VJ_FLAG_COUNTERS, 3, 1),
                                              (VJ_FLAG_CV_CANNY_PRUNING | VJ_FLAG_COUNTERS, 0, 0),
                                              (VJ_FLAG_CV_FIND_BIGGEST | VJ_FLAG_CV_ROUGH_SEARCH, 2, 0)])
def test_flags_equal_per_frame_calls(env, cascades, flags, mn, atlases):
    c, a = cascades("frontalface_alt")
    fr = mc.frames()
    r = env.detect_opencv_mixed(c, fr, flags=flags, min_neighbors=mn)
    assert _info(env)["atlases"] == atlases and _info(env)["on_atlas"] == (N if atlases else 0)
    parts = _per_frame_cv(env, c, fr, flags=flags, min_neighbors=mn)
    assert _same_as_per_frame(r, parts) >= 3
    if flags & VJ_FLAG_COUNTERS:
        _same_counters(r, parts)


# -------------------------------------------------------------------------------------------------------------- 6. clod profile
def _check_clod(oracle, name, a, r, **kw):
    res = mc.oracle_clod(oracle, name, a, **kw)
    for i, (ro, _) in enumerate(res):
        assert mc.rows(r.rects[r.rects["frame"] == i]) == mc.rows(ro), f"frame {i} {mc.SIZES[i]}"
    assert len(r.rects) == sum(len(ro) for ro, _ in res) >= 40
    _sorted_by_frame(r)
    return res


def _per_frame_clod(env, c, fr, p):
    return [env.detect(c, f, p) for f in fr]


@pytest.mark.parametrize("name", ["frontalface_alt", "frontalface_alt2", "frontalface_alt_tree"])
def test_clod_profile_matches_the_oracle(env, oracle, cascades, name):
    c, a = cascades(name)
    fr = mc.frames()
    p = default_params(flags=VJ_FLAG_COUNTERS)
    r = env.detect_mixed(c, fr, p)
    res = _check_clod(oracle, name, a, r)
    assert [int((r.rects["frame"] == i).sum()) for i in range(N)] == mc.EXPECTED[name][1]
    info = env.mixed_info()
    assert (info.atlases, info.frames_atlas, info.own_calls) == (1, N, 0) and info.windows == r.windows
    assert r.windows == sum(st["windows"] for _, st in res)
    parts = _per_frame_clod(env, c, fr, p)
    _same_as_per_frame(r, parts)
    _same_counters(r, parts)
    r0 = env.detect_mixed(c, fr)
    assert np.array_equal(r0.rects, r.rects)
    for kw in (dict(atlas_px=42000, own_call_px=NEVER), dict(own_call_px=2 * 240 * 180), dict(own_call_px=1)):   # the routes
        rr = env.detect_mixed(c, fr, p, **kw)
        assert np.array_equal(rr.rects, r.rects) and (rr.windows, rr.stage_entered, rr.stump_evals) == (r.windows, r.stage_entered, r.stump_evals)
    assert _info(env) == dict(atlases=0, own_calls=N - 1, on_atlas=0, own=N, oversized=0)


def test_clod_profile_flags_and_parameters(env, oracle, cascades):
    fr = mc.frames()
    c, a = cascades("frontalface_alt")
    # grouped, every frame on its own
    p = default_params(min_neighbors=3)
    r = env.detect_mixed(c, fr, p)
    assert _same_as_per_frame(r, _per_frame_clod(env, c, fr, p)) >= 3
    _grouped_like_the_oracle(oracle, r, mc.oracle_clod(oracle, "frontalface_alt", a), 3)
    # the reference's signed read of the window sum
    p = default_params(flags=VJ_FLAG_SIGNED_MEAN)
    _check_clod(oracle, "frontalface_alt", a, env.detect_mixed(c, fr, p), signed_mean=True)
    # a scale mask selects scales by their index in the frame's own enumeration
    scales = [0, 2, 3, 5, 8]
    p = default_params(scales=scales)
    r = env.detect_mixed(c, fr, p)
    assert _same_as_per_frame(r, _per_frame_clod(env, c, fr, p)) >= 10
    for i, (ro, _) in enumerate(mc.oracle_clod(oracle, "frontalface_alt", a)):
        assert mc.rows(r.rects[r.rects["frame"] == i]) == mc.rows(ro[np.isin(ro["scale_idx"], scales)]), f"frame {i}"
    # a skip mode walks the image's own window list: per group, no atlas
    p = default_params(flags=VJ_FLAG_SKIP_ROW | VJ_FLAG_COUNTERS)
    r = env.detect_mixed(c, fr, p)
    assert _info(env) == dict(atlases=0, own_calls=N - 1, on_atlas=0, own=N, oversized=0)
    parts = _per_frame_clod(env, c, fr, p)
    assert _same_as_per_frame(r, parts) >= 40
    _same_counters(r, parts)
    # tilted features as upright ones, as the reference evaluates them
    c, a = cascades("mcs_mouth")
    p = default_params(flags=VJ_FLAG_TILTED_AS_UPRIGHT)
    r = env.detect_mixed(c, fr, p)
    assert _info(env)["atlases"] == 1
    assert _same_as_per_frame(r, _per_frame_clod(env, c, fr, p)) >= 10
    with pytest.raises(VjError) as ei:                  # without the flag the cascade is refused, as everywhere
        env.detect_mixed(c, fr)
    assert ei.value.code == 4


# --------------------------------------------------------------------------------------------------- 7. uniform batch and errors
def test_uniform_batch_returns_what_the_batched_calls_return(env, cascades):
    c, a = cascades("frontalface_alt")
    fr = [mc.cc.faces_frame(s, 97, 131, n_faces=3) for s in (2, 21, 22)]
    want = env.detect_opencv(c, np.stack(fr), flags=VJ_FLAG_COUNTERS)
    for kw in ({}, dict(own_call_px=1)):                # on the atlas, and through the batched call itself
        r = env.detect_opencv_mixed(c, fr, flags=VJ_FLAG_COUNTERS, **kw)
        assert _info(env)["atlases"] == (0 if kw else 1)
        assert np.array_equal(r.rects, want.rects) and len(r.rects) >= 10
        assert (r.windows, r.stage_entered, r.stump_evals, r.gather_bytes) == (want.windows, want.stage_entered, want.stump_evals, want.gather_bytes)
    p = default_params(flags=VJ_FLAG_COUNTERS)
    want = env.detect(c, np.stack(fr), p)
    for kw in ({}, dict(own_call_px=1)):
        r = env.detect_mixed(c, fr, p, **kw)
        assert _info(env)["atlases"] == (0 if kw else 1)
        assert np.array_equal(r.rects, want.rects) and len(r.rects) >= 10
        assert (r.windows, r.stage_entered, r.stump_evals, r.gather_bytes) == (want.windows, want.stage_entered, want.stump_evals, want.gather_bytes)


def test_argument_handling(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    fr = mc.frames()
    # no frames: VJ_OK, nothing
    r = env.detect_opencv_mixed(c, [], flags=VJ_FLAG_COUNTERS)
    assert len(r.rects) == 0 and r.windows == 0 and env.mixed_info().frames == 0
    assert len(env.detect_mixed(c, []).rects) == 0
    atlas, origins = env.pack_frames([])
    assert atlas.size == 0 and len(origins) == 0
    # only frames too small for any scale
    r = env.detect_opencv_mixed(c, [fr[i] for i in mc.TINY], flags=VJ_FLAG_COUNTERS)
    assert len(r.rects) == 0 and r.windows == 0
    assert len(env.detect_mixed(c, [fr[i] for i in mc.TINY]).rects) == 0
    # a bad frame is VJ_ERR_ARG and is named
    good, keep = env._one_image(fr[1])
    p, cp, res, opts = Params(), CvParams(0, 0, 1.1, 0, 0), _Result(), MixedOpts(0, 0)
    lib.vj_params_default(C.byref(p))
    w, h, org = C.c_int(0), C.c_int(0), (C.c_int32 * 6)()
    for bad in (_Image(None, 40, 40, 40, 0, 1), _Image(good.data, 0, 40, 40, 0, 1), _Image(good.data, 40, -2, 40, 0, 1),
                _Image(good.data, 40, 40, 39, 0, 1), _Image(good.data, 40, 40, 119, 0, 3), _Image(good.data, 40, 40, 80, 0, 2)):
        imgs = (_Image * 3)(good, good, bad)
        assert lib.vj_detect_opencv_mixed(env._h, c._h, imgs, 3, C.byref(cp), C.byref(opts), C.byref(res)) == 1
        assert b"frame 2" in lib.vj_last_error() and res.count == 0
        assert lib.vj_detect_mixed(env._h, c._h, imgs, 3, C.byref(p), None, C.byref(res)) == 1
        assert b"frame 2" in lib.vj_last_error()
        assert lib.vj_pack_frames(env._h, imgs, 3, 0, None, 0, C.byref(w), C.byref(h), org) == 1
        assert b"frame 2" in lib.vj_last_error()
    with pytest.raises(VjError) as ei:
        env.detect_opencv_mixed(c, fr, scale_factor=1.0)
    assert ei.value.code == 1
    # null arguments; the options may be null
    imgs = (_Image * 1)(good)
    assert lib.vj_detect_opencv_mixed(None, c._h, imgs, 1, C.byref(cp), None, C.byref(res)) == 1
    assert lib.vj_detect_opencv_mixed(env._h, c._h, None, 1, C.byref(cp), None, C.byref(res)) == 1
    assert lib.vj_detect_opencv_mixed(env._h, c._h, None, 0, C.byref(cp), None, C.byref(res)) == 0 and res.count == 0
    assert lib.vj_detect_mixed(env._h, c._h, imgs, 1, None, None, C.byref(res)) == 1
    assert lib.vj_detect_mixed(env._h, c._h, None, 0, C.byref(p), None, C.byref(res)) == 0 and res.count == 0
    assert lib.vj_mixed_info_get(env._h, None) == 1 and lib.vj_mixed_info_get(None, C.byref(MixedInfo())) == 1
    assert lib.vj_pack_frames(env._h, imgs, 1, 0, None, 0, None, C.byref(h), org) == 1
    small = np.zeros((4, 4), np.uint8)                  # an atlas buffer narrower than the atlas
    assert lib.vj_pack_frames(env._h, imgs, 1, 0, small.ctypes.data, 4, C.byref(w), C.byref(h), org) == 1
    assert lib.vj_detect_opencv_mixed(env._h, c._h, imgs, 1, C.byref(cp), None, C.byref(res)) == 0
    lib.vj_result_free(C.byref(res))
