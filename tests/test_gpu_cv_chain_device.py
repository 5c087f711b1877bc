"""vj_detect_opencv_chain with VJ_FLAG_CV_CHAIN_DEVICE on the device: the first cascade's rectangles become the second one's regions
and units without leaving the device, and everything the call returns — both rectangle lists, their order, the counters — is what
the call without the flag returns, what the two public calls return, and what the oracle computes region for region.
vj_cv_chain_info tells which way a call went and what its region pass walked: the units and windows the device counted are those the
host formula (cv_roi_build_units) gives on the unflagged route.  Cases: tests/cv_rois_cases.py (CHAIN_CASES) and
tests/cv_chain_device_cases.py, premises in tests/test_cv_chain_device_cpu.py."""
import numpy as np
import pytest

import cv_chain_device_cases as dc
import cv_rois_cases as cc
from cases import tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_CHAIN_DEVICE, VJ_FLAG_CV_SCALE_IMAGE, DeviceFrames

pytestmark = pytest.mark.gpu

DEV = VJ_FLAG_CV_CHAIN_DEVICE
COUNT = VJ_FLAG_COUNTERS


def _chain(env, c1, c2, frames, device, flags=0, **kw):
    """-> (first, second, info) of one chain call, flagged or not."""
    r1, r2 = env.detect_opencv_chain(c1, c2, frames, flags=flags | (DEV if device else 0), **kw)
    return r1, r2, env.cv_chain_info()


def _same(x, y, counted=False):
    assert np.array_equal(x.rects, y.rects)
    if counted:
        assert x.windows == y.windows and x.stage_entered == y.stage_entered and x.stump_evals == y.stump_evals
        assert x.gather_bytes == y.gather_bytes


def _same_geometry(i, j):
    assert (i.regions, i.units, i.windows) == (j.regions, j.units, j.windows)
    assert i.sub_batches == j.sub_batches


def _regions_of(r1):
    return np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)


def _both(env, c1, c2, frames, counted=True, device_sub_batches=None, **kw):
    """Flagged and unflagged, compared: rectangles, counters, geometry; the flagged call went over the device.  -> flagged results"""
    extra = dict(flags=COUNT, flags_second=COUNT) if counted else {}
    d1, d2, di = _chain(env, c1, c2, frames, True, **extra, **kw)
    h1, h2, hi = _chain(env, c1, c2, frames, False, **extra, **kw)
    _same(d1, h1, counted)
    _same(d2, h2, counted)
    assert hi.handoff == 2 and hi.sub_batches_device == 0 and hi.reruns == 0 and hi.handoff_ms == 0.0
    assert di.handoff == 1
    assert di.sub_batches_device == (di.sub_batches if device_sub_batches is None else device_sub_batches)
    _same_geometry(di, hi)
    assert di.regions == len(d1.rects)
    return d1, d2, di


@pytest.mark.parametrize("name", list(cc.CHAIN_CASES))
def test_chain_cases(env, oracle, cascades, name):
    first, second, seeds, mn = cc.CHAIN_CASES[name]
    c1, a1 = cascades(first)
    c2, a2 = cascades(second)
    frames = cc.chain_frames(name)
    r1, r2, info = _both(env, c1, c2, frames, min_neighbors=mn)
    assert info.sub_batches == 1 and info.units > 0 and info.windows > info.units and info.handoff_ms > 0.0
    base = env.detect_opencv(c1, frames, min_neighbors=mn, flags=COUNT)                           # out_first is detect_opencv's
    _same(r1, base, True)
    regions = _regions_of(r1)
    want = env.detect_opencv_rois(c2, frames, regions, flags=COUNT)                               # out_second is detect_opencv_rois' on them
    _same(r2, want, True)
    o_regions, o_res = cc.oracle_chain(oracle, a1, a2, frames, mn)                                # and both are the oracle's
    assert np.array_equal(regions, o_regions) and len(regions) >= 5
    for i, (ro, _) in enumerate(o_res):
        assert cc.rows(r2.rects[r2.rects["frame"] == i]) == cc.rows(ro), f"region {i}"
    assert r2.windows == sum(st["windows"] for _, st in o_res) <= info.windows     # (visited: a reject skips the next grid position)
    assert r2.stage_entered[:a2.n_stages] == np.sum([st["stage_entered"] for _, st in o_res], axis=0).tolist()
    assert len(r2.rects) == sum(len(ro) for ro, _ in o_res) >= 3
    with tunables(env, ("max_subbatch", "1")):                                                    # sub-batches: the same
        s1, s2, si = _chain(env, c1, c2, frames, True, min_neighbors=mn)
    _same(s1, r1)
    _same(s2, r2)
    assert si.handoff == 1 and si.sub_batches == si.sub_batches_device == len(frames)
    assert (si.regions, si.units, si.windows) == (info.regions, info.units, info.windows)
    g1, g2, gi = _chain(env, c1, c2, frames, True, min_neighbors=mn, min_neighbors_second=2)     # the second cascade grouped per region
    _same(g1, r1)
    _same(g2, env.detect_opencv_rois(c2, frames, regions, min_neighbors=2))
    assert gi.handoff == 1 and gi.sub_batches_device == 1


def test_stage_tree_as_second_cascade(env, oracle, cascades):
    first, second, seeds, mn = dc.TREE_CASE
    c1, a1 = cascades(first)
    c2, a2 = cascades(second)
    frames = dc.tree_frames()
    r1, r2, info = _both(env, c1, c2, frames, min_neighbors=mn)
    o_regions, o_res = cc.oracle_chain(oracle, a1, a2, frames, mn)
    assert np.array_equal(_regions_of(r1), o_regions) and len(o_regions) == 9
    for i, (ro, _) in enumerate(o_res):
        assert cc.rows(r2.rects[r2.rects["frame"] == i]) == cc.rows(ro), f"region {i}"
    assert len(r2.rects) == 15 and r2.stage_entered[a2.n_stages - 1] >= 1
    assert r2.stage_entered[:a2.n_stages] == np.sum([st["stage_entered"] for _, st in o_res], axis=0).tolist()
    _both(env, c1, c2, frames, counted=False, min_neighbors=mn)                                   # uncounted: the same rectangles
    with tunables(env, ("max_subbatch", "1")):
        s1, s2, _ = _both(env, c1, c2, frames, min_neighbors=mn)
    _same(s1, r1, True)
    _same(s2, r2, True)


@pytest.mark.parametrize("mn", [0, 3])
def test_frames_that_give_nothing(env, oracle, cascades, mn):
    c1, a1 = cascades(dc.NOTHING_CASE[0])
    c2, a2 = cascades(dc.NOTHING_CASE[1])
    frames = dc.nothing_frames()
    r1, r2, info = _both(env, c1, c2, frames, min_neighbors=mn)
    per_frame = [int(np.sum(r1.rects["frame"] == f)) for f in range(4)]
    assert per_frame[1] == 0 and per_frame[2] == (0 if mn else 1) and per_frame[0] > 0 and per_frame[3] > 0
    assert len(r2.rects) >= 10
    if mn:                                                                                        # (the raw twin of this: test_chain_cases)
        o_regions, o_res = cc.oracle_chain(oracle, a1, a2, frames, mn)
        assert np.array_equal(_regions_of(r1), o_regions)
        for i, (ro, _) in enumerate(o_res):
            assert cc.rows(r2.rects[r2.rects["frame"] == i]) == cc.rows(ro), f"region {i}"
    with tunables(env, ("max_subbatch", "1")):                                                    # a sub-batch with no region at all
        s1, s2, si = _both(env, c1, c2, frames, min_neighbors=mn)
    _same(s1, r1, True)
    _same(s2, r2, True)
    assert si.sub_batches == 4 and (si.regions, si.units, si.windows) == (info.regions, info.units, info.windows)
    e1, e2, ei = _both(env, c1, c2, frames[1:2], min_neighbors=mn)                                # and a call with none
    assert len(e1.rects) == 0 and len(e2.rects) == 0 and ei.regions == 0 and ei.units == 0 and e2.windows == 0


def test_group_max_sends_a_sub_batch_through_the_host(env, cascades):
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = dc.group_max_frames()
    with tunables(env, ("group_max", "100"), ("max_subbatch", "1")):
        r1, r2, info = _both(env, c1, c2, frames, device_sub_batches=1, min_neighbors=3)          # 97 / 120 / 185 raw candidates
    assert info.sub_batches == 3 and len(r2.rects) >= 10
    with tunables(env, ("group_max", "96"), ("max_subbatch", "1")):
        s1, s2, si = _both(env, c1, c2, frames, device_sub_batches=0, min_neighbors=3)
    _same(s1, r1, True)
    _same(s2, r2, True)
    with tunables(env, ("group_max", "100")):                                                     # one sub-batch of three frames: all of it
        t1, t2, ti = _both(env, c1, c2, frames, device_sub_batches=0, min_neighbors=3)
    _same(t1, r1, True)
    _same(t2, r2, True)
    w1, w2, wi = _both(env, c1, c2, frames, min_neighbors=3)                                      # the default groups them all on the device
    _same(w1, r1, True)
    _same(w2, r2, True)
    with tunables(env, ("group_max", "100")):                                                     # raw candidates are not grouped: no limit
        _both(env, c1, c2, frames[1:2], min_neighbors=0)


@pytest.mark.parametrize("mn,seeds", [(0, [2]), (3, [2, 5])])
def test_every_buffer_regrows(env, cascades, mn, seeds):
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = np.stack([dc.faces(s) for s in seeds])
    h1, h2, hi = _chain(env, c1, c2, frames, False, flags=COUNT, flags_second=COUNT, min_neighbors=mn)
    assert len(h1.rects) > 4 and hi.units > 4 and len(h2.rects) > 1                              # every buffer of "det_cap 1" is short
    with tunables(env, ("det_cap", "1")):
        d1, d2, di = _chain(env, c1, c2, frames, True, flags=COUNT, flags_second=COUNT, min_neighbors=mn)
        assert di.handoff == 1 and di.reruns >= 3 and di.sub_batches_device == di.sub_batches == 1
        e1, e2, ei = _chain(env, c1, c2, frames, True, flags=COUNT, flags_second=COUNT, min_neighbors=mn)   # grown buffers are capacities of
        assert ei.reruns >= 1                                                                     # the call, not of the environment
    _same(d1, h1, True)
    _same(d2, h2, True)
    _same(e1, h1, True)
    _same(e2, h2, True)
    _same_geometry(di, hi)
    r1, r2, ri = _chain(env, c1, c2, frames, True, flags=COUNT, flags_second=COUNT, min_neighbors=mn)       # back at the defaults
    assert ri.reruns == 0
    _same(r1, h1, True)
    _same(r2, h2, True)


def test_min_size_and_scale_factor_of_the_second_cascade(env, cascades):
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = cc.chain_frames("alt2_lefteye_grouped")
    kw = dict(min_neighbors=3, min_size_second=(30, 20), scale_factor_second=1.25)
    r1, r2, info = _both(env, c1, c2, frames, **kw)
    assert len(r2.rects) >= 3 and np.all(r2.rects["w"] >= 30) and np.all(r2.rects["h"] >= 20)
    want = env.detect_opencv_rois(c2, frames, _regions_of(r1), min_size=(30, 20), scale_factor=1.25, flags=COUNT)
    _same(r2, want, True)
    p1, p2, pinfo = _both(env, c1, c2, frames, min_neighbors=3)                                    # other factors, skipped slots: other units
    assert pinfo.units > info.units and pinfo.regions == info.regions
    _both(env, c1, c2, frames[:1], min_neighbors=0, min_size_second=(30, 20), scale_factor_second=1.25)


def test_bgr_and_device_frames(env, cascades):
    import torch
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = cc.chain_frames("alt2_lefteye_grouped")
    gray1, gray2, _ = _both(env, c1, c2, frames, min_neighbors=3)
    bgr = np.repeat(frames[..., None], 3, axis=3)
    bgr[..., 1] = frames[:, ::-1]
    bgr[..., 2] = frames[:, :, ::-1]
    b1, b2, _ = _both(env, c1, c2, list(bgr), min_neighbors=3, color=True)
    assert len(b1.rects) >= 1
    n, h, w = frames.shape                                                                        # DeviceFrames, row stride above the width
    stride = w + 40
    t = torch.zeros((n, h, stride), dtype=torch.uint8).cuda()
    t[:, :, :w] = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    dev = DeviceFrames(t.data_ptr(), n, h, w, stride, 1)
    for mn in (0, 3):
        d1, d2, _ = _both(env, c1, c2, dev, min_neighbors=mn)
    _same(d1, gray1, True)
    _same(d2, gray2, True)


def test_tilted_integral_for_the_second_cascade_alone(env, cascades):
    """need_tilted: frontalface_alt2 reads no tilted integral, mcs_mouth does — on raw candidates too (the grouped twin: CHAIN_CASES)."""
    c1, a1 = cascades("frontalface_alt2")
    c2, a2 = cascades("mcs_mouth")
    assert not any(a1.node_tilted) and any(a2.node_tilted)
    r1, r2, _ = _both(env, c1, c2, cc.chain_frames("alt2_tilted_grouped")[:1], min_neighbors=0)
    assert len(r2.rects) >= 3


def test_flag_combinations(env, cascades):
    c1, _ = cascades("frontalface_alt2")
    c2, _ = cascades("mcs_lefteye")
    frames = cc.chain_frames("alt2_lefteye_grouped")
    h1, h2, _ = _chain(env, c1, c2, frames, False, min_neighbors=3, flags_second=VJ_FLAG_CV_SCALE_IMAGE)
    f1, f2, fi = _chain(env, c1, c2, frames, True, min_neighbors=3, flags_second=VJ_FLAG_CV_SCALE_IMAGE)   # the two public calls
    assert fi.handoff == 3 and fi.sub_batches_device == 0 and fi.regions == len(f1.rects)
    _same(f1, h1)
    _same(f2, h2)
    s1, s2, si = _chain(env, c1, c2, frames, True, flags=VJ_FLAG_CV_SCALE_IMAGE, min_neighbors=3)
    assert si.handoff == 3
    _same(s1, env.detect_opencv(c1, frames, min_neighbors=3, flags=VJ_FLAG_CV_SCALE_IMAGE))
    d1, d2, di = _chain(env, c1, c2, frames, False, min_neighbors=3, flags_second=DEV)            # only the first word is read for the bit
    assert di.handoff == 2
    _same(d1, h1)
    # the other entry points ignore the bit
    base = env.detect_opencv(c1, frames, min_neighbors=3, flags=COUNT)
    _same(env.detect_opencv(c1, frames, min_neighbors=3, flags=COUNT | DEV), base, True)
    assert env.cv_plan_info(c1, 640, 360, 2, flags=DEV).tile_windows == env.cv_plan_info(c1, 640, 360, 2).tile_windows
    regions = _regions_of(base)
    want = env.detect_opencv_rois(c2, frames, regions, flags=COUNT)
    _same(env.detect_opencv_rois(c2, frames, regions, flags=COUNT | DEV), want, True)
    _same(d2, env.detect_opencv_rois(c2, frames, regions))
    assert env.cv_chain_info().handoff == 2                                                       # the record is the last CHAIN call's
