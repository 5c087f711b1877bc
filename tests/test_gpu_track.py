"""vj_track on the device: every case of tests/track_cases.py through Environment.track against the numpy
restatement, field by field — host arrays, device frames and the two mixed in one call, at padded strides and every address mod 4,
whole and with max_subbatch at 1 and 2 —, scratch reuse across calls of differing t and r, no rows, every argument error followed
by a call that still matches, bridge_detections on the device against its CPU run with the restatement, and end to end around the
detector and paint().  The premises (the cases tell the wrong readings of the definition apart) are checked on the CPU in
tests/test_track_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import paint_cases as pcs
import prep_cases as pc
import track_cases as tc
from cases import tunables
from clfacedetection_amd import TRACK_RESULT_DTYPE, DeviceFrames, TrackParams, VjError, bridge_detections
from clfacedetection_amd.api import _Image
from test_gpu_paint import Frame

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8


def kinds(sources, variant=0):
    """The frames as host views, as device frames and the two mixed, at addresses 0 .. 3 mod 4 and with padded strides."""
    n = len(sources)
    return {"host": [Frame(s, "host", (i + variant) % 4, (3 * i + variant) % 5) for i, s in enumerate(sources)],
            "dev": [Frame(s, "dev", (i + 1 + variant) % 4, (i + 2 * variant) % 4) for i, s in enumerate(sources)],
            "mixed": [Frame(s, "dev" if (i + variant) % 2 else "host", (i + 2) % 4, (i + variant) % 3) for i, s in enumerate(sources)] if n > 1 else []}


def check(env, oracle, name, sources, rows, t, r, scale=(1.0, 1.0), subs=(None, "1", "2"), variant=0):
    want = pc.once(("track", name, t, r), lambda: tc.restate(oracle, sources, rows, t, r, scale))
    for kind, frames in kinds(sources, variant).items():
        if not frames:
            continue
        for sub in subs:
            with tunables(env, *((("max_subbatch", sub),) if sub else ())):
                got = env.track([f.item for f in frames], rows, tmpl=t, radius=r, scale=scale)
            assert got.dtype == TRACK_RESULT_DTYPE
            if not tc.equal(got, want):
                bad = [k for k in range(len(want)) if any(int(got[f][k]) != int(want[f][k]) for f in tc.RESULT_FIELDS)]
                raise AssertionError((name, kind, sub, "rows", bad[:5], "got", got[bad[0]], "want", want[bad[0]]))
        for f in frames:
            assert np.array_equal(f.now(), f.before), "track() wrote into a frame"
    return want


# ------------------------------------------------------------------------------------------------------------------- 1. the cases
def test_the_known_shift(env, oracle):
    rows = tc.both_ways([tc.SHIFT_BOX]) + [(1, 1) + tc.SHIFT_BOX]
    want = check(env, oracle, "shift", tc.shift_pair(), rows, *tc.SHIFT_TR)
    assert (want["dx"][0], want["dy"][0], want["sad"][0], want["sad0"][0]) == (3, -2, 0, tc.SHIFT_SAD0)


def test_scaled(env, oracle):
    want = check(env, oracle, "scaled", tc.scaled_pair(), tc.both_ways([tc.SCALED_BOX]), *tc.SCALED_TR)
    assert (want["dx"][0], want["dy"][0]) == (2, -1)


def test_ties_and_the_accumulator(env, oracle):
    flat = [tc.flat_frame(), tc.flat_frame(78)]
    want = check(env, oracle, "flat", flat, [(0, 0, 10, 10, 30, 20), (0, 1, 10, 10, 30, 20), (1, 0, -5, 30, 40, 40)], 32, 8)
    assert all((m["dx"], m["dy"]) == (0, 0) for m in want)
    want = check(env, oracle, "period4", tc.period4_pair(), tc.both_ways([tc.PERIOD4_BOX]), *tc.PERIOD4_TR)
    assert (want["dx"][0], want["dy"][0], want["sad"][0]) == (-2, 0, 0)
    want = check(env, oracle, "acc", tc.acc_pair(), tc.both_ways([tc.ACC_BOX]), *tc.ACC_TR)
    assert all((m["dx"], m["dy"], m["sad"], m["sad0"]) == (0, 0, tc.ACC_SAD, tc.ACC_SAD) for m in want)


def test_boxes_partly_and_wholly_outside_their_frames(env, oracle):
    check(env, oracle, "outside", tc.shift_pair(), tc.both_ways(tc.OUTSIDE_BOXES), *tc.SHIFT_TR, variant=1)


@pytest.mark.parametrize("t,r", tc.TR_PAIRS)
def test_the_ends_of_t_and_r(env, oracle, t, r):
    check(env, oracle, "tr", tc.shift_pair(), tc.both_ways(tc.TR_BOXES), t, r, variant=t % 3)


def test_the_batch(env, oracle):
    res = check(env, oracle, "batch", tc.batch_frames(), tc.batch_rows(), *tc.BATCH_TR, tc.BATCH_SCALE)
    assert len(res) == 70
    ms, match = env.track_timing()
    assert ms > 0 and 0 < match <= ms


# ------------------------------------------------------------------------------------------------ 2. call shapes, scratch reuse
def test_a_second_call_with_other_t_and_r_reuses_the_scratch(env, oracle):
    src = tc.shift_pair()
    rows = tc.both_ways(tc.TR_BOXES)
    for t, r in [(64, 16), (8, 1), (36, 7), (64, 16), (12, 3)]:               # larger, smaller, larger again on one environment
        want = pc.once(("track", "tr", t, r), lambda: tc.restate(oracle, src, rows, t, r))
        assert tc.equal(env.track(list(src), rows, tmpl=t, radius=r), want), (t, r)


def test_no_rows_arrays_and_tensors(env, oracle):
    import torch
    src = tc.shift_pair()
    got = env.track(list(src), np.zeros((0, 6), np.int32))
    assert got.dtype == TRACK_RESULT_DTYPE and len(got) == 0
    rows = tc.both_ways([tc.SHIFT_BOX])
    want = pc.once(("track", "pair", 24, 5), lambda: tc.restate(oracle, src, rows, *tc.SHIFT_TR))
    batch = np.stack(src)
    assert tc.equal(env.track(batch, rows, tmpl=24, radius=5), want)                         # a batch as one array
    assert tc.equal(env.track(torch.from_numpy(batch).cuda(), rows, tmpl=24, radius=5), want)   # as one CUDA tensor
    bgr = np.stack([np.stack([f, f, f], axis=-1) for f in src])                            # B = G = R = g: the gray value is g
    assert tc.equal(env.track(bgr, rows, tmpl=24, radius=5, color=True), want)
    with pytest.raises(ValueError):
        env.track(list(src), np.zeros((1, 6)))
    with pytest.raises(ValueError):
        env.track([src[0].astype(np.int16)], rows)


# -------------------------------------------------------------------------------------------------------------- 3. the error cases
def test_argument_errors_leave_the_environment_as_it_was(env, lib, oracle):
    import torch
    src = tc.shift_pair()
    dev = torch.from_numpy(np.array(src[0])).cuda()
    torch.cuda.synchronize()
    host = np.array(src[1])
    h, w = host.shape
    ok = [_Image(dev.data_ptr(), w, h, w, 1, 1), _Image(host.ctypes.data, w, h, host.strides[0], 0, 1)]
    good = tc.both_ways([tc.SHIFT_BOX])
    want = pc.once(("track", "pair", 24, 5), lambda: tc.restate(oracle, src, good, *tc.SHIFT_TR))
    f = lib.vj_track

    def call(images=ok, n=None, rows=good, nr=None, p=True, e=env._h, out=True, **kw):
        q = TrackParams()
        lib.vj_track_default(C.byref(q))
        q.tmpl, q.radius = tc.SHIFT_TR
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images) if images is not None else None
        r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 6)) if rows is not None else None
        m = len(r) if r is not None else 2
        res = np.zeros(max(m, 1), TRACK_RESULT_DTYPE)
        rc = f(e, arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if r is not None else None,
               m if nr is None else nr, C.byref(q) if p else None, res.ctypes.data if out else None)
        err = lib.vj_last_error().decode()
        if rc != 0:                                                               # ... and a track still matches
            assert not res.view(np.uint8).any()
            assert tc.equal(env.track([dev[None], host], good, tmpl=tc.SHIFT_TR[0], radius=tc.SHIFT_TR[1]), want)
        return rc, err, res[:m]

    rc, err, res = call()
    assert rc == 0 and tc.equal(res, want), err
    for kw in (dict(e=None), dict(images=None), dict(rows=None), dict(p=False), dict(out=False), dict(n=-1), dict(nr=-1)):
        assert call(**kw)[0] == VJ_ERR_ARG, kw
    for bad in (_Image(None, 8, 4, 8, 1, 1), _Image(dev.data_ptr(), 0, 4, 8, 1, 1), _Image(dev.data_ptr(), 8, 4, 7, 1, 1), _Image(dev.data_ptr(), 8, 4, 16, 1, 2)):
        rc, err, _ = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err
    for bad, word in [((2, 0, 0, 0, 4, 4), "src_frame"), ((0, -1, 0, 0, 4, 4), "dst_frame"), ((0, 1, 0, 0, 0, 4), "region 2"), ((1, 0, 0, 0, 4, -1), "region 2")]:
        rc, err, _ = call(rows=good + [bad])
        assert rc == VJ_ERR_ARG and word in err and " 2" in err, bad
    for kw, word in [(dict(tmpl=4), "tmpl"), (dict(tmpl=68), "tmpl"), (dict(tmpl=30), "tmpl"), (dict(radius=0), "radius"), (dict(radius=17), "radius"),
                     (dict(flags=1), "flags"), (dict(reserved=7), "reserved"), (dict(sx=-1.0), "sx"), (dict(sy=float("nan")), "sy"),
                     (dict(sx=float("inf")), "sx")]:
        rc, err, _ = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    for bad, word in [((0, 1, 0, 0, 65536, 4), "65535"), ((0, 1, (1 << 24) + 1, 0, 4, 4), "2^24"), ((0, 1, 0, 0, 4, 60000), "65535")]:
        rc, err, _ = call(rows=good + [bad])
        assert rc == VJ_ERR_LIMIT and word in err, bad
    assert call(rows=[])[0] == 0
    assert f(env._h, None, 0, None, 0, C.byref(TrackParams(32, 8, 0.0, 0.0, 0, 0)), None) == 0
    with pytest.raises(VjError) as ei:
        env.track([host], [(0, 0, 0, 0, 4, 4)], tmpl=10)
    assert ei.value.code == VJ_ERR_ARG
    rc, err, res = call()
    assert rc == 0 and tc.equal(res, want), err


# ------------------------------------------------------------------------------------------------------- 4. bridge_detections
def test_bridge_detections_on_the_device_equals_its_cpu_run(env, oracle):
    import torch
    video = tc.video()
    a, b = tc.video_box(30, 20, 32, 32), tc.video_box(90, 60, 32, 32)
    kw = dict(tmpl=tc.VIDEO_TR[0], radius=tc.VIDEO_TR[1])
    for rects in ([a[0], a[4]] + b[:2] + b[3:], [a[0], a[1], a[4], b[2]], a + b):
        want = bridge_detections(None, video, rects, track=tc.track_with(oracle), **kw)
        got = bridge_detections(env, torch.from_numpy(np.stack(video)).cuda(), rects, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got = bridge_detections(env, list(video), rects, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # DeviceFrames, what preprocess() and yuv_to_bgr() return: one that holds all frames, the same inside a list, one per frame
        t = torch.from_numpy(np.stack(video)).cuda()
        torch.cuda.synchronize()
        whole = DeviceFrames.from_torch(t)
        assert whole.n == len(video)
        singles = [DeviceFrames(whole.frame_ptr(i), 1, whole.height, whole.width, whole.stride, whole.channels, 0, t) for i in range(whole.n)]
        for frames in (whole, [whole], singles, [singles[0], list(video)[1]] + singles[2:]):
            got = bridge_detections(env, frames, rects, **kw)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert len(want[0]) == len(a + b)
    rects = [a[0], a[4]] + b[:2] + b[3:]
    want = bridge_detections(None, video, rects, track=tc.track_with(oracle), **kw)
    assert sorted(want[1][len(rects):].tolist()) == [-1, 1, 1, 2]


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("which", [0, 1, 2])
def test_the_detectors_gaps_bridged_and_blurred(env, oracle, cascades, which):
    """Each 432 x 324 colour source of tests/extract_cases.py moved by (3, 2) per frame into a four-frame video: preprocess ->
    detect_opencv(min_neighbors=3) per frame -> one frame's faces removed -> bridge_detections -> paint("blur")."""
    import torch
    c, _ = cascades(pc.CASC)
    src = ec.e2e_bgr()[which]
    video = np.stack([ec.padded_crop(src, -3 * f, -2 * f, pc.E2E_SRC_W, pc.E2E_SRC_H) for f in range(4)])
    small = env.preprocess(video, size=pc.E2E_SIZE, equalize=True, color=True)[0]
    rects = env.detect_opencv(c, small, min_neighbors=3).rects
    per = [int((rects["frame"] == i).sum()) for i in range(4)]
    print("boxes per frame:", per)
    assert per[1] >= 1 and per[3] >= 1, "premise: the detector finds faces in the frames next to the emptied one"
    rects = rects[rects["frame"] != 2]
    kw = dict(scale=ec.MANY_SCALE)
    want_rects, want_age = bridge_detections(None, list(video), rects, track=tc.track_with(oracle), **kw)
    added = want_rects[len(rects):]
    print("carried:", [tuple(int(v) for v in r) + (int(g),) for r, g in zip(added, want_age[len(rects):])])
    assert len(added) >= 1 and (added[:, 0] == 2).any(), "premise: the restated bridge fills frame 2"
    t = torch.from_numpy(video.copy()).cuda()
    got_rects, got_age = bridge_detections(env, DeviceFrames.from_torch(t), rects, **kw)
    assert np.array_equal(got_rects, want_rects) and np.array_equal(got_age, want_age)
    want = np.stack(pcs.restate(list(video), want_rects, "blur", **kw))
    assert (want[2] != video[2]).mean() > 0.003
    assert env.paint(t, got_rects, "blur", **kw) is t
    assert np.array_equal(t.cpu().numpy(), want)
