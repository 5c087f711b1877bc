"""vj_track on the CPU: vj_track_layout through ctypes against the restated mappings, every argument error and its
message, the premises of the GPU tests stated on the restatement alone (tests/track_cases.py), and bridge_detections driven with
the restatement as its track= on the five-frame synthetic video."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import prep_cases as pc
import track_cases as tc
from clfacedetection_amd import TrackParams, VjError, bridge_detections, track_layout
from clfacedetection_amd.api import _Image

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8


# ------------------------------------------------------------------------------------------------------------------ 1. the layout
def test_layout_matches_the_restated_mappings():
    frames = tc.batch_frames()
    rows = tc.batch_rows()
    for (t, r), scale in [(tc.BATCH_TR, tc.BATCH_SCALE), ((12, 3), (1.0, 1.0)), ((64, 16), (0.7, 2.3)), ((8, 1), (0, 0))]:
        tr, sr, nbytes = track_layout(frames, rows, t, r, scale)
        for k, row in enumerate(rows):
            assert tuple(tr[k]) == ec.map_region((row[0],) + row[2:], scale, 0.0), (t, r, k)
            assert tuple(sr[k]) == ec.map_region((row[1],) + row[2:], scale, r / t), (t, r, k)
        side = (t + 2 * r) ** 2
        assert nbytes == len(rows) * t * t + len(rows) * ((side + 15) // 16 * 16)
    assert track_layout(frames, np.zeros((0, 6), np.int32))[2] == 0


def test_a_box_of_the_templates_size_is_searched_at_identity():
    """cvRound(t * (r / t)) == r for every legal pair: at w0 = t the search patch is t + 2 r source pixels wide."""
    for t in range(8, 65, 4):
        for r in range(1, 17):
            assert pc.cv_round(t * (r / t)) == r
    tr, sr, _ = track_layout(tc.shift_pair(), [(0, 1) + tc.SHIFT_BOX], *tc.SHIFT_TR)
    x, y, w, h = tc.SHIFT_BOX
    t, r = tc.SHIFT_TR
    assert tuple(tr[0]) == (0, x, y, w, h) and tuple(sr[0]) == (1, x - r, y - r, t + 2 * r, t + 2 * r)


def test_default_params(lib):
    p = TrackParams()
    lib.vj_track_default(C.byref(p))
    assert (p.tmpl, p.radius, p.sx, p.sy, p.flags, p.reserved) == (32, 8, 0.0, 0.0, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ 2. the errors
def test_every_argument_error_and_its_message(lib):
    a, b = np.zeros((40, 50), np.uint8), np.zeros((30, 36, 3), np.uint8)
    ok = [_Image(a.ctypes.data, 50, 40, 50, 0, 1), _Image(b.ctypes.data, 36, 30, 108, 0, 3)]
    good = [(0, 1, 5, 5, 20, 20), (1, 1, -3, 2, 30, 20)]

    def call(images=ok, n=None, rows=good, nr=None, p=True, outs=True, **kw):
        q = TrackParams()
        lib.vj_track_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images) if images is not None else None
        r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 6)) if rows is not None else None
        m = len(r) if r is not None else 2
        tr, sr = np.zeros((max(m, 1), 5), np.int32), np.zeros((max(m, 1), 5), np.int32)
        nbytes = C.c_uint64(7)
        rc = lib.vj_track_layout(arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if r is not None else None,
                                 m if nr is None else nr, C.byref(q) if p else None, tr.ctypes.data if outs else None,
                                 sr.ctypes.data if outs else None, C.byref(nbytes))
        return rc, lib.vj_last_error().decode()

    assert call()[0] == 0
    for kw in (dict(images=None), dict(rows=None), dict(p=False), dict(outs=False), dict(n=-1), dict(nr=-1)):
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and "null argument" in err, kw
    for bad in (_Image(None, 8, 4, 8, 0, 1), _Image(a.ctypes.data, 0, 4, 8, 0, 1), _Image(a.ctypes.data, 8, 4, 7, 0, 1), _Image(a.ctypes.data, 8, 4, 16, 0, 2)):
        rc, err = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err
    for bad, word in [((2, 0, 0, 0, 4, 4), "src_frame"), ((-1, 0, 0, 0, 4, 4), "src_frame"), ((0, 2, 0, 0, 4, 4), "dst_frame"),
                      ((0, -1, 0, 0, 4, 4), "dst_frame")]:
        rc, err = call(rows=good + [bad])
        assert rc == VJ_ERR_ARG and "row 2" in err and word in err, bad
    for bad in ((0, 1, 0, 0, 0, 4), (0, 1, 0, 0, 4, 0), (1, 0, 0, 0, -3, 4)):
        rc, err = call(rows=good + [bad])
        assert rc == VJ_ERR_ARG and "region 2" in err, bad
    for kw, word in [(dict(tmpl=4), "tmpl"), (dict(tmpl=68), "tmpl"), (dict(tmpl=30), "tmpl"), (dict(tmpl=0), "tmpl"), (dict(tmpl=-32), "tmpl"),
                     (dict(radius=0), "radius"), (dict(radius=17), "radius"), (dict(radius=-1), "radius"), (dict(flags=1), "flags"),
                     (dict(reserved=7), "reserved"), (dict(sx=-1.0), "sx"), (dict(sx=float("inf")), "sx"), (dict(sy=float("nan")), "sy"),
                     (dict(sy=-0.5), "sy")]:
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    for bad, kw, word in [((0, 1, 0, 0, 65536, 4), {}, "65535"), ((0, 1, (1 << 24) + 1, 0, 4, 4), {}, "2^24"), ((0, 1, 0, 0, 4, 40000), dict(sy=2.0), "65535"),
                          ((0, 1, 0, 0, 60000, 4), dict(tmpl=8, radius=16), "65535")]:    # the margin takes the last one over the limit
        rc, err = call(rows=good + [bad], **kw)
        assert rc == VJ_ERR_LIMIT and word in err and "region 2" in err, bad
    assert call(rows=[])[0] == 0
    assert lib.vj_track_layout(None, 0, None, 0, C.byref(TrackParams(32, 8, 0.0, 0.0, 0, 0)), None, None, C.byref(C.c_uint64(0))) == 0
    with pytest.raises(VjError) as ei:
        track_layout([a], [(0, 0, 0, 0, 4, 4)], tmpl=10)
    assert ei.value.code == VJ_ERR_ARG and "tmpl" in str(ei.value)


# ---------------------------------------------------------------------------------------------------------------- 3. the premises
def one(oracle, frames, row, t, r, scale=(1.0, 1.0)):
    return tc.restate(oracle, frames, [row], t, r, scale)[0]


def test_premise_the_known_shift(oracle):
    m = one(oracle, tc.shift_pair(), (0, 1) + tc.SHIFT_BOX, *tc.SHIFT_TR)
    x, y, w, h = tc.SHIFT_BOX
    assert (m["dx"], m["dy"], m["sad"], m["sad0"]) == (3, -2, 0, tc.SHIFT_SAD0)
    assert (m["x"], m["y"], m["w"], m["h"]) == (x + 3, y - 2, w, h)
    back = one(oracle, tc.shift_pair(), (1, 0) + tc.SHIFT_BOX, *tc.SHIFT_TR)
    assert (back["dx"], back["dy"], back["sad"]) == (-3, 2, 0)
    same = one(oracle, tc.shift_pair(), (1, 1) + tc.SHIFT_BOX, *tc.SHIFT_TR)
    assert (same["dx"], same["dy"], same["sad"], same["sad0"]) == (0, 0, 0, 0)


def test_premise_scaled(oracle):
    m = one(oracle, tc.scaled_pair(), (0, 1) + tc.SCALED_BOX, *tc.SCALED_TR)
    x, y, w, h = tc.SCALED_BOX
    assert (m["dx"], m["dy"]) == (2, -1) and m["sad"] < m["sad0"]
    # the search patch of a 96 x 72 box is 144 x 108 source pixels on 48 patch pixels: 3 and 2.25 per patch pixel; -2.25 rounds to -2
    assert (m["x"], m["y"], m["w"], m["h"]) == (x + 6, y - 2, w, h)


def test_premise_ties_and_the_accumulator(oracle):
    flat = one(oracle, [tc.flat_frame(), tc.flat_frame(78)], (0, 0, 10, 10, 30, 20), 32, 8)
    assert (flat["dx"], flat["dy"], flat["sad"], flat["sad0"]) == (0, 0, 0, 0)
    off = one(oracle, [tc.flat_frame(), tc.flat_frame(78)], (0, 1, 10, 10, 30, 20), 32, 8)
    assert (off["dx"], off["dy"], off["sad"]) == (0, 0, 32 * 32)                     # every sum equal: the flat patch stays
    t, r = tc.PERIOD4_TR
    T, S = tc.patches(oracle, tc.period4_pair(), [(0, 1) + tc.PERIOD4_BOX], t, r)
    sad = tc.sads(T[0], S[0], r)
    assert (sad[:, [r - 2, r + 2]] == 0).all() and (sad[:, [c for c in range(2 * r + 1) if c not in (r - 2, r + 2)]] > 0).all()
    m = one(oracle, tc.period4_pair(), (0, 1) + tc.PERIOD4_BOX, t, r)
    assert (m["dx"], m["dy"], m["sad"]) == (-2, 0, 0)
    t, r = tc.ACC_TR
    T, S = tc.patches(oracle, tc.acc_pair(), [(0, 1) + tc.ACC_BOX], t, r)
    assert (tc.sads(T[0], S[0], r) == tc.ACC_SAD).all() and tc.ACC_SAD == 1044480 and 257 * 255 <= 65535 < 258 * 255
    m = one(oracle, tc.acc_pair(), (0, 1) + tc.ACC_BOX, t, r)
    assert (m["dx"], m["dy"], m["sad"], m["sad0"]) == (0, 0, tc.ACC_SAD, tc.ACC_SAD)


def test_premise_boxes_outside_their_frames(oracle):
    res = tc.restate(oracle, tc.shift_pair(), [(0, 1) + b for b in tc.OUTSIDE_BOXES], *tc.SHIFT_TR)
    assert (res["dx"][0], res["dy"][0]) == (3, -2)                                   # the box at (-10, -7): enough of it lies inside
    assert (res["dx"][1], res["dy"][1]) == (3, -2)
    wholly = [k for k, (x, y, w, h) in enumerate(tc.OUTSIDE_BOXES) if x + w <= 0 or y + h <= 0 or x >= tc.SHIFT_W or y >= tc.SHIFT_H]
    assert len(wholly) >= 4 and len(wholly) < len(tc.OUTSIDE_BOXES)


def test_premise_the_ends_of_t_and_r():
    counts = [((2 * r + 1) ** 2, (2 * r + 1 + 3) // 4 * (2 * r + 1)) for t, r in tc.TR_PAIRS]
    assert any(c % 4 == 0 for _, c in counts) and any(c % 4 for _, c in counts)
    # units of four dx: fewer than a wave's lanes, more than a workgroup's; the batch's (32, 8) lies between
    assert any(u > 256 for _, u in counts) and any(u < 64 for _, u in counts) and 64 < (2 * 8 + 1 + 3) // 4 * (2 * 8 + 1) <= 256 and tc.BATCH_TR == (32, 8)
    assert {t for t, _ in tc.TR_PAIRS} >= {8, 64} and {r for _, r in tc.TR_PAIRS} >= {1, 16}
    assert any((t + 2 * r) % 4 == 2 for t, r in tc.TR_PAIRS) and any((t + 2 * r) % 4 == 0 for t, r in tc.TR_PAIRS)


def test_premise_the_batch(oracle):
    rows = tc.batch_rows()
    assert len(rows) == 70 and {r[0] for r in rows} == set(range(5))
    assert any(r[0] < r[1] for r in rows) and any(r[0] > r[1] for r in rows) and any(r[0] == r[1] for r in rows)
    assert {f.shape[2] if f.ndim == 3 else 1 for f in tc.batch_frames()} == {1, 3, 4}
    res = pc.once("track_batch", lambda: tc.restate(oracle, tc.batch_frames(), rows, *tc.BATCH_TR, tc.BATCH_SCALE))
    assert len({(int(m["dx"]), int(m["dy"])) for m in res}) > 10 and (res["sad"] <= res["sad0"]).all()
    assert len({int(v) for v in res["sad"]}) > 60 and (res["sad"] > 0).any()


# ------------------------------------------------------------------------------------------------------- 4. bridge_detections
A = (30, 20, 32, 32)
B = (90, 60, 32, 32)
KW = dict(tmpl=tc.VIDEO_TR[0], radius=tc.VIDEO_TR[1])


class Counting:
    def __init__(self, fn):
        self.fn, self.calls, self.rows = fn, 0, []

    def __call__(self, frames, rows, **kw):
        self.calls += 1
        self.rows.append(np.asarray(rows).reshape(-1, 6))
        return self.fn(frames, rows, **kw)


def bridged(oracle, rects, frames=None, **kw):
    track = Counting(tc.track_with(oracle))
    rects = np.asarray(rects, np.int32).reshape(-1, 5)
    out, age = bridge_detections(None, frames or tc.video(), rects, track=track, **dict(KW, **kw))
    assert np.array_equal(out[:len(rects)], rects) and (age[:len(rects)] == 0).all() and len(out) == len(age)
    assert track.calls <= 2 * kw.get("max_age", 2)
    return [tuple(int(v) for v in r) + (int(a),) for r, a in zip(out[len(rects):], age[len(rects):])], track


def test_bridge_a_box_removed_from_one_frame_comes_back(oracle):
    full = tc.video_box(*A) + tc.video_box(*B)
    rects = [r for r in full if r != tc.video_box(*A)[2]]
    assert len(rects) == len(full) - 1
    added, track = bridged(oracle, rects)
    assert added == [tc.video_box(*A)[2] + (1,)]                                     # the neighbour's position moved by (2, 1)
    assert track.calls == 1 and len(track.rows[0]) == 1 and tuple(track.rows[0][0][:2]) == (1, 2)


def test_bridge_a_gap_is_filled_from_both_sides(oracle):
    a = tc.video_box(*A)
    rects = [a[0], a[4]] + tc.video_box(*B)
    added, track = bridged(oracle, rects, max_age=2)
    assert added == [a[1] + (1,), a[2] + (2,), a[3] + (-1,)]
    assert track.calls == 3
    added, _ = bridged(oracle, [a[0], a[1], a[4]], max_age=1)                        # a two-frame gap, one step from each side
    assert added == [a[2] + (1,), a[3] + (-1,)]
    added, _ = bridged(oracle, [a[0], a[1], a[4]], max_age=2)                        # ... and the forward pass alone where it may go on
    assert added == [a[2] + (1,), a[3] + (2,)]


def test_bridge_a_box_with_a_partner_is_not_tracked(oracle):
    full = tc.video_box(*A) + tc.video_box(*B)
    added, track = bridged(oracle, full)
    assert added == [] and track.calls == 0
    # a partner that overlaps enough counts, one that does not does not: against the box of frame 1 the true box of frame 2 moved by
    # 6 more pixels has IoU 0.57, moved by 20 more pixels 0.18
    a = tc.video_box(*A)
    near = (2, a[2][1] + 6, a[2][2], 32, 32)
    far = (2, a[2][1] + 20, a[2][2], 32, 32)
    added, track = bridged(oracle, [a[0], a[1], near, a[3], a[4]])
    assert added == [] and track.calls == 0
    added, track = bridged(oracle, [a[0], a[1], far, a[3], a[4]])
    assert a[2] + (1,) in added


def test_bridge_a_row_over_max_mad_is_dropped(oracle):
    frames = [np.array(f) for f in tc.video()]
    b = tc.video_box(*B)
    _, x, y, w, h = b[2]
    frames[2][y - 8:y + h + 8, x - 8:x + w + 8] = np.random.default_rng(56).integers(0, 256, (h + 16, w + 16), dtype=np.uint8)
    rects = [r for r in b if r[0] != 2]
    m = tc.restate(oracle, frames, [(1, 2) + b[1][1:]], *tc.VIDEO_TR)[0]
    assert m["sad"] > 12.0 * 32 * 32
    added, track = bridged(oracle, rects, frames=frames)
    assert added == [] and track.calls == 2                                          # tried from both sides, dropped both times
    added, _ = bridged(oracle, rects, frames=frames, max_mad=255.0)
    assert [r[0] for r in added] == [2] and added[0][5] == 1


def test_bridge_max_age_0_returns_the_input(oracle):
    rects = [tc.video_box(*A)[0], tc.video_box(*B)[3]]
    added, track = bridged(oracle, rects, max_age=0)
    assert added == [] and track.calls == 0


def test_bridge_scale_takes_the_boxes_to_the_frames_and_back(oracle):
    """Detector coordinates at half the frames' resolution: the boxes come back in them."""
    a = tc.video_box(*A)
    half = [(f, x // 2, y // 2, 16, 16) for f, x, y, w, h in a]
    rects = [half[0], half[1], half[3], half[4]]
    added, _ = bridged(oracle, rects, scale=(2.0, 2.0))
    want = tc.restate(oracle, tc.video(), [(1, 2) + half[1][1:]], *tc.VIDEO_TR, scale=(2.0, 2.0))[0]
    assert added == [(2, pc.cv_round(want["x"] / 2.0), pc.cv_round(want["y"] / 2.0), 16, 16, 1)]
