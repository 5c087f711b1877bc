"""vj_paint_yuv on the device: the WHOLE buffers after Environment.paint_yuv — sentinel bytes before and behind
every plane and in the row padding included — against the numpy restatement (tests/paint_yuv_cases.py) with np.array_equal, and,
asserted directly, every byte outside the union of the painted sets bit-identical to the input.  The smallest shapes at which the
kernels can still go wrong: 2 x 2, 38 x 30 and 300 x 40 frames in all three layouts (and one 524 x 68 frame whose I420 chroma rows
straddle the block constants too); regions of 1 x 1 at even and odd positions, 2 x 2 at an odd corner, 1 x n, n x 1, every side and
corner, partly and wholly outside, the whole frame, all sixteen parities of K; every mode with and without the ellipse, every size
as `size` and one as `rel`; overlaps and the shared chroma sample; planes at every address mod 4; the eleven mixed frames whole and in
slices; the detector's boxes end to end; the error cases.  The premises are checked on the CPU in tests/test_paint_yuv_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import mixed_cases as mc
import paint_cases as pcs
import paint_yuv_cases as pyc
import prep_cases as pc
import track_cases as tc
import yuv_cases as yc
from cases import tunables
from clfacedetection_amd import PaintParams, VjError, YuvFrames, bridge_detections
from clfacedetection_amd.api import _YuvImage

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
MODES = ["fill", "outline", "pixelate", "blur"]
# every size of the issue: BLUR kk 3, 5, 15, 31, 255; PIXELATE s 1, 2, 3, 7, 64; OUTLINE t 1, 2, 3, 40
SIZES = {"fill": [0], "outline": [1, 2, 3, 40], "pixelate": [1, 2, 3, 7, 64], "blur": [3, 5, 15, 31, 255]}
NAMES = yc.LAYOUT_NAMES


class Frame:
    """A frame whose planes lie in one buffer at chosen addresses mod 4 with padded strides (paint_yuv_cases.place), everything that
    is no sample holding the sentinel: writeable strided host views, or device memory."""

    def __init__(self, planes, layout, kind, mods=(0, 0, 0), pad=0):
        self.planes, self.layout, self.kind = planes, layout, kind
        self.before, self.offs = pyc.place(planes, layout, mods, pad)
        self.h, self.w = planes[0].shape
        if kind == "host":
            self.base = self.before.copy()
            self.item = tuple(np.lib.stride_tricks.as_strided(self.base[o:], shape=p.shape, strides=(st, 1), writeable=True)
                              for p, (o, st) in zip(planes, self.offs))
        else:
            import torch
            self.t = torch.from_numpy(self.before).cuda()
            torch.cuda.synchronize()
            ptr = [self.t.data_ptr() + o for o, _ in self.offs] + [0]
            self.item = YuvFrames(ptr[0], ptr[1], ptr[2] if layout == yc.I420 else 0, 1, self.h, self.w, self.offs[0][1], self.offs[1][1], layout, 0, self.t)

    def reset(self):
        if self.kind == "host":
            self.base[:] = self.before
        else:
            import torch
            self.t.copy_(torch.from_numpy(self.before))
            torch.cuda.synchronize()

    def now(self):
        return self.base if self.kind == "host" else self.t.cpu().numpy()

    def want(self, planes):
        b = self.before.copy()
        for p, (o, st) in zip(planes, self.offs):
            b[o:o + st * p.shape[0]].reshape(p.shape[0], st)[:, :p.shape[1]] = p
        return b

    def plane_views(self, buf):
        return [buf[o:o + st * p.shape[0]].reshape(p.shape[0], st)[:, :p.shape[1]] for p, (o, st) in zip(self.planes, self.offs)]


_ONCE = {}


def check(env, frames, rects, mode, **kw):
    """One paint_yuv() call on `frames` (Frame objects; the host frames share one layout) against the restatement: every byte of
    every buffer; and every byte outside the union of the painted sets against the INPUT."""
    for f in frames:
        f.reset()                                                                 # a Frame may serve several calls
    items = [f.item for f in frames]
    host_lay = next((f.layout for f in frames if f.kind == "host"), yc.NV12)
    assert all(f.layout == host_lay for f in frames if f.kind == "host")
    got = env.paint_yuv(items, rects, mode, layout=NAMES[host_lay], **kw)
    assert got is items
    sources, lays = [f.planes for f in frames], [f.layout for f in frames]
    key = (tuple(p.tobytes() for s in sources for p in s), tuple(lays), np.asarray(rects).tobytes(), mode, repr(sorted(kw.items())))
    if hash(key) not in _ONCE:
        _ONCE[hash(key)] = (pyc.restate(sources, lays, rects, mode, **kw),
                            pyc.painted_union(sources, rects, mode, **{k: v for k, v in kw.items() if k != "fill"}))
    want, union = _ONCE[hash(key)]
    for i, f in enumerate(frames):
        now, exp = f.now(), f.want(want[i])
        if not np.array_equal(now, exp):
            bad = np.flatnonzero(now != exp)
            pl = max(j for j, (o, _) in enumerate(f.offs) if o <= bad[0]) if bad[0] >= f.offs[0][0] else -1
            o, st = f.offs[max(pl, 0)]
            raise AssertionError((mode, kw, "frame", i, f.kind, NAMES[f.layout], "first bad byte", int(bad[0]), "of", len(bad), "plane", pl,
                                  "row", int((bad[0] - o) // st), "col", int((bad[0] - o) % st), "got", int(now[bad[0]]), "want", int(exp[bad[0]])))
        # directly: nothing outside the painted sets changed (the sentinels are covered by the comparison above)
        lm, cm = union[i]
        views, orig = f.plane_views(now), f.planes
        assert np.array_equal(views[0][~lm], orig[0][~lm])
        if f.layout == yc.I420:
            assert np.array_equal(views[1][~cm], orig[1][~cm]) and np.array_equal(views[2][~cm], orig[2][~cm])
        else:
            keep = ~np.repeat(cm, 2, axis=1)
            assert np.array_equal(views[1][keep], orig[1][keep])


def both_kinds(planes_list, lays, variant=0):
    """The frames as host views and as device frames, their planes at addresses 0 .. 3 mod 4 and with padded strides."""
    host = [Frame(p, l, "host", ((i + variant) % 4, (i + 2 * variant + 1) % 4, (3 * i + variant + 2) % 4), (3 * i + variant) % 5)
            for i, (p, l) in enumerate(zip(planes_list, lays))]
    dev = [Frame(p, l, "dev", ((i + 1 + variant) % 4, (2 * i + variant + 3) % 4, (i + 3 * variant) % 4), (i + 2 * variant) % 4)
           for i, (p, l) in enumerate(zip(planes_list, lays))]
    return host, dev


def on_frame(rects, i):
    return [(i,) + tuple(r[1:]) for r in rects]


# ------------------------------------------------------------------------------------------------- 1. small regions, every size
@pytest.mark.parametrize("lay", pyc.LAYOUTS)
@pytest.mark.parametrize("ellipse", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_small_regions_every_size(env, mode, ellipse, lay):
    src = [pyc.frame(pyc.W, pyc.H, lay, 21), pyc.frame(2, 2, lay, 22)]
    rects = pyc.SMALL_RECTS + on_frame(pyc.TINY_RECTS, 1)
    for v, size in enumerate(SIZES[mode]):
        for frames in both_kinds(src, [lay, lay], v):
            check(env, frames, rects, mode, size=size, ellipse=ellipse, fill=pyc.FILL_BGR)
    whole = pyc.WHOLE + [(1, 0, 0, 2, 2)]
    for frames in both_kinds(src, [lay, lay], 1):                        # one size as a fraction of the shorter side
        check(env, frames, rects, mode, rel=0.3, ellipse=ellipse, fill=pyc.FILL_BGR)
        check(env, frames, whole, mode, rel=0.2, ellipse=ellipse, fill=pyc.FILL_BGR)
        check(env, frames, whole, mode, size=SIZES[mode][-1], ellipse=ellipse, fill=pyc.FILL_BGR)
        check(env, frames, rects, mode, rel=0.4, scale=(1.5, 0.5), margin=0.25, ellipse=ellipse, fill=pyc.FILL_BGR)


# -------------------------------------------------------------------------------------- 2. widths and heights around the blocks
@pytest.mark.parametrize("mode", MODES)
def test_widths_and_heights_around_the_blocks(env, mode):
    """Luma, pair-plane and I420 chroma rows of 254 .. 260 bytes (on each side of a wave row of 64 four-byte slots and of a band of 256
    byte columns) and of 2 .. 6 bytes (a lane's slot), heights on each side of the 32-row block and band — one wide region per call,
    so that no later region hides it, with the small ones."""
    size = {"fill": 0, "outline": 2, "pixelate": 5, "blur": 7}[mode]
    wide, big = pyc.wide_rects(), pyc.big_rects()
    for lay in pyc.LAYOUTS:
        src = [pyc.frame(pyc.WIDE_W, pyc.WIDE_H, lay, 5)]
        for v, r in enumerate(wide[:4]):
            for frames in both_kinds(src, [lay], v):
                check(env, frames, [r] + wide[4:], mode, size=size, ellipse=bool(v & 1), fill=pyc.FILL_BGR)
        for frames in both_kinds(src, [lay], 2):                          # the whole frame, the largest blur and cell
            check(env, frames, [(0, 0, 0, pyc.WIDE_W, pyc.WIDE_H)], mode, size={"fill": 0, "outline": 3, "pixelate": 64, "blur": 255}[mode])
    for lay in (yc.I420, yc.NV21):
        src = [pyc.frame(pyc.BIG_W, pyc.BIG_H, lay, 6)]
        for v, r in enumerate(big):
            frames = both_kinds(src, [lay], v)[v & 1]
            check(env, frames, [r], mode, size=size if v < 3 else {"fill": 0, "outline": 40, "pixelate": 64, "blur": 255}[mode], ellipse=v == 2)


# -------------------------------------------------------------------------------------------------------------------- 3. overlaps
@pytest.mark.parametrize("mode", MODES)
def test_overlaps_the_highest_index_wins_from_the_original_planes(env, mode):
    lays = [yc.NV12, yc.NV21, yc.I420]
    mixed = [(2, 3, 3, 20, 15), (0, 11, 7, 22, 18), (1, 6, 12, 13, 9), (0, 3, 3, 20, 15), (2, 11, 7, 22, 18), (1, 2, 2, 30, 20), (0, 6, 12, 13, 9),
             (1, 7, 4, 5, 7), (2, 2, 4, 5, 7), (2, 7, 4, 5, 7)]                               # regions given in mixed frame order
    cases = [pyc.OVERLAP_RECTS, pyc.OVERLAP_RECTS[:2], pyc.TWICE_RECTS, pyc.SHARED_RECTS, pyc.SHARED_RECTS[::-1]]
    for v, rects in enumerate(cases):
        all3 = [q for i in range(3) for q in on_frame(rects, i)]
        for lay in lays:                                                                    # host frames share the call's layout
            src = [pyc.frame(pyc.W, pyc.H, lay, 30 + i) for i in range(3)]
            check(env, both_kinds(src, [lay] * 3, v)[0], all3, mode, rel=0.3, fill=pyc.FILL_BGR)
        src = [pyc.frame(pyc.W, pyc.H, l, 40 + i) for i, l in enumerate(lays)]
        check(env, both_kinds(src, lays, v)[1], all3, mode, rel=0.3, fill=pyc.FILL_BGR)
    src = [pyc.frame(pyc.W, pyc.H, l, 50 + i) for i, l in enumerate(lays)]
    check(env, both_kinds(src, lays, 1)[1], mixed, mode, size=3, fill=pyc.FILL_BGR)
    # a later ellipse that leaves the earlier region the corners of its rectangle
    nested = [q for i in range(3) for q in on_frame([(0, 3, 2, 31, 25), (0, 8, 6, 19, 15)], i)]
    check(env, both_kinds(src, lays, 2)[1], nested, mode, rel=0.25, ellipse=True, fill=pyc.FILL_BGR)


# ------------------------------------------------------------------------------------------------------------ 4. memory placement
@pytest.mark.parametrize("lay", pyc.LAYOUTS)
def test_planes_at_every_address_mod_4_with_padded_strides(env, lay):
    src = [pyc.frame(pyc.W, pyc.H, lay, 23)]
    rects = [(0, 1, 1, 35, 27), (0, -2, 5, 12, 9), (0, 21, 15, 30, 30), (0, 0, 0, pyc.W, pyc.H), (0, 3, 3, 11, 8), (0, 7, 9, 2, 2)]
    for a in range(4):
        for b in range(4):
            for kind in ("dev", "host"):
                f = Frame(src[0], lay, kind, (a, b, (a + 2 * b + 1) % 4), (a + b) % 4)
                odd = (a + b) % 2
                check(env, [f], rects, "blur" if odd else "pixelate", size=5 if odd else 3, ellipse=b == 2)
                if kind == "dev":
                    check(env, [f], rects[:3], "fill" if odd else "outline", size=2, fill=pyc.FILL_BGR)


@pytest.mark.parametrize("lay", pyc.LAYOUTS)
def test_separate_planes_stacked_arrays_tensors_and_what_is_refused(env, lay):
    import torch
    name = NAMES[lay]
    srcs = [pyc.frame(pyc.W, pyc.H, lay, 60), pyc.frame(pyc.W, pyc.H, lay, 61)]
    rects = [(0, 4, 4, 21, 15), (1, -3, 10, 15, 30), (1, 9, 3, 8, 9)]
    want = pyc.restate(srcs, lay, rects, "blur", size=5)
    stacked_want = np.stack([yc.stacked(w, lay) for w in want])
    # a batch as one stacked array, painted in place; the same as a CUDA tensor
    batch = np.stack([yc.stacked(s, lay) for s in srcs])
    arr = batch.copy()
    assert env.paint_yuv(arr, rects, "blur", size=5, layout=name) is arr and np.array_equal(arr, stacked_want)
    t = torch.from_numpy(batch).cuda()
    assert env.paint_yuv(t, rects, "blur", size=5, layout=name) is t and np.array_equal(t.cpu().numpy(), stacked_want)
    yf = YuvFrames.from_torch(torch.from_numpy(batch).cuda(), name)
    env.paint_yuv(yf, rects, "blur", size=5)
    assert np.array_equal(yf.owner.cpu().numpy(), stacked_want) and env.paint_yuv_timing() > 0
    # a list mixing a stacked host array, a tensor of one frame and a YuvFrames
    one = yc.stacked(srcs[0], lay).copy()
    t1 = torch.from_numpy(yc.stacked(srcs[1], lay)[None].copy()).cuda()
    env.paint_yuv([one, t1], rects, "blur", size=5, layout=name)
    assert np.array_equal(one, stacked_want[0]) and np.array_equal(t1.cpu().numpy()[0], stacked_want[1])
    # separately allocated device planes
    planes = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in srcs[0]]
    sep = YuvFrames(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr() if lay == yc.I420 else 0, 1, pyc.H, pyc.W,
                    pyc.W, srcs[0][1].shape[1], lay, 0, planes)
    env.paint_yuv(sep, rects[:1], "pixelate", size=4)
    w1 = pyc.restate(srcs[:1], lay, rects[:1], "pixelate", size=4)[0]
    assert all(np.array_equal(p.cpu().numpy(), q) for p, q in zip(planes, w1))
    # a strided host view of a wider stacked array (the pair layouts: the chroma rows of I420 must follow each other)
    if lay != yc.I420:
        widebuf = np.full((pyc.H * 3 // 2, pyc.W + 6), pyc.SENTINEL, np.uint8)
        view = widebuf[:, 3:3 + pyc.W]
        view[:] = yc.stacked(srcs[0], lay)
        env.paint_yuv(view, rects[:1], "blur", size=5, layout=name)
        assert np.array_equal(view, stacked_want[0])                                         # (frame 0 holds the first region only)
        assert (widebuf[:, :3] == pyc.SENTINEL).all() and (widebuf[:, 3 + pyc.W:] == pyc.SENTINEL).all()
    # what the wrapper would have to copy is refused, and nothing is painted
    ro = batch.copy()
    ro.setflags(write=False)
    for bad in (ro, batch.astype(np.int16), batch.astype(np.float32), batch[:, :, ::2]):
        with pytest.raises(ValueError):
            env.paint_yuv(bad, rects[:1], "fill", layout=name)
    assert np.array_equal(ro, batch)
    with pytest.raises(ValueError):
        env.paint_yuv(batch.copy(), rects[:1], "smear", layout=name)
    with pytest.raises(ValueError):
        env.paint_yuv(batch.copy(), rects[:1], "fill", fill=(1, 2, 3, 4), layout=name)


# ---------------------------------------------------------------------------------------------------------- 5. batches and slicing
@pytest.mark.parametrize("mode", ["outline", "pixelate", "blur"])
def test_the_eleven_mixed_frames_in_one_call_and_in_slices(env, mode):
    rects = []
    for i, (w, h) in enumerate(yc.MIXED_SIZES):
        rects += [(i, w // 4, h // 4, w // 2 + 1, h // 2 + 1), (i, -3, h - 11, 25, 24), (i, w // 3, 1, 49, 47)]
    rects = rects[::2] + rects[1::2]                                                         # not sorted by frame
    kw = dict(rel=0.2, margin=0.1, fill=pyc.FILL_BGR)
    for host_lay in pyc.LAYOUTS:
        lays = [host_lay if i % 2 == 0 else pyc.LAYOUTS[(i // 2) % 3] for i in range(len(yc.MIXED_SIZES))]
        src = [pyc.frame(w, h, l, 70 + i) for i, ((w, h), l) in enumerate(zip(yc.MIXED_SIZES, lays))]
        frames = [Frame(s, l, "dev" if i % 2 else "host", ((i + 1) % 4, (i + 2) % 4, (3 * i) % 4), i % 4) for i, (s, l) in enumerate(zip(src, lays))]
        for sub in (None, "3", "2", "1"):
            with tunables(env, *((("max_subbatch", sub),) if sub else ())):
                check(env, frames, rects, mode, **kw)


def test_no_region_and_regions_that_paint_nothing(env):
    lays = [yc.NV12, yc.NV21, yc.I420]
    src = [pyc.frame(pyc.W, pyc.H, l, 80 + i) for i, l in enumerate(lays)]
    check(env, both_kinds(src, lays)[1], np.zeros((0, 5), np.int32), "blur")
    check(env, both_kinds(src, lays)[1], [(0, 100, 100, 6, 6), (1, -40, 3, 6, 6), (2, 5, -30, 6, 6)], "fill", fill=(9, 9, 9))
    check(env, both_kinds(src[:1], lays[:1])[0], [(0, 100, 100, 6, 6)], "pixelate")
    assert env.paint_yuv([], np.zeros((0, 5), np.int32)) == []


# ---------------------------------------------------------------------------------------------------------------- 6. cross-checks
@pytest.mark.parametrize("mode", MODES)
def test_the_y_plane_is_what_paint_makes_of_it_as_a_gray_frame(env, mode):
    import torch
    f = pyc.frame(pyc.WIDE_W, pyc.WIDE_H, yc.NV12, 90)
    rects = pyc.wide_rects() + [(0, 30, 4, 100, 30), (0, 60, 10, 100, 25)]
    Yc = pyc.color_of(pyc.FILL_BGR)[0]
    for ellipse in (False, True):
        t = torch.from_numpy(yc.stacked(f, yc.NV12)[None].copy()).cuda()
        gray = torch.from_numpy(f[0][None].copy()).cuda()
        env.paint_yuv(t, rects, mode, rel=0.2, ellipse=ellipse, fill=pyc.FILL_BGR)
        env.paint(gray, rects, mode, rel=0.2, ellipse=ellipse, fill=(Yc,))
        assert np.array_equal(t.cpu().numpy()[0, :pyc.WIDE_H], gray.cpu().numpy()[0])


# ------------------------------------------------------------------------------------------------------------------ 7. end to end
def test_the_detectors_gaps_bridged_and_blurred_in_nv12(env, oracle, cascades):
    """A 432 x 324 colour source of tests/extract_cases.py moved by (3, 2) per frame into a four-frame video, encoded as NV12:
    detect_opencv(luma()) -> one frame's faces removed -> bridge_detections on the luma -> paint_yuv("blur")."""
    import torch
    c, _ = cascades(pc.CASC)
    src = ec.e2e_bgr()[0]
    video = [ec.padded_crop(src, -3 * f, -2 * f, pc.E2E_SRC_W, pc.E2E_SRC_H) for f in range(4)]
    planes = [yc.encode(v, yc.NV12) for v in video]
    t = torch.from_numpy(np.stack([yc.stacked(p, yc.NV12) for p in planes])).cuda()
    yuv = YuvFrames.from_torch(t)
    rects = env.detect_opencv(c, yuv.luma(), min_neighbors=3).rects
    per = [int((rects["frame"] == i).sum()) for i in range(4)]
    print("boxes per frame:", per)
    assert per[1] >= 1 and per[3] >= 1, "premise: the detector finds faces in the frames next to the emptied one"
    rects = rects[rects["frame"] != 2]
    want_rects, want_age = bridge_detections(None, [p[0] for p in planes], rects, track=tc.track_with(oracle))
    added = want_rects[len(rects):]
    assert len(added) >= 1 and (added[:, 0] == 2).any(), "premise: the restated bridge fills frame 2"
    got_rects, got_age = bridge_detections(env, yuv.luma(), rects)
    assert np.array_equal(got_rects, want_rects) and np.array_equal(got_age, want_age)
    want = pyc.restate(planes, yc.NV12, want_rects, "blur")
    assert (want[2][0] != planes[2][0]).mean() > 0.003          # (the sources are gray pictures stored as BGR: their chroma is flat)
    assert env.paint_yuv(yuv, got_rects) is yuv
    assert np.array_equal(t.cpu().numpy(), np.stack([yc.stacked(w, yc.NV12) for w in want]))


# -------------------------------------------------------------------------------------------------------------- 8. the error cases
def test_argument_errors_leave_the_planes_and_the_environment_as_they_were(env, lib, cascades):
    import torch
    c, a = cascades(pc.CASC)
    plain = mc.frames()[0]
    base = env.detect(c, plain)
    assert len(base.rects) >= 10
    w, h = 130, 98
    dsrc = yc.stacked(pyc.frame(w, h, yc.NV12, 95), yc.NV12)
    dev = torch.from_numpy(dsrc.copy()).cuda()
    torch.cuda.synchronize()
    hsrc = yc.stacked(pyc.frame(66, 34, yc.I420, 96), yc.I420)
    host = hsrc.copy()
    hp = host.ctypes.data
    ok = [_YuvImage(dev.data_ptr(), dev.data_ptr() + w * h, None, w, h, w, w, yc.NV12, 1),
          _YuvImage(hp, hp + 66 * 34, hp + 66 * 34 + 33 * 17, 66, 34, 66, 33, yc.I420, 0)]
    good = [(0, 5, 5, 40, 40), (1, -3, 2, 30, 20)]
    f = lib.vj_paint_yuv

    def call(images=ok, n=None, rects=good, nr=None, p=True, e=env._h, expect_unchanged=True, **kw):
        q = PaintParams()
        lib.vj_paint_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_YuvImage * max(len(images), 1))(*images) if images is not None else None
        r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5)) if rects is not None else None
        rc = f(e, arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if r is not None else None,
               (len(r) if r is not None else 2) if nr is None else nr, C.byref(q) if p else None)
        err = lib.vj_last_error().decode()
        if expect_unchanged:                                                      # every error: the planes are as they were ...
            assert np.array_equal(dev.cpu().numpy(), dsrc) and np.array_equal(host, hsrc)
        assert np.array_equal(env.detect(c, plain).rects, base.rects)             # ... and a plain detect still matches
        return rc, err

    for kw in (dict(e=None), dict(images=None), dict(rects=None), dict(p=False), dict(n=-1), dict(nr=-1)):
        assert call(**kw)[0] == VJ_ERR_ARG, kw
    d = dev.data_ptr()
    for bad in (_YuvImage(None, d + w * h, None, 8, 4, 8, 8, 0, 1), _YuvImage(d, None, None, 8, 4, 8, 8, 0, 1), _YuvImage(d, d + 64, None, 8, 4, 8, 4, 2, 1),
                _YuvImage(d, d + 64, None, 0, 4, 8, 8, 0, 1), _YuvImage(d, d + 64, None, 7, 4, 8, 8, 0, 1), _YuvImage(d, d + 64, None, 8, 3, 8, 8, 0, 1),
                _YuvImage(d, d + 64, None, 8, 4, 7, 8, 0, 1), _YuvImage(d, d + 64, None, 8, 4, 8, 7, 0, 1), _YuvImage(d, d + 64, None, 8, 4, 8, 8, 3, 1)):
        rc, err = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err, err
    for bad in ((2, 0, 0, 4, 4), (-1, 0, 0, 4, 4), (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (1, 0, 0, -3, 4)):
        rc, err = call(rects=good + [bad])
        assert rc == VJ_ERR_ARG and "region 2" in err
    for kw, word in [(dict(mode=4), "mode"), (dict(mode=-1), "mode"), (dict(flags=2), "flags"), (dict(reserved=7), "reserved"),
                     (dict(size=-1), "size"), (dict(rel=0.0), "rel"), (dict(rel=-0.5), "rel"), (dict(rel=float("nan")), "rel"),
                     (dict(rel=float("inf")), "rel"), (dict(sx=-1.0), "sx"), (dict(sy=float("nan")), "sy"), (dict(margin=float("inf")), "margin")]:
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    # planes whose memory overlaps: another frame's by one byte (device, host), the same frame twice, the planes of one frame
    for images in (ok + [_YuvImage(d + w * h * 3 // 2 - 1, d + (1 << 20), None, 2, 2, 2, 2, 0, 1)], ok + [_YuvImage(hp + host.size - 1, hp + (1 << 20), None, 2, 2, 2, 2, 0, 0)],
                   ok + [ok[0]]):
        rc, err = call(images=images)
        assert rc == VJ_ERR_ARG and "overlaps" in err and "frame 2" in err, err
    rc, err = call(images=[_YuvImage(d, d + w * h - 1, None, w, h, w, w, yc.NV12, 1), ok[1]])
    assert rc == VJ_ERR_ARG and "frame 0" in err and "c0 plane overlaps frame 0's y plane" in err, err
    for kw, rects, word in [(dict(), good + [(0, 0, 0, 32768, 4)], "32767"), (dict(), good + [(0, (1 << 24) + 1, 0, 4, 4)], "2^24"), (dict(size=257), good, "255"),
                            (dict(mode=2, size=4097), good, "4096")]:
        rc, err = call(rects=rects, **kw)
        assert rc == VJ_ERR_LIMIT and word in err, kw
    rc, err = call(images=ok + [_YuvImage(d, d + 64, None, 65536, 2, 65536, 65536, 0, 1)])
    assert rc == VJ_ERR_LIMIT and "65534" in err
    assert call(rects=[])[0] == 0
    assert f(env._h, None, 0, None, 0, C.byref(PaintParams(3, 0, 1.0, 1.0, 0.0, 0, 0.25))) == 0
    # and the environment still paints
    rc, err = call(expect_unchanged=False, size=5)
    assert rc == 0, err
    want = pyc.restate([yc.unstack(dsrc, yc.NV12), yc.unstack(hsrc, yc.I420)], [yc.NV12, yc.I420], good, "blur", size=5)
    assert np.array_equal(dev.cpu().numpy(), yc.stacked(want[0], yc.NV12)) and np.array_equal(host, yc.stacked(want[1], yc.I420))
    with pytest.raises(VjError) as ei:
        env.paint_yuv(host, [(0, 0, 0, 4, 4)], "blur", size=999, layout="i420")
    assert ei.value.code == VJ_ERR_LIMIT
