"""vj_paint_layout through ctypes (host only, no device): the clipped rectangles, the sizes and the scratch bytes of every mode
against the restatement (tests/paint_cases.py), every argument error with its message, every limit at its bound and one above it.
And the premises of tests/test_gpu_paint.py, with the restatement alone: its cases tell the wrong readings of the definition —
lowest index wins, sequential painting, truncation, the border replicated at the frame instead of K — from the right one."""
import ctypes as C
import math

import numpy as np
import pytest

import extract_cases as ec
import paint_cases as pcs
from clfacedetection_amd import (PaintParams, VJ_PAINT_BLUR, VJ_PAINT_ELLIPSE, VJ_PAINT_FILL, VJ_PAINT_OUTLINE, VJ_PAINT_PIXELATE, VjError,
                                 paint_layout)
from clfacedetection_amd.api import _Image

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(1 << 16, np.uint8)


def image(w, h, ch=1, stride=None, data=True, on_device=0, at=0):
    """A frame record; the layout never reads the pixels.  `at`: the frame's place, so that the frames of a call do not overlap."""
    return _Image(PX.ctypes.data + at * 8192 if data else None, w, h, w * max(ch, 1) if stride is None else stride, on_device, ch)


def layout(lib, images, rects, **kw):
    """-> (rc, K rows as tuples, sizes, scratch bytes, last error)"""
    p = PaintParams()
    lib.vj_paint_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    n = len(images)
    arr = (_Image * max(n, 1))(*images)
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5))
    k = np.full((max(len(r), 1), 5), -7, np.int32)
    s = np.full(max(len(r), 1), -7, np.int32)
    nbytes = C.c_uint64(12345)
    rc = lib.vj_paint_layout(arr, n, r.ctypes.data, len(r), C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(nbytes))
    return rc, [tuple(int(v) for v in row) for row in k[:len(r)]], [int(v) for v in s[:len(r)]], int(nbytes.value), lib.vj_last_error().decode()


def test_default(lib):
    p = PaintParams(1, 2, 3.0, 4.0, 5.0, 6, 7.0, (C.c_uint8 * 4)(1, 2, 3, 4), 9)
    lib.vj_paint_default(C.byref(p))
    assert (p.mode, p.flags, p.sx, p.sy, p.margin, p.size, p.rel, list(p.color), p.reserved) == (VJ_PAINT_BLUR, 0, 1.0, 1.0, 0.0, 0, 0.25, [0] * 4, 0)
    assert (VJ_PAINT_FILL, VJ_PAINT_OUTLINE, VJ_PAINT_PIXELATE, VJ_PAINT_BLUR, VJ_PAINT_ELLIPSE) == (0, 1, 2, 3, 1)
    lib.vj_paint_default(None)


@pytest.mark.parametrize("mode", ["fill", "outline", "pixelate", "blur"])
def test_layout_gives_the_restatements_rectangles_sizes_and_scratch(lib, mode):
    frames = pcs.sources(3) + [pcs.wide_frame()]
    ims = [image(pcs.W, pcs.H, 1, at=0), image(pcs.W, pcs.H, 3, stride=pcs.W * 3 + 5, at=1), image(pcs.W, pcs.H, 4, at=2), image(300, 40, 3, at=3)]
    rects = [(i,) + r[1:] for i in range(3) for r in pcs.SMALL_RECTS + pcs.WHOLE] + [(3, -5, -5, 400, 20), (3, 10, 3, 257, 33), (3, 299, 39, 5, 5)]
    for kw in [dict(), dict(size=1), dict(size=2), dict(size=6), dict(size=7), dict(rel=0.5), dict(rel=1e-9), dict(rel=0.3, sx=1.5, sy=0.5, margin=0.25),
               dict(size=64 if mode != "blur" else 255), dict(rel=3.0)]:
        rc, k, s, nbytes, err = layout(lib, ims, rects, mode=pcs.MODES[mode], **kw)
        assert rc == 0, err
        rk = dict(size=kw.get("size", 0), rel=kw.get("rel", 0.25), scale=(kw.get("sx", 1.0), kw.get("sy", 1.0)), margin=kw.get("margin", 0.0))
        wk, ws, wb = pcs.layout(frames, rects, mode, **rk)
        assert k == [tuple(r) for r in wk.tolist()] and s == ws.tolist() and nbytes == wb, (mode, kw)
        assert (nbytes > 0) == (mode in ("pixelate", "blur"))
    # BLUR: kk = max(s | 1, 3); PIXELATE, OUTLINE: s; FILL: 0 — and rel: cvRound of the shorter mapped side times rel, at least 1
    want = {"fill": [0] * 4, "outline": [1, 2, 6, 7], "pixelate": [1, 2, 6, 7], "blur": [3, 3, 7, 7]}[mode]
    assert [layout(lib, ims, [(0, 0, 0, 9, 9)], mode=pcs.MODES[mode], size=v)[2][0] for v in (1, 2, 6, 7)] == want
    want = {"fill": 0, "outline": 2, "pixelate": 2, "blur": 3}[mode]                       # 10 * 0.25 = 2.5 -> 2 (the tie to even)
    assert layout(lib, ims, [(0, 0, 0, 30, 10)], mode=pcs.MODES[mode])[2] == [want]
    assert layout(lib, ims, [], mode=pcs.MODES[mode])[:4] == (0, [], [], 0) and layout(lib, [], [], mode=pcs.MODES[mode])[0] == 0


def test_the_python_twin():
    frames = pcs.sources(4)
    rects = np.array([(0, 5, 7, 50, 7), (2, -1, 3, 4, 3), (1, 90, 3, 4, 3)], np.int32)
    k, s, nbytes = paint_layout(frames, rects, "blur", size=4)
    assert k.tolist() == [[0, 5, 7, 32, 7], [2, 0, 3, 3, 3], [1, 0, 0, 0, 0]] and s.tolist() == [5, 5, 5] and nbytes == 2 * 32 * 7 + 80
    k, s, nbytes = paint_layout(np.stack([frames[1], frames[1]]), rects[:1], "pixelate", rel=0.5, color=True)
    assert k.tolist() == [[0, 5, 7, 32, 7]] and s.tolist() == [4] and nbytes == 48                # 8 x 2 cells of 3 channels
    with pytest.raises(VjError):
        paint_layout(frames, rects, "blur", size=-1)
    with pytest.raises(ValueError):
        paint_layout(frames, rects, "smear")
    ro = frames[0].copy()
    ro.setflags(write=False)
    for bad in (ro, frames[0].astype(np.float32), frames[0][:, ::2]):
        with pytest.raises(ValueError):
            paint_layout([bad], rects[:1])


def test_argument_errors(lib):
    ok = [image(8, 4, at=0), image(5, 3, at=1)]
    good = [(0, 0, 0, 4, 4), (1, 1, 1, 2, 2)]
    p = PaintParams()
    lib.vj_paint_default(C.byref(p))
    arr = (_Image * 2)(*ok)
    r = np.array(good, np.int32)
    k, s, n = np.zeros((2, 5), np.int32), np.zeros(2, np.int32), C.c_uint64(0)
    f = lib.vj_paint_layout
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(n)) == 0
    assert f(None, 2, r.ctypes.data, 2, C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, None, 2, C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, None, k.ctypes.data, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), None, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), k.ctypes.data, None, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), k.ctypes.data, s.ctypes.data, None) == VJ_ERR_ARG
    assert f(arr, -1, r.ctypes.data, 2, C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, -1, C.byref(p), k.ctypes.data, s.ctypes.data, C.byref(n)) == VJ_ERR_ARG
    assert "null" in lib.vj_last_error().decode()
    # a bad frame, by vj_detect_mixed's rules: the frame is named
    for bad in (image(8, 4, data=False), image(0, 4, at=2), image(8, -1, at=2), image(8, 4, stride=7, at=2), image(8, 4, 3, stride=23, at=2),
                image(8, 4, 2, stride=16, at=2)):
        rc, _, _, nbytes, err = layout(lib, ok + [bad], good)
        assert rc == VJ_ERR_ARG and "frame 2" in err and nbytes == 0
    # a region's frame index out of range, w <= 0, h <= 0: the row is named
    for bad in ((2, 0, 0, 4, 4), (-1, 0, 0, 4, 4), (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (1, 0, 0, -3, 4), (1, 0, 0, 4, -3)):
        rc, _, _, nbytes, err = layout(lib, ok, good + [bad])
        assert rc == VJ_ERR_ARG and "region 2" in err and nbytes == 0, bad
    # the fields: the field is named
    for kw, word in [(dict(mode=4), "mode"), (dict(mode=-1), "mode"), (dict(flags=2), "flags"), (dict(flags=1 | 1 << 31), "flags"),
                     (dict(reserved=1), "reserved"), (dict(size=-1), "size"),
                     (dict(rel=0.0), "rel"), (dict(rel=-0.25), "rel"), (dict(rel=math.nan), "rel"), (dict(rel=math.inf), "rel"),
                     (dict(sx=-0.5), "sx"), (dict(sy=-0.5), "sy"), (dict(margin=-0.1), "margin"), (dict(sx=math.inf), "sx"),
                     (dict(sy=math.nan), "sy"), (dict(margin=math.nan), "margin")]:
        for mode in range(4):
            rc, _, _, nbytes, err = layout(lib, ok, good, **dict(dict(mode=mode), **kw))
            assert rc == VJ_ERR_ARG and word in err and nbytes == 0, (kw, mode)
    assert layout(lib, ok, [], reserved=1)[0] == VJ_ERR_ARG                              # ... also without any region
    assert layout(lib, ok, good, size=3, rel=-1.0)[0] == 0                               # rel is not read when size is given
    # two frames of the call whose memory overlaps, host or device, by one byte; the same frame twice
    for dev in (0, 1):
        a = image(8, 4, stride=10, on_device=dev)                                        # bytes [0, 38)
        for other, bad in ((_Image(PX.ctypes.data + 38, 8, 4, 8, dev, 1), False), (_Image(PX.ctypes.data + 37, 8, 4, 8, dev, 1), True),
                           (a, True), (_Image(PX.ctypes.data + 9, 1, 1, 1, dev, 1), True), (_Image(PX.ctypes.data + 37, 8, 4, 8, 1 - dev, 1), False)):
            rc, _, _, _, err = layout(lib, [image(5, 3, at=3), a, other], [(1, 0, 0, 4, 4)])
            assert (rc == VJ_ERR_ARG and "overlaps" in err and "frame 2" in err and "frame 1" in err) if bad else rc == 0, (dev, err)


def test_limits(lib):
    U = pcs.units_header()
    side, kk, cell = U["PAINT_MAX_SIDE"], U["PAINT_MAX_KK"], U["PAINT_MAX_CELL"]
    assert (side, kk, cell) == (32767, 255, 4096)
    ims = [image(8, 4)]
    # vj_extract's mapping limits
    assert layout(lib, ims, [(0, -(1 << 24), 1 << 23, 1, 1)])[0] == 0
    for rects, kw, word in [([(0, 0, 0, 65536, 4)], {}, "65535"), ([(0, 0, 0, 4, 4)], dict(sy=1e300), "65535"), ([(0, 0, 0, 4, 4)], dict(margin=1e300), "65535"),
                            ([(0, (1 << 24) + 1, 0, 4, 4)], {}, "2^24"), ([(0, 1 << 23, 0, 4, 4)], dict(sx=3.0), "2^24")]:
        rc, _, _, _, err = layout(lib, ims, [(0, 0, 0, 2, 2)] + rects, size=3, **kw)
        assert rc == VJ_ERR_LIMIT and word in err, (rects, kw)
    # a mapped side: 32767 passes, 32768 is refused, the region is named; the margin counts
    for mode in range(4):
        assert layout(lib, ims, [(0, 0, 0, side, side)], mode=mode, size=3)[0] == 0
        for bad, kw in (((0, 0, 0, side + 1, 4), {}), ((0, 0, 0, 4, side + 1), {}), ((0, 0, 0, side - 1, 4), dict(margin=0.0001)), ((0, 0, 0, 20000, 4), dict(sx=2.0))):
            rc, _, _, _, err = layout(lib, ims, [(0, 0, 0, 2, 2), bad], mode=mode, size=3, **kw)
            assert rc == VJ_ERR_LIMIT and "32767" in err and "region 1" in err, (mode, bad)
    # BLUR: kk = 255 passes (size 254 and 255), 257 is refused; by rel too: 1020 * 0.25 = 255, 1028 * 0.25 = 257
    assert [layout(lib, ims, [(0, 0, 0, 9, 9)], size=v)[2] for v in (kk - 1, kk)] == [[kk], [kk]]
    assert layout(lib, ims, [(0, 0, 0, 1020, 2000)])[2] == [kk]
    for rects, kw in (([(0, 0, 0, 9, 9)], dict(size=kk + 1)), ([(0, 0, 0, 2000, 1028)], {}), ([(0, 0, 0, 9, 9)], dict(rel=1e300))):
        rc, _, _, _, err = layout(lib, ims, [(0, 0, 0, 2, 2)] + rects, **dict(dict(size=3), **kw)) if "size" in kw else layout(lib, ims, rects, **kw)
        assert rc == VJ_ERR_LIMIT and "255" in err and "region" in err, (rects, kw)
    assert layout(lib, ims, [(0, 0, 0, 9, 9)], size=kk + 1, mode=VJ_PAINT_OUTLINE)[0] == 0     # the other modes do not have this limit
    # PIXELATE: s = 4096 passes, 4097 is refused
    assert layout(lib, ims, [(0, 0, 0, 9, 9)], mode=VJ_PAINT_PIXELATE, size=cell)[2] == [cell]
    rc, _, _, _, err = layout(lib, ims, [(0, 0, 0, 9, 9)], mode=VJ_PAINT_PIXELATE, size=cell + 1)
    assert rc == VJ_ERR_LIMIT and "4096" in err and "region 0" in err
    assert layout(lib, ims, [(0, 0, 0, 9, 9)], mode=VJ_PAINT_OUTLINE, size=1 << 30)[0] == 0
    assert layout(lib, ims, [(0, 0, 0, 9, 9)], mode=VJ_PAINT_OUTLINE, rel=1e300)[:3] == (0, [(0, 0, 0, 8, 4)], [65536])
    # work units beyond a 32-bit index: K of 32767 x 32767 x 4 bytes is 512 blocks of 64 slots x 1024 blocks of 32 rows = 2^19 units
    big = [_Image(PX.ctypes.data, side, side, side * 4, 0, 4)]
    per = (((side * 4 + 6) // 4 + U["PAINT_BLOCK_SLOTS"] - 1) // U["PAINT_BLOCK_SLOTS"]) * ((side + U["PAINT_BLOCK_H"] - 1) // U["PAINT_BLOCK_H"])
    assert per == 1 << 19
    fit = (2 ** 31 - 1) // per
    assert layout(lib, big, [(0, 0, 0, side, side)] * fit, mode=VJ_PAINT_FILL)[0] == 0
    rc, _, _, _, err = layout(lib, big, [(0, 0, 0, side, side)] * (fit + 1), mode=VJ_PAINT_FILL)
    assert rc == VJ_ERR_LIMIT and "work units" in err


# --------------------------------------------------------------------------------------------------- the premises of the GPU tests
def test_fill_pixelate_1_and_blur_of_a_constant_are_what_they_must_be():
    src = pcs.sources(21)
    for f, o in zip(src, pcs.restate(src, [(i, 0, 0, pcs.W, pcs.H) for i in range(3)], "fill", fill=pcs.FILL_COLOR)):
        assert np.array_equal(o.reshape(pcs.H, pcs.W, -1), np.broadcast_to(np.array(pcs.FILL_COLOR[:o.reshape(pcs.H, pcs.W, -1).shape[2]], np.uint8), (pcs.H, pcs.W, o.reshape(pcs.H, pcs.W, -1).shape[2])))
    rects = [(i,) + r[1:] for i in range(3) for r in pcs.SMALL_RECTS + pcs.WHOLE]
    for f, o in zip(src, pcs.restate(src, rects, "pixelate", size=1)):                       # PIXELATE with s = 1 is the identity
        assert np.array_equal(f, o)
    const = [np.full_like(f, 77) for f in src]
    const[1][5:20, 3:30] = 200                                                               # BLUR of a constant region is the identity
    out = pcs.restate(const, [(i, 3, 5, 27, 15) for i in range(3)] + [(1, 0, 0, 3, 5)], "blur", size=15)
    assert all(np.array_equal(a, b) for a, b in zip(const, out))


def test_blur_255_on_20_by_17_has_every_tap_clamped():
    """kk = 255, r = 127: every window covers the whole 20 x 17 region and more, so every pixel is the weighted sum in which
    column x counts 128 - x times if x == 0, 108 + x if x == 19 ... : restated directly."""
    f = ec.edge_frame(3)
    _, x, y, w, h = ec.EDGE_RECT
    out = pcs.restate([f], [ec.EDGE_RECT], "blur", size=255)[0]
    crop = f[y:y + h, x:x + w].astype(np.int64)
    want = np.zeros_like(crop)
    for py in range(h):
        wy = np.bincount(np.clip(np.arange(py - 127, py + 128), 0, h - 1), minlength=h)
        for px in range(w):
            wx = np.bincount(np.clip(np.arange(px - 127, px + 128), 0, w - 1), minlength=w)
            want[py, px] = ((crop * wy[:, None, None] * wx[None, :, None]).sum(axis=(0, 1)) + 255 * 255 // 2) // (255 * 255)
    assert np.array_equal(out[y:y + h, x:x + w], want) and int(want.max()) <= 60
    rest = out.copy()
    rest[y:y + h, x:x + w] = f[y:y + h, x:x + w]
    assert np.array_equal(rest, f)


@pytest.mark.parametrize("mode", ["pixelate", "blur"])
def test_the_overlap_case_tells_the_wrong_orders_apart(mode):
    src = pcs.sources(22)
    right = pcs.restate(src, pcs.OVERLAP_RECTS, mode, rel=0.3)
    assert not np.array_equal(right[0], pcs.restate(src, pcs.OVERLAP_RECTS, mode, rel=0.3, winner="first")[0])     # lowest index wins
    assert not np.array_equal(right[0], pcs.restate(src, pcs.OVERLAP_RECTS, mode, rel=0.3, sequential=True)[0])    # reads painted pixels
    nested = [(0, 3, 2, 30, 24), (0, 8, 6, 18, 14)]
    a, b = pcs.restate(src, nested, mode, rel=0.25, ellipse=True)[0], pcs.restate(src, nested, mode, rel=0.25)[0]
    assert not np.array_equal(a[6:8, 8:10], b[6:8, 8:10])                     # the later ellipse leaves the earlier region its corners


@pytest.mark.parametrize("mode", ["pixelate", "blur"])
def test_the_rounding_case_tells_truncation_apart(mode):
    for src in pcs.sources(21):
        for size in (2, 7) if mode == "pixelate" else (3, 5):
            right = pcs.restate([src], pcs.ROUNDING_RECT, mode, size=size)[0]
            assert not np.array_equal(right, pcs.restate([src], pcs.ROUNDING_RECT, mode, size=size, truncate=True)[0])


def test_the_edge_frame_tells_the_two_clamps_apart():
    for ch in (1, 3, 4):
        f = ec.edge_frame(ch)
        at_k = pcs.restate([f], [ec.EDGE_RECT], "blur", size=5)[0]
        at_frame = pcs.restate([f], [ec.EDGE_RECT], "blur", size=5, clamp="frame")[0]
        _, x, y, w, h = ec.EDGE_RECT
        assert not np.array_equal(at_k, at_frame)
        assert np.array_equal(at_k[y + 2:y + h - 2, x + 2:x + w - 2], at_frame[y + 2:y + h - 2, x + 2:x + w - 2])   # the interior agrees
        assert int(at_k[y:y + h, x:x + w].max()) <= 60 < int(at_frame[y:y + h, x:x + w].max())                     # the neighbours leak in


def test_the_ellipse_has_the_counted_pixels():
    for (w, h), n in pcs.ELLIPSE_COUNTS.items():
        for x0, y0 in ((0, 0), (5, 3), (-2, -1)):
            m = pcs.painted(pcs.FILL, (x0, y0, w, h), (x0, y0, x0 + w, y0 + h), 0, True)
            assert int(m.sum()) == n and np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1]), (w, h)
    # the outline of an ellipse: the shape minus the shape of the rectangle shrunk by t; a shrunk side <= 0: the whole shape
    full = pcs.painted(pcs.OUTLINE, (0, 0, 9, 7), (0, 0, 9, 7), 4, True)
    assert np.array_equal(full, pcs.painted(pcs.FILL, (0, 0, 9, 7), (0, 0, 9, 7), 0, True))
    ring = pcs.painted(pcs.OUTLINE, (0, 0, 9, 7), (0, 0, 9, 7), 2, True)
    assert ring.sum() == full.sum() - pcs.painted(pcs.FILL, (2, 2, 5, 3), (0, 0, 9, 7), 0, True).sum() and not ring[3, 4] and ring[3, 0]
