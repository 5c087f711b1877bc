"""vj_paint_yuv_layout through ctypes (host only, no device): K, Kc, the sizes and the scratch bytes of every mode and layout against
the restatement (tests/paint_yuv_cases.py), every argument error with its message, every limit at its bound and one above it.  And
the premises of tests/test_gpu_paint_yuv.py, with the restatement alone: its cases tell the wrong readings of the definition from the
right one, and cover the parities and the widths the kernels' constants make interesting."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import paint_cases as pcs
import paint_yuv_cases as pyc
import yuv_cases as yc
from clfacedetection_amd import PaintParams, VjError, paint_yuv_layout
from clfacedetection_amd.api import _YuvImage

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(1 << 20, np.uint8)


def image(w, h, lay=yc.NV12, at=0, y_stride=None, c_stride=None, y=True, c0=True, c1=True, on_device=0):
    """A frame record; the layout never reads the pixels.  `at`: the frame's place, so that the planes of a call do not overlap."""
    base = PX.ctypes.data + at * (1 << 17)
    ys = w if y_stride is None else y_stride
    cs = (w // 2 if lay == yc.I420 else w) if c_stride is None else c_stride
    py = base
    p0 = py + max(ys, 1) * max(h, 1)
    p1 = p0 + max(cs, 1) * max(h // 2, 1)
    return _YuvImage(py if y else None, p0 if c0 else None, p1 if (c1 and lay == yc.I420) else None, w, h, ys, cs, lay, on_device)


def layout(lib, images, rects, **kw):
    """-> (rc, K rows, Kc rows, sizes, chroma sizes, scratch bytes, last error)"""
    p = PaintParams()
    lib.vj_paint_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    n = len(images)
    arr = (_YuvImage * max(n, 1))(*images)
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5))
    m = max(len(r), 1)
    k, kc = np.full((m, 5), -7, np.int32), np.full((m, 5), -7, np.int32)
    s, cs = np.full(m, -7, np.int32), np.full(m, -7, np.int32)
    nbytes = C.c_uint64(12345)
    rc = lib.vj_paint_yuv_layout(arr, n, r.ctypes.data, len(r), C.byref(p), k.ctypes.data, kc.ctypes.data, s.ctypes.data, cs.ctypes.data, C.byref(nbytes))
    rows = lambda a: [tuple(int(v) for v in row) for row in a[:len(r)]]
    return rc, rows(k), rows(kc), [int(v) for v in s[:len(r)]], [int(v) for v in cs[:len(r)]], int(nbytes.value), lib.vj_last_error().decode()


@pytest.mark.parametrize("lay", pyc.LAYOUTS)
@pytest.mark.parametrize("mode", ["fill", "outline", "pixelate", "blur"])
def test_layout_gives_the_restatements_rectangles_sizes_and_scratch(lib, mode, lay):
    sizes = [(pyc.W, pyc.H), (2, 2), (pyc.WIDE_W, pyc.WIDE_H)]
    ims = [image(w, h, lay, at=i, y_stride=w + 3 * i, c_stride=w + 8) for i, (w, h) in enumerate(sizes)]
    rects = pyc.SMALL_RECTS + pyc.WHOLE + [(1,) + r[1:] for r in pyc.TINY_RECTS] + [(2,) + r[1:] for r in pyc.wide_rects()]
    for kw in [dict(), dict(size=1), dict(size=2), dict(size=6), dict(size=7), dict(rel=0.5), dict(rel=1e-9), dict(rel=0.3, sx=1.5, sy=0.5, margin=0.25),
               dict(size=64 if mode != "blur" else 255), dict(rel=3.0)]:
        rc, k, kc, s, cs, nbytes, err = layout(lib, ims, rects, mode=pcs.MODES[mode], **kw)
        assert rc == 0, err
        rk = dict(size=kw.get("size", 0), rel=kw.get("rel", 0.25), scale=(kw.get("sx", 1.0), kw.get("sy", 1.0)), margin=kw.get("margin", 0.0))
        wk, wkc, ws, wcs, wb = pyc.layout(sizes, rects, mode, **rk)
        assert k == [tuple(r) for r in wk.tolist()] and kc == [tuple(r) for r in wkc.tolist()], (mode, kw)
        assert s == ws.tolist() and cs == wcs.tolist() and nbytes == wb, (mode, kw)
        assert (nbytes > 0) == (mode in ("pixelate", "blur"))
    # the chroma sizes: sc = (s + 1) >> 1; kkc = max((kk >> 1) | 1, 3); OUTLINE keeps t; FILL 0
    want = {"fill": [0] * 5, "outline": [1, 2, 6, 7, 31], "pixelate": [1, 1, 3, 4, 16], "blur": [3, 3, 3, 3, 15]}[mode]
    assert [layout(lib, ims, [(0, 0, 0, 9, 9)], mode=pcs.MODES[mode], size=v)[4][0] for v in (1, 2, 6, 7, 31)] == want
    assert layout(lib, ims, [], mode=pcs.MODES[mode])[:6] == (0, [], [], [], [], 0) and layout(lib, [], [], mode=pcs.MODES[mode])[0] == 0


def test_the_python_twin():
    a = np.zeros((3, 45, 38), np.uint8)
    rects = np.array([(0, 5, 7, 50, 7), (2, -1, 3, 4, 3), (1, 90, 3, 4, 3)], np.int32)
    k, kc, s, cs, nbytes = paint_yuv_layout(a, rects, "blur", size=9)
    assert k.tolist() == [[0, 5, 7, 33, 7], [2, 0, 3, 3, 3], [1, 0, 0, 0, 0]] and kc.tolist() == [[0, 2, 3, 17, 4], [2, 0, 1, 2, 2], [1, 0, 0, 0, 0]]
    assert s.tolist() == [9, 9, 9] and cs.tolist() == [5, 5, 5] and nbytes == (2 * 33 * 7 + 2) + 2 * (2 * 17 * 4 + 8) + 32 + 2 * 16
    for lay in ("nv21", "i420"):
        assert paint_yuv_layout([a[0], a[1:]], rects, "blur", size=9, layout=lay)[4] == nbytes
    with pytest.raises(VjError):
        paint_yuv_layout(a, rects, "blur", size=-1)
    with pytest.raises(ValueError):
        paint_yuv_layout(a, rects, "smear")
    ro = a.copy()
    ro.setflags(write=False)
    for bad in (ro, a.astype(np.float32), a[:, :, ::2]):
        with pytest.raises(ValueError):
            paint_yuv_layout(bad, rects[:1])
    with pytest.raises(ValueError):
        paint_yuv_layout(np.zeros((45, 40), np.uint8)[:, :38], rects[:1], layout="i420")     # a copy would be needed
    paint_yuv_layout(np.zeros((45, 40), np.uint8)[:, :38], rects[:1], layout="nv12")          # a strided view is painted in place


def test_argument_errors(lib):
    def err(images, rects=((0, 0, 0, 4, 4),), **kw):
        rc, *_, nbytes, msg = layout(lib, images, rects, **kw)
        assert nbytes == (0 if rc else nbytes)
        return rc, msg

    ok = [image(8, 4, at=0), image(6, 2, yc.I420, at=1)]
    assert err(ok)[0] == 0
    p = PaintParams()
    lib.vj_paint_default(C.byref(p))
    arr = (_YuvImage * 2)(*ok)
    r = np.array([(0, 0, 0, 4, 4), (1, 1, 1, 2, 2)], np.int32)
    k, kc, s, cs, n = np.zeros((2, 5), np.int32), np.zeros((2, 5), np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), C.c_uint64(0)
    f = lib.vj_paint_yuv_layout
    good = [arr, 2, r.ctypes.data, 2, C.byref(p), k.ctypes.data, kc.ctypes.data, s.ctypes.data, cs.ctypes.data, C.byref(n)]
    assert f(*good) == 0
    for i in (0, 2, 4, 5, 6, 7, 8, 9):
        assert f(*[None if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG and "null" in lib.vj_last_error().decode()
    for i in (1, 3):
        assert f(*[-1 if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG
    # the frame errors of vj_yuv_to_bgr: the frame is named
    for bad, word in [(image(8, 4, y=False, at=2), "null y plane"), (image(8, 4, c0=False, at=2), "null c0 plane"),
                      (image(8, 4, yc.I420, c1=False, at=2), "null c1 plane"), (image(0, 4, at=2), "must be positive"), (image(8, -2, at=2), "must be positive"),
                      (image(7, 4, at=2), "must be even"), (image(8, 3, at=2), "must be even"), (image(8, 4, y_stride=7, at=2), "y_stride"),
                      (image(8, 4, c_stride=7, at=2), "c_stride"), (image(8, 4, yc.I420, c_stride=3, at=2), "c_stride"), (image(8, 4, 3, at=2), "unknown layout")]:
        rc, msg = err([ok[0], bad])
        assert rc == VJ_ERR_ARG and "frame 1" in msg and word in msg, msg
    # the region and parameter errors of vj_paint
    for rects, word in [([(2, 0, 0, 4, 4)], "region 0: frame 2"), ([(0, 0, 0, 4, 4), (-1, 0, 0, 4, 4)], "region 1: frame -1"), ([(0, 0, 0, 0, 4)], "must be positive"),
                        ([(0, 0, 0, 4, -1)], "must be positive")]:
        rc, msg = err(ok, rects)
        assert rc == VJ_ERR_ARG and word in msg, msg
    for kw, word in [(dict(mode=4), "unknown mode"), (dict(mode=-1), "unknown mode"), (dict(flags=2), "unknown bits"), (dict(reserved=1), "reserved"),
                     (dict(size=-1), "size"), (dict(sx=-1.0), "sx"), (dict(sy=float("nan")), "sy"), (dict(margin=float("inf")), "margin"),
                     (dict(rel=0.0), "rel"), (dict(rel=float("nan")), "rel")]:
        rc, msg = err(ok, **kw)
        assert rc == VJ_ERR_ARG and word in msg, (kw, msg)
    # any two planes of the call whose byte extents overlap, planes of one frame included
    a = image(8, 4, at=3)
    same_frame = _YuvImage(a.y, a.y + 8, None, 8, 4, 8, 8, yc.NV12, 0)              # the pair plane begins inside the Y plane
    rc, msg = err([same_frame])
    assert rc == VJ_ERR_ARG and "frame 0" in msg and "c0 plane overlaps frame 0's y plane" in msg, msg
    b = _YuvImage(a.c0 + 15, a.c0 + 64, None, 8, 4, 8, 8, yc.NV12, 0)               # its Y plane begins on the last byte of a's pair plane
    rc, msg = err([a, b])
    assert rc == VJ_ERR_ARG and "frame 1" in msg and "y plane overlaps frame 0's c0 plane" in msg, msg
    b = _YuvImage(a.c0 + 16, a.c0 + 64, None, 8, 4, 8, 8, yc.NV12, 0)               # one byte later: they only touch
    assert err([a, b])[0] == 0
    i = image(8, 4, yc.I420, at=4)
    rc, msg = err([_YuvImage(i.y, i.c0, i.c0 + 3, 8, 4, 8, 4, yc.I420, 0)])
    assert rc == VJ_ERR_ARG and "c1 plane overlaps frame 0's c0 plane" in msg, msg
    assert err([a, _YuvImage(a.y, a.c0, None, 8, 4, 8, 8, yc.NV12, 1)])[0] == 0      # a host frame and a device frame live in two address spaces


def test_limits_at_the_bound_and_one_past_it(lib):
    def rc_of(images, rects, **kw):
        rc, *_, msg = layout(lib, images, rects, **kw)
        return rc, msg
    # a side of 65534 passes, 65536 is refused (65535 is odd: VJ_ERR_ARG)
    assert rc_of([image(65534, 2, at=0)], [(0, 0, 0, 4, 2)])[0] == 0
    rc, msg = rc_of([image(65536, 2, at=0)], [(0, 0, 0, 4, 2)])
    assert rc == VJ_ERR_LIMIT and "65534" in msg
    rc, msg = rc_of([image(2, 65536, at=0, y_stride=2, c_stride=2)], [(0, 0, 0, 2, 2)])
    assert rc == VJ_ERR_LIMIT and "65534" in msg
    big = [image(40000, 2, at=0)]
    # vj_paint's limits: a mapped side of 32767 / 32768; kk 255 / 257; s 4096 / 4097
    assert rc_of(big, [(0, 0, 0, 32767, 2)], mode=pyc.FILL)[0] == 0
    rc, msg = rc_of(big, [(0, 0, 0, 32768, 2)], mode=pyc.FILL)
    assert rc == VJ_ERR_LIMIT and "32767" in msg
    assert rc_of(big, [(0, 0, 0, 300, 2)], mode=pyc.BLUR, size=255)[0] == 0
    rc, msg = rc_of(big, [(0, 0, 0, 300, 2)], mode=pyc.BLUR, size=256)
    assert rc == VJ_ERR_LIMIT and "255" in msg
    assert rc_of(big, [(0, 0, 0, 300, 2)], mode=pyc.PIXELATE, size=4096)[0] == 0
    rc, msg = rc_of(big, [(0, 0, 0, 300, 2)], mode=pyc.PIXELATE, size=4097)
    assert rc == VJ_ERR_LIMIT and "4096" in msg


# ------------------------------------------------------------------------------------------------ the premises, restatement alone
def small(lay, seed=3):
    return [pyc.frame(pyc.W, pyc.H, lay, seed)]


@pytest.mark.parametrize("lay", pyc.LAYOUTS)
def test_each_wrong_reading_differs_on_the_case_meant_to_catch_it(lay):
    fr = small(lay)
    cases = {"top_left": (pyc.SMALL_RECTS, "fill", {}), "luma_sizes": (pyc.ROUNDING_RECT, "blur", dict(size=9)),
             "k_lists": (pyc.SHARED_RECTS, "pixelate", dict(size=3)), "sequential": (pyc.OVERLAP_RECTS, "blur", dict(size=5)),
             "frame_clamp": (pyc.ROUNDING_RECT, "blur", dict(size=7)), "swap_uv": (pyc.ROUNDING_RECT, "fill", {}),
             "truncate": (pyc.ROUNDING_RECT, "pixelate", dict(size=3))}
    assert sorted(cases) == sorted(pyc.VARIANTS)
    for variant, (rects, mode, kw) in cases.items():
        src = [pyc.smooth_frame(pyc.W, pyc.H, lay, 9)] if variant == "truncate" else fr
        right = pyc.restate(src, lay, rects, mode, fill=pyc.FILL_BGR, **kw)
        wrong = pyc.restate(src, lay, rects, mode, fill=pyc.FILL_BGR, variant=variant, **kw)
        assert not pyc.same(right, wrong), variant
        # and in the chroma planes, not only in Y
        assert any(not np.array_equal(a, b) for p, q in zip(right, wrong) for a, b in zip(p[1:], q[1:])), variant
    assert not pyc.same(pyc.restate(fr, lay, pyc.ROUNDING_RECT, "pixelate", size=2), pyc.restate(fr, lay, pyc.ROUNDING_RECT, "pixelate", size=2, variant="luma_sizes"))


@pytest.mark.parametrize("lay", pyc.LAYOUTS)
def test_fill_of_the_whole_frame_is_the_encoded_constant_image(lay):
    got = pyc.restate(small(lay), lay, pyc.WHOLE, "fill", fill=pyc.FILL_BGR)
    img = np.broadcast_to(np.array(pyc.FILL_BGR, np.uint8), (pyc.H, pyc.W, 3))
    assert pyc.same(got, [yc.encode(img, lay)])
    assert pyc.color_of((0, 0, 0)) == (16, 128, 128) and pyc.color_of((255, 255, 255)) == (235, 128, 128) and pyc.color_of((255, 0, 0)) == (41, 240, 110)


@pytest.mark.parametrize("lay", pyc.LAYOUTS)
def test_identities(lay):
    fr = small(lay)
    assert pyc.same(pyc.restate(fr, lay, pyc.SMALL_RECTS + pyc.WHOLE, "pixelate", size=1), fr)
    const = [yc.join_chroma(np.full((pyc.H, pyc.W), 77, np.uint8), np.full((pyc.H // 2, pyc.W // 2), 33, np.uint8), np.full((pyc.H // 2, pyc.W // 2), 201, np.uint8), lay)]
    for kk in (3, 15, 255):
        assert pyc.same(pyc.restate(const, lay, pyc.SMALL_RECTS + pyc.WHOLE, "blur", size=kk), const)
    assert pyc.same(pyc.restate(fr, lay, [], "blur"), fr) and pyc.same(pyc.restate(fr, lay, [(0, 100, 100, 5, 5)], "fill"), fr)


def test_the_shared_sample_takes_the_later_regions_value():
    fr = small(yc.I420)
    first = pyc.restate(fr, yc.I420, pyc.SHARED_RECTS[:1], "fill", fill=(255, 0, 0))
    both = pyc.restate(fr, yc.I420, [pyc.SHARED_RECTS[0]], "fill", fill=(255, 0, 0))
    assert first[0][1][2, 3] == 240 and both[0][1][2, 3] == 240
    a = pyc.restate(fr, yc.I420, pyc.SHARED_RECTS, "pixelate", size=64)
    only_second = pyc.restate(fr, yc.I420, pyc.SHARED_RECTS[1:], "pixelate", size=64)
    only_first = pyc.restate(fr, yc.I420, pyc.SHARED_RECTS[:1], "pixelate", size=64)
    for pl in (1, 2):
        assert np.array_equal(a[0][pl][2:6, 3], only_second[0][pl][2:6, 3]) and not np.array_equal(a[0][pl][2:6, 3], only_first[0][pl][2:6, 3])
        assert np.array_equal(a[0][pl][2:6, 1:3], only_first[0][pl][2:6, 1:3])
    kc = [pyc.chroma_rect(pcs.clip(ec.map_region(r, (1, 1), 0)[1:], pyc.W, pyc.H)) for r in ec.as_rows(pyc.SHARED_RECTS)]
    assert kc[0][2] == 4 and kc[1][0] == 3                                   # Kc [1, 4) and [3, 6): sample 3 in both


def test_all_parities_and_the_straddled_constants():
    par = set()
    for r in ec.as_rows(pyc.SMALL_RECTS):
        k = pcs.clip(ec.map_region(r, (1, 1), 0)[1:], pyc.W, pyc.H)
        if k:
            par.add(tuple(v & 1 for v in k))
    assert len(par) == 16
    u = pyc.units_header()
    wr, bh = u["PAINT_BLOCK_SLOTS"] * 4, u["PAINT_BLOCK_H"]
    assert (wr, u["PAINT_BAND_COLS"], bh, u["PAINT_BAND_H"], u["PAINT_WAVES"]) == (256, 256, 32, 32, 4)
    luma, pair, planar, rows, crows = set(), set(), set(), set(), set()
    for rects, (w, h) in ((pyc.wide_rects(), (pyc.WIDE_W, pyc.WIDE_H)), (pyc.big_rects(), (pyc.BIG_W, pyc.BIG_H))):
        for r in ec.as_rows(rects):
            k = pcs.clip(ec.map_region(r, (1, 1), 0)[1:], w, h)
            kc = pyc.chroma_rect(k)
            luma.add(k[2] - k[0]), pair.add(2 * (kc[2] - kc[0])), planar.add(kc[2] - kc[0]), rows.add(k[3] - k[1]), crows.add(kc[3] - kc[1])
    for widths in (luma, pair, planar):          # the wave row / the band of byte columns: below, at, above; the lane's 4 bytes likewise
        assert min(w for w in widths if w > 8) < wr and wr in widths and max(widths) > wr, widths
    assert {3, 4, 5} <= luma and {2, 4, 6} <= pair and {2, 3} <= planar
    for hs in (rows, crows):
        assert any(v < bh for v in hs) and bh in hs and any(v > bh for v in hs), hs
    # BLUR's staged prefix: the widest halo (kk = 255 -> 127 samples each side) of a full wave row fits
    assert 256 + 2 * 127 + 1 <= u["PAINT_YUV_PREFIX_MAX"] and (128 + 1 + 2 * 127) * 2 <= u["PAINT_YUV_PREFIX_MAX"]
