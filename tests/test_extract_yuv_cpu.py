"""vj_extract_yuv_layout / vj_extract_affine_yuv_layout through ctypes (host only, no device): the mapped regions, the channel count
and the byte counts for every flag combination against the restated mapping, every argument error with its message, every limit at
its bound and one step past it.  And the premises of tests/test_gpu_extract_yuv.py, with the restatement alone: the tap-by-tap
model says what the definition's sentence says, each wrong reading differs from the right one on the case meant to catch it, alpha
stays 255, the random frames saturate every channel at both ends, and the output sizes straddle the work units' sides."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import affine_cases as ac
import extract_cases as ec
import extract_yuv_cases as eyc
import yuv_cases as yc
from clfacedetection_amd import (AFFINE_DTYPE, AffineParams, ExtractParams, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VJ_YUV_RGB_ORDER, VjError, YuvParams,
                                 extract_affine_yuv_layout, extract_yuv_layout)
from clfacedetection_amd.api import _YuvImage

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(1 << 20, np.uint8)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def image(w, h, lay=yc.NV12, at=0, y_stride=None, c_stride=None, y=True, c0=True, c1=True, on_device=0):
    """A frame record; the layout calls never read the pixels."""
    base = PX.ctypes.data + at * (1 << 17)
    ys = w if y_stride is None else y_stride
    cs = (w // 2 if lay == yc.I420 else w) if c_stride is None else c_stride
    p0 = base + max(ys, 1) * max(h, 1)
    p1 = p0 + max(cs, 1) * max(h // 2, 1)
    return _YuvImage(base if y else None, p0 if c0 else None, p1 if (c1 and lay == yc.I420) else None, w, h, ys, cs, lay, on_device)


def yuv_params(lib, channels=3, flags=0, reserved=0):
    yp = YuvParams()
    lib.vj_yuv_default(C.byref(yp))
    yp.channels, yp.flags, yp.reserved = channels, flags, reserved
    return yp


def layout(lib, images, rects, size=(4, 4), yp=None, **kw):
    """vj_extract_yuv_layout -> (rc, mapped rows, channels, bytes, last error)"""
    p = ExtractParams()
    lib.vj_extract_default(C.byref(p))
    p.out_w, p.out_h = size
    for k, v in kw.items():
        setattr(p, k, v)
    yp = yuv_params(lib) if yp is None else yp
    n = len(images)
    arr = (_YuvImage * max(n, 1))(*images)
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5))
    src = np.full((max(len(r), 1), 5), -7, np.int32)
    ch, nbytes = C.c_int(-7), C.c_uint64(12345)
    rc = lib.vj_extract_yuv_layout(arr, n, r.ctypes.data, len(r), C.byref(p), C.byref(yp), src.ctypes.data, C.byref(ch), C.byref(nbytes))
    return rc, [tuple(int(v) for v in row) for row in src[:len(r)]], int(ch.value), int(nbytes.value), lib.vj_last_error().decode()


def affine_layout(lib, images, rows, size=(4, 4), yp=None, **kw):
    """vj_extract_affine_yuv_layout -> (rc, channels, bytes, last error)"""
    p = AffineParams()
    lib.vj_affine_default(C.byref(p))
    p.out_w, p.out_h = size
    for k, v in kw.items():
        setattr(p, k, v)
    yp = yuv_params(lib) if yp is None else yp
    a = np.zeros(len(rows), AFFINE_DTYPE)
    for i, row in enumerate(rows):
        a[i]["frame"], a[i]["m"] = int(row[0]), row[1:7]
        if len(row) > 7:
            a[i]["reserved"] = row[7]
    n = len(images)
    arr = (_YuvImage * max(n, 1))(*images)
    ch, nbytes = C.c_int(-7), C.c_uint64(12345)
    rc = lib.vj_extract_affine_yuv_layout(arr, n, a.ctypes.data, len(a), C.byref(p), C.byref(yp), C.byref(ch), C.byref(nbytes))
    return rc, int(ch.value), int(nbytes.value), lib.vj_last_error().decode()


OK_FRAMES = lambda: [image(38, 30, yc.NV12, at=0, y_stride=41, c_stride=40), image(8, 4, yc.I420, at=1), image(66, 34, yc.NV21, at=2)]
IDENT = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------- the layouts
def test_both_layouts_give_the_restated_mapping_channels_and_bytes(lib):
    rects = eyc.crops(0) + [(1, 0, 0, 8, 4), (2, 5, 7, 33, 21), (2, -9, 3, 5, 7)]
    rows = [[r[0]] + IDENT for r in rects]
    for kw in [dict(), dict(sx=0.5, sy=0.5), dict(sx=1.8, sy=1.8, margin=0.1), dict(margin=0.25), dict(sx=0.0, sy=0.0)]:
        for f in eyc.FLAG_CASES:
            flags = (VJ_EXTRACT_GRAY if f["gray"] else 0) | (VJ_EXTRACT_PLANAR if f["planar"] else 0)
            yp = yuv_params(lib, 4 if f["alpha"] else 3, VJ_YUV_RGB_ORDER if f["rgb"] else 0)
            want_c = 1 if f["gray"] else 4 if f["alpha"] else 3
            for size in [(1, 1), (7, 3), (64, 34)]:
                rc, src, ch, nbytes, err = layout(lib, OK_FRAMES(), rects, size, yp, flags=flags, **kw)
                assert rc == 0, err
                want = [ec.map_region(r, (kw.get("sx", 1.0), kw.get("sy", 1.0)), kw.get("margin", 0.0)) for r in rects]
                assert src == want and ch == want_c and nbytes == len(rects) * size[0] * size[1] * want_c, (kw, f, size)
                rc, ch, nbytes, err = affine_layout(lib, OK_FRAMES(), rows, size, yp, flags=flags)
                assert rc == 0 and ch == want_c and nbytes == len(rects) * size[0] * size[1] * want_c, (err, f, size)
    assert layout(lib, OK_FRAMES(), [])[:4] == (0, [], 3, 0) and layout(lib, [], [])[0] == 0
    assert affine_layout(lib, OK_FRAMES(), [])[:3] == (0, 3, 0) and affine_layout(lib, [], [])[0] == 0


def test_the_python_twins():
    a = np.zeros((3, 45, 38), np.uint8)
    rects = np.array([(0, 5, 7, 50, 7), (2, -1, 3, 4, 3)], np.int32)
    src, ch, nbytes = extract_yuv_layout(a, rects, (7, 3), margin=0.5)
    assert src.tolist() == [[0, -20, 3, 100, 15], [2, -3, 1, 8, 7]] and (ch, nbytes) == (3, 2 * 7 * 3 * 3)
    assert extract_yuv_layout(a, rects, (7, 3), alpha=True, planar=True)[1:] == (4, 2 * 7 * 3 * 4)
    assert extract_yuv_layout(a, rects, (7, 3), alpha=True, gray=True, layout="i420")[1:] == (1, 2 * 7 * 3)
    assert extract_yuv_layout([(a[0, :30], a[0, 30:])], rects[:1], (7, 3), rgb=True, layout="nv21")[1:] == (3, 63)
    rows = np.array([[0.0] + IDENT, [2.0] + ac.ROT], np.float64)
    assert extract_affine_yuv_layout(a, rows, (33, 21)) == (3, 2 * 33 * 21 * 3)
    assert extract_affine_yuv_layout(a, rows, (33, 21), gray=True, alpha=True) == (1, 2 * 33 * 21)
    assert extract_affine_yuv_layout(a, rows, (33, 21), alpha=True, planar=True, layout="i420") == (4, 2 * 33 * 21 * 4)
    with pytest.raises(VjError):
        extract_yuv_layout(a, [(3, 0, 0, 4, 4)], (7, 3))
    with pytest.raises(VjError):
        extract_affine_yuv_layout(a, [[3.0] + IDENT], (7, 3))
    with pytest.raises(ValueError):
        extract_yuv_layout(a, rects, (7, 3), layout="yuy2")
    with pytest.raises(ValueError):
        extract_yuv_layout(a.astype(np.float32), rects, (7, 3))


# ------------------------------------------------------------------------------------------------------------------- the errors
def test_argument_errors_of_both_calls(lib):
    def both(images, word, yp=None):
        rc, _, ch, nbytes, msg = layout(lib, images, [(0, 0, 0, 4, 4)], yp=yp)
        assert rc == VJ_ERR_ARG and word in msg and (ch, nbytes) == (0, 0), msg
        rc, ch, nbytes, msg = affine_layout(lib, images, [[0] + IDENT], yp=yp)
        assert rc == VJ_ERR_ARG and word in msg and (ch, nbytes) == (0, 0), msg

    ok = OK_FRAMES()
    assert layout(lib, ok, [(0, 0, 0, 4, 4)])[0] == 0 and affine_layout(lib, ok, [[0] + IDENT])[0] == 0
    # null arguments and negative counts
    p, ap, yp = ExtractParams(), AffineParams(), yuv_params(lib)
    lib.vj_extract_default(C.byref(p))
    p.out_w = p.out_h = ap.out_w = ap.out_h = 4
    arr = (_YuvImage * 3)(*ok)
    r = np.array([(0, 0, 0, 4, 4), (1, 1, 1, 2, 2)], np.int32)
    a = np.zeros(2, AFFINE_DTYPE)
    a["m"] = IDENT
    src, ch, n = np.zeros((2, 5), np.int32), C.c_int(0), C.c_uint64(0)
    good = [arr, 3, r.ctypes.data, 2, C.byref(p), C.byref(yp), src.ctypes.data, C.byref(ch), C.byref(n)]
    assert lib.vj_extract_yuv_layout(*good) == 0
    for i in (0, 2, 4, 5, 6, 7, 8):
        assert lib.vj_extract_yuv_layout(*[None if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG and "null" in lib.vj_last_error().decode(), i
    for i in (1, 3):
        assert lib.vj_extract_yuv_layout(*[-1 if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG
    good = [arr, 3, a.ctypes.data, 2, C.byref(ap), C.byref(yp), C.byref(ch), C.byref(n)]
    assert lib.vj_extract_affine_yuv_layout(*good) == 0
    for i in (0, 2, 4, 5, 6, 7):
        assert lib.vj_extract_affine_yuv_layout(*[None if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG and "null" in lib.vj_last_error().decode(), i
    for i in (1, 3):
        assert lib.vj_extract_affine_yuv_layout(*[-1 if j == i else v for j, v in enumerate(good)]) == VJ_ERR_ARG
    # the frame errors of vj_yuv_to_bgr: the frame is named
    for bad, word in [(image(8, 4, y=False, at=3), "null y plane"), (image(8, 4, c0=False, at=3), "null c0 plane"),
                      (image(8, 4, yc.I420, c1=False, at=3), "null c1 plane"), (image(0, 4, at=3), "must be positive"), (image(8, -2, at=3), "must be positive"),
                      (image(7, 4, at=3), "must be even"), (image(8, 3, at=3), "must be even"), (image(8, 4, y_stride=7, at=3), "y_stride"),
                      (image(8, 4, c_stride=7, at=3), "c_stride"), (image(8, 4, yc.I420, c_stride=3, at=3), "c_stride"), (image(8, 4, 3, at=3), "unknown layout")]:
        both([ok[0], bad], "frame 1")
        both([ok[0], bad], word)
    # yp
    for bad, word in [(yuv_params(lib, 1), "channels"), (yuv_params(lib, 5), "channels"), (yuv_params(lib, 0), "channels"), (yuv_params(lib, 3, 2), "unknown bits"),
                      (yuv_params(lib, 3, 0x80000001), "unknown bits"), (yuv_params(lib, 4, 0, 1), "reserved")]:
        both(ok, word, yp=bad)
        both(ok, "vj_yuv_params", yp=bad)
    # the region and parameter errors of vj_extract
    for rects, word in [([(3, 0, 0, 4, 4)], "region 0: frame 3"), ([(0, 0, 0, 4, 4), (-1, 0, 0, 4, 4)], "region 1: frame -1"), ([(0, 0, 0, 0, 4)], "region 0: w and h"),
                        ([(0, 0, 0, 4, 4), (1, 0, 0, 4, -1)], "region 1: w and h")]:
        rc, _, ch_, nb, msg = layout(lib, ok, rects)
        assert rc == VJ_ERR_ARG and word in msg and (ch_, nb) == (0, 0), msg
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=-1), "out_h"), (dict(sx=-0.5), "sx"), (dict(sy=float("nan")), "sy"), (dict(margin=float("inf")), "margin"),
                     (dict(margin=-0.1), "margin"), (dict(flags=4), "unknown bits"), (dict(reserved=1), "reserved")]:
        rc, _, ch_, nb, msg = layout(lib, ok, [(0, 0, 0, 4, 4)], **kw)
        assert rc == VJ_ERR_ARG and word in msg and (ch_, nb) == (0, 0), (kw, msg)
    # the affine and parameter errors of vj_extract_affine
    for rows, word in [([[3] + IDENT], "affine 0: frame 3"), ([[0] + IDENT, [-1] + IDENT], "affine 1: frame -1"), ([[0] + IDENT + [1]], "affine 0: reserved"),
                       ([[0] + IDENT, [0, 1.0, float("nan"), 0, 0, 1, 0]], "affine 1: m[1]"), ([[0, 1.0, 0, 0, 0, 1, float("inf")]], "affine 0: m[5]")]:
        rc, ch_, nb, msg = affine_layout(lib, ok, rows)
        assert rc == VJ_ERR_ARG and word in msg and (ch_, nb) == (0, 0), msg
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=-1), "out_h"), (dict(flags=4), "unknown bits"), (dict(reserved=1), "reserved")]:
        rc, ch_, nb, msg = affine_layout(lib, ok, [[0] + IDENT], **kw)
        assert rc == VJ_ERR_ARG and word in msg and (ch_, nb) == (0, 0), (kw, msg)


def test_every_limit_at_its_bound_and_one_step_past_it(lib):
    ok = OK_FRAMES()
    # the frames' 65534 side limit (vj_yuv_to_bgr's)
    assert layout(lib, [image(65534, 2, at=0)], [(0, 0, 0, 4, 4)])[0] == 0 and affine_layout(lib, [image(2, 65534, at=0)], [[0] + IDENT])[0] == 0
    for bad in (image(65536, 2, at=0), image(2, 65536, at=0)):
        rc, *_, msg = layout(lib, [ok[0], bad], [(0, 0, 0, 4, 4)])
        assert rc == VJ_ERR_LIMIT and "frame 1" in msg and "65534" in msg, msg
        rc, *_, msg = affine_layout(lib, [ok[0], bad], [[0] + IDENT])
        assert rc == VJ_ERR_LIMIT and "frame 1" in msg and "65534" in msg, msg
    # vj_extract's: output and mapped sides up to 65535, coordinates within +-2^24
    assert layout(lib, ok, [(0, 0, 0, 65535, 65535)], (65535, 1))[2:4] == (3, 65535 * 3)
    assert layout(lib, ok, [(0, -(1 << 24), 1 << 23, 1, 1)])[0] == 0
    for rect, size, kw, word in [((0, 0, 0, 4, 4), (65536, 4), {}, "65535"), ((0, 0, 0, 4, 4), (4, 65536), {}, "65535"), ((0, 0, 0, 65536, 4), (4, 4), {}, "65535"),
                                 ((0, 0, 0, 4, 65536), (4, 4), {}, "65535"), ((0, 0, 0, 40000, 4), (4, 4), dict(sx=2.0), "65535"),
                                 ((0, 0, 0, 40000, 4), (4, 4), dict(margin=0.5), "65535"), ((0, (1 << 24) + 1, 0, 4, 4), (4, 4), {}, "2^24"),
                                 ((0, 0, -(1 << 24) - 1, 4, 4), (4, 4), {}, "2^24"), ((0, 1 << 24, 0, 4, 4), (4, 4), {}, "2^24")]:
        rc, _, ch, nb, msg = layout(lib, ok, [(0, 0, 0, 4, 4), rect], size, **kw)
        assert rc == VJ_ERR_LIMIT and word in msg and ("region 1" in msg or "vj_extract_params" in msg) and (ch, nb) == (0, 0), msg
    # the work units of the DECODED channels: 65535 x 65535 x 3 interleaved is 768 x 4096 blocks per region — 682 regions fit,
    # 683 do not; the planner's own check on the one-channel Y planes (257 x 4096 blocks) would let 2040 through
    many = [(0, 0, 0, 2, 2)] * 683
    rc, _, ch, nb, msg = layout(lib, ok, many, (65535, 65535))
    assert rc == VJ_ERR_LIMIT and "work units" in msg and (ch, nb) == (0, 0), msg
    assert layout(lib, ok, many[:682], (65535, 65535))[2] == 3
    assert layout(lib, ok, many * 2 + many[:674], (65535, 65535), flags=VJ_EXTRACT_GRAY)[2] == 1          # 2040
    assert layout(lib, ok, many * 2 + many[:675], (65535, 65535), flags=VJ_EXTRACT_GRAY)[0] == VJ_ERR_LIMIT
    rows = [[0] + IDENT] * 683
    assert affine_layout(lib, ok, rows, (65535, 65535))[0] == VJ_ERR_LIMIT and "work units" in lib.vj_last_error().decode()
    assert affine_layout(lib, ok, rows[:682], (65535, 65535))[1] == 3
    # vj_extract_affine's: output sides up to 65535, the terms within 2^19
    assert affine_layout(lib, ok, [[0] + IDENT], (65535, 1))[0] == 0
    assert affine_layout(lib, ok, [[0] + IDENT], (65536, 1))[0] == VJ_ERR_LIMIT and "65535" in lib.vj_last_error().decode()
    assert affine_layout(lib, ok, [[0] + IDENT], (1, 65536))[0] == VJ_ERR_LIMIT
    lim = 524288.0
    assert affine_layout(lib, ok, [[0, lim / 16, 0, lim, 0, 1, -lim]], (17, 4))[0] == 0
    for row, word in [([0, lim / 16 + 1, 0, 0, 0, 1, 0], "|m[0]| (out_w - 1)"), ([0, 1, 0, 0, -lim / 16 - 1, 1, 0], "|m[3]| (out_w - 1)"),
                      ([0, 1, 0, lim + 1, 0, 1, 0], "|m[2]|"), ([0, 1, lim / 3 + 1, 0, 0, 1, 0], "|m[1] (out_h - 1) + m[2]|"),
                      ([0, 1, 0, 0, 0, 1, -lim - 1], "|m[5]|"), ([0, 1, 0, 0, 0, lim / 3 + 1, 0], "|m[4] (out_h - 1) + m[5]|")]:
        rc, ch, nb, msg = affine_layout(lib, ok, [[0] + IDENT, row], (17, 4))
        assert rc == VJ_ERR_LIMIT and "affine 1" in msg and word in msg and (ch, nb) == (0, 0), msg


# ------------------------------------------------------------------------------------------------------------------- the premises
@pytest.mark.parametrize("layout_id", eyc.LAYOUTS)
def test_the_tap_by_tap_model_is_the_definitions_sentence(oracle, layout_id):
    """decode first, clamps on the luma coordinate, chroma from the clamped one: written out per tap it gives the composition's
    bytes — on the copy, the mean and the bilinear path, at every parity of the origin, across the frame's edges, with alpha, in RGB."""
    fr = eyc.frames(layout_id)
    for (rects, size), (alpha, rgb) in zip(eyc.resize_cases(), [(False, False), (True, False), (False, True), (True, True), (False, False), (True, True), (False, True)]):
        want = eyc.restate(oracle, fr, layout_id, rects, size, alpha=alpha, rgb=rgb)
        for k, r in enumerate(rects):
            assert np.array_equal(eyc.model(fr[0], layout_id, r[1:], size, alpha=alpha, rgb=rgb), want[k]), (r, size)
    want = eyc.restate(oracle, fr, layout_id, [(1, 3, 5, 50, 21)], (33, 17), margin=0.1)
    assert np.array_equal(eyc.model(fr[1], layout_id, ec.map_region((1, 3, 5, 50, 21), margin=0.1)[1:], (33, 17)), want[0])


@pytest.mark.parametrize("layout_id", eyc.LAYOUTS)
def test_each_wrong_variant_differs_on_the_case_meant_to_catch_it(oracle, layout_id):
    edge = eyc.edge_planes(layout_id)
    _, x, y, w, h = ec.EDGE_RECT
    right = eyc.model(edge, layout_id, (x, y, w, h), ec.EDGE_SIZE)
    assert np.array_equal(right, eyc.restate(oracle, [edge], layout_id, [ec.EDGE_RECT], ec.EDGE_SIZE)[0])
    differs = lambda variant, planes, region, size, ref: int((eyc.model(planes, layout_id, region, size, variant) != ref).sum())
    # the crop whose edges differ from its surroundings, in Y and in chroma: the crop-edge clamp, on both coordinates
    assert int(right.max()) < 200                                                 # nothing from outside the crop leaks in
    wrong = eyc.model(edge, layout_id, (x, y, w, h), ec.EDGE_SIZE, "frame_clamp")
    assert differs("frame_clamp", edge, (x, y, w, h), ec.EDGE_SIZE, right) > 0 and np.array_equal(wrong[2:-2, 2:-2], right[2:-2, 2:-2])
    assert y % 2 == 0 and x % 2 == 0                                              # the row above and the column left of the crop: other chroma samples
    wrong = eyc.model(edge, layout_id, (x, y, w, h), ec.EDGE_SIZE, "chroma_before")
    assert not np.array_equal(wrong[0], right[0]) and np.array_equal(wrong[2:-2, 2:-2], right[2:-2, 2:-2])
    # a crop at an odd origin: the chroma index of the sum is not the sum of the indices
    fr = eyc.frames(layout_id)
    for region, size in [((9, 7, 10, 10), (10, 10)), ((9, 7, 10, 10), (5, 5)), ((9, 6, 20, 17), (64, 34)), ((8, 7, 20, 17), (64, 34))]:
        ref = eyc.model(fr[0], layout_id, region, size)
        assert differs("chroma_split", fr[0], region, size, ref) > 0, (region, size)
    for region, size in [((8, 6, 10, 10), (10, 10)), ((8, 6, 20, 17), (64, 34))]:   # (at an even one it is)
        assert differs("chroma_split", fr[0], region, size, eyc.model(fr[0], layout_id, region, size)) == 0
    # crops over each frame edge: the frame clamp acts on the luma coordinate, the chroma follows — and everywhere: decode first, U is U
    for r in [(-5, 8, 10, 10), (33, 9, 10, 10), (8, -5, 10, 10), (9, 25, 10, 10), (8, 6, 10, 10)]:
        for size in [(10, 10), (5, 5), (21, 17)]:
            ref = eyc.restate(oracle, fr, layout_id, [(0,) + r], size)[0]
            assert np.array_equal(eyc.model(fr[0], layout_id, r, size), ref)
            assert differs("swap_uv", fr[0], r, size, ref) > 0
            if size != (10, 10):                                                  # (a copy blends nothing)
                assert differs("blend_first", fr[0], r, size, ref) > 0
    # U and V exchanged for NV21: NV21 read as NV12 is the swap
    if layout_id == yc.NV21:
        as_nv12 = eyc.model(fr[0], yc.NV12, (8, 6, 10, 10), (5, 5))
        assert np.array_equal(as_nv12, eyc.model(fr[0], yc.NV21, (8, 6, 10, 10), (5, 5), "swap_uv"))
        assert not np.array_equal(as_nv12, eyc.model(fr[0], yc.NV21, (8, 6, 10, 10), (5, 5)))


def test_alpha_is_255_in_every_resize_mode_and_in_the_affine_blend(oracle):
    fr = eyc.frames(yc.NV12)
    for rects, size in eyc.resize_cases():
        for planar in (False, True):
            out = eyc.restate(oracle, fr, yc.NV12, rects, size, alpha=True, planar=planar)
            a = out[:, 3] if planar else out[..., 3]
            assert out.shape[1 if planar else 3] == 4 and int(a.min()) == 255, (size, planar)
    for name, ms, size in eyc.affine_matrices():
        out = eyc.restate_affine(oracle, fr, yc.NV12, ac.rows_for(0, ms), size, alpha=True)
        assert out.shape[3] == 4 and int(out[..., 3].min()) == 255, name


@pytest.mark.parametrize("layout_id", eyc.LAYOUTS)
def test_the_random_frames_reach_sat_at_both_ends_of_every_channel_inside_the_crops(layout_id):
    """Inside the 20 x 17 and the 5 x 5 crops the GPU tests cut, the unsaturated B, G and R fall below 0 and above 255."""
    fr = eyc.frames(layout_id)
    for planes, (x, y, w, h) in [(fr[0], (8, 6, 20, 17)), (fr[0], (9, 7, 20, 17)), (fr[1], (8, 6, 20, 17))]:
        Y, U, V = (p.astype(np.int64) for p in yc.split_chroma(planes, layout_id))
        U, V = (np.repeat(np.repeat(c, 2, axis=0), 2, axis=1) for c in (U, V))
        s = (slice(y, y + h), slice(x, x + w))
        yy = np.maximum(Y[s] - 16, 0) * 1220542 + yc.H
        for t in (yy + 2116026 * (U[s] - 128), yy - 852492 * (V[s] - 128) - 409993 * (U[s] - 128), yy + 1673527 * (V[s] - 128)):
            assert int((t >> 20).min()) < 0 and int((t >> 20).max()) > 255


def test_the_output_sizes_straddle_the_work_units_sides():
    """EXTRACT_BLOCK_SLOTS four-byte slots and EXTRACT_BLOCK_H rows, read from the header: rows of one, three and four bytes per pixel
    with fewer, exactly as many and more bytes than a block's, at every alignment; heights below, at and above a block's."""
    text = open(os.path.join(ROOT, "clfacedetection_amd", "csrc", "vj_extract_units.hpp")).read()
    slots, rows = (int(v) for v in re.search(r"EXTRACT_BLOCK_SLOTS = (\d+), EXTRACT_BLOCK_H = (\d+);", text).groups())
    assert (slots, rows) == (64, 16)
    block = 4 * slots
    for c in (1, 3, 4):                                   # a row of exactly k blocks' bytes, one pixel fewer and one pixel more
        b = {w * c for w in eyc.OUT_WIDTHS}
        exact = [v for v in b if v % block == 0]
        assert exact and all(v - c in b and v + c in b for v in exact) and min(b) <= 4, c
    assert {w * c % 4 for w in eyc.OUT_WIDTHS for c in (1, 3)} == {0, 1, 2, 3}      # rows that begin at every address mod 4
    assert {rows - 1, rows, rows + 1} <= set(eyc.OUT_HEIGHTS) and min(eyc.OUT_HEIGHTS) == 1
