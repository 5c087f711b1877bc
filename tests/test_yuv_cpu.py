"""vj_yuv_to_bgr_layout, vj_bgr_to_yuv_layout and vj_yuv_luma through ctypes (host only, no device): pitches, offsets, alignment, no
overlap, the exact byte count, mixed sizes; every argument error with its message and each limit at the bound and one step past it.
And the premises of tests/test_gpu_yuv.py with the numpy restatement (tests/yuv_cases.py) alone: the known answers of the
definition, every deliberately wrong variant differing from the right one on the case meant to catch it, gray round trips, the
encoder's range, and the decode frames reaching both ends of the saturation."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_cases as yc
from clfacedetection_amd import (VJ_YUV_I420, VJ_YUV_NV12, VJ_YUV_NV21, VJ_YUV_RGB_ORDER, VjError, YuvParams, bgr_to_yuv_layout,
                                 yuv_to_bgr_layout)
from clfacedetection_amd.api import _Image, _YuvImage

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(64, np.uint8)
LAYOUTS = (VJ_YUV_NV12, VJ_YUV_NV21, VJ_YUV_I420)


def yuv(w, h, layout=VJ_YUV_NV12, y_stride=None, c_stride=None, y=True, c0=True, c1=True, on_device=0):
    p = PX.ctypes.data
    crow = w // 2 if layout == VJ_YUV_I420 else w
    return _YuvImage(p if y else None, p if c0 else None, p if c1 else None, w, h, w if y_stride is None else y_stride,
                     crow if c_stride is None else c_stride, layout, on_device)


def bgr(w, h, ch=3, stride=None, data=True, on_device=0):
    return _Image(PX.ctypes.data if data else None, w, h, w * max(ch, 1) if stride is None else stride, on_device, ch)


def params(lib, **kw):
    p = YuvParams(9, 9, 9)
    lib.vj_yuv_default(C.byref(p))
    assert (p.channels, p.flags, p.reserved) == (3, 0, 0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def decode_layout(lib, images, **kw):
    """-> (rc, [(offset, w, h, stride, on_device, channels)], bytes, last error)"""
    p = params(lib, **kw)
    n = len(images)
    arr = (_YuvImage * max(n, 1))(*images)
    out = (_Image * max(n, 1))()
    nbytes = C.c_uint64(12345)
    rc = lib.vj_yuv_to_bgr_layout(arr, n, C.byref(p), out, C.byref(nbytes))
    return rc, [(int(o.data or 0), o.width, o.height, o.stride, o.on_device, o.channels) for o in out[:n]], int(nbytes.value), lib.vj_last_error().decode()


def encode_layout(lib, images, layout=VJ_YUV_NV12, **kw):
    """-> (rc, [(y, c0, c1, w, h, y_stride, c_stride, layout, on_device)], bytes, last error)"""
    p = params(lib, **kw)
    n = len(images)
    arr = (_Image * max(n, 1))(*images)
    out = (_YuvImage * max(n, 1))()
    nbytes = C.c_uint64(12345)
    rc = lib.vj_bgr_to_yuv_layout(arr, n, C.byref(p), layout, out, C.byref(nbytes))
    return rc, [(int(o.y or 0), int(o.c0 or 0), int(o.c1 or 0), o.width, o.height, o.y_stride, o.c_stride, o.layout, o.on_device)
                for o in out[:n]], int(nbytes.value), lib.vj_last_error().decode()


SIZES = yc.MIXED_SIZES + [(w, 2 + w % 6 // 2 * 2) for w in range(2, 12, 2)]


# ---------------------------------------------------------------------------------------------------------------- the layouts
def test_the_header_constants():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "clfacedetection_amd", "csrc", "vj_yuv_units.hpp")).read()
    lane = int(re.search(r"YUV_LANE_W = (\d+)", src).group(1))
    block_h = int(re.search(r"YUV_BLOCK_H = (\d+)", src).group(1))
    assert re.search(r"YUV_BLOCK_W = 64u \* YUV_LANE_W", src)
    assert (lane, 64 * lane, block_h) == (yc.LANE_W, yc.BLOCK_W, yc.BLOCK_H)
    # the shapes the GPU tests use straddle a lane, a wave's row and a block's height
    for edge in (lane, 64 * lane):
        assert {edge - 2, edge, edge + 2} <= set(yc.WIDTHS)
    assert {2 * 64 * lane - 2, 2 * 64 * lane + 2} <= set(yc.WIDTHS)
    for edge in (block_h, 2 * block_h):
        assert {edge - 2, edge, edge + 2} <= set(yc.HEIGHTS)
    assert {2, 4, 6} <= set(yc.HEIGHTS)


@pytest.mark.parametrize("channels", [3, 4])
def test_decode_layout(lib, channels):
    ims = [yuv(w, h, LAYOUTS[i % 3]) for i, (w, h) in enumerate(SIZES)]
    rc, recs, nbytes, _ = decode_layout(lib, ims, channels=channels)
    assert rc == 0
    end = 0
    for (off, w, h, stride, dev, ch), (sw, sh) in zip(recs, SIZES):
        assert (w, h, ch, dev) == (sw, sh, channels, 1) and stride == (sw * channels + 3) // 4 * 4
        assert off % 256 == 0 and off >= end and off - end < 256
        end = off + stride * h
    assert nbytes == end
    # the layout does not depend on the source's layout, strides or residence
    rc, again, nbytes2, _ = decode_layout(lib, [yuv(w, h, VJ_YUV_I420, y_stride=w + 5, c_stride=w, on_device=1) for w, h in SIZES], channels=channels,
                                          flags=VJ_YUV_RGB_ORDER)
    assert rc == 0 and again == recs and nbytes2 == nbytes
    assert decode_layout(lib, [], channels=channels)[::2] == (0, 0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_layout(lib, layout):
    ims = [bgr(w, h, 3 + i % 2) for i, (w, h) in enumerate(SIZES)]
    rc, recs, nbytes, _ = encode_layout(lib, ims, layout)
    assert rc == 0
    end = 0
    for (y, c0, c1, w, h, ys, cs, lay, dev), (sw, sh) in zip(recs, SIZES):
        assert (w, h, lay, dev) == (sw, sh, layout, 1)
        assert y % 256 == 0 and y >= end and y - end < 256 and ys == (sw + 3) // 4 * 4
        assert c0 == y + ys * h and c0 % 4 == 0                                  # chroma right below the Y plane
        if layout == VJ_YUV_I420:
            assert cs == (sw // 2 + 3) // 4 * 4 and c1 == c0 + cs * (h // 2) and c1 % 4 == 0
            end = c1 + cs * (h // 2)
        else:
            assert cs == ys and c1 == 0
            end = c0 + cs * (h // 2)
    assert nbytes == end
    # a width that is a multiple of 4 (8 for I420) gives the stacked form OpenCV and the decoders hand out: h * 3 / 2 rows of w bytes
    rc, recs, nbytes, _ = encode_layout(lib, [bgr(16, 6)], layout)
    assert rc == 0 and nbytes == 16 * 9 and recs[0][1] == 16 * 6 and (layout != VJ_YUV_I420 or recs[0][2] == 16 * 6 + 8 * 3)
    assert encode_layout(lib, [], layout)[::2] == (0, 0)


def test_luma(lib):
    out = _Image()
    f = yuv(10, 6, VJ_YUV_I420, y_stride=17, on_device=1)
    assert lib.vj_yuv_luma(C.byref(f), C.byref(out)) == 0
    assert (out.data, out.width, out.height, out.stride, out.on_device, out.channels) == (PX.ctypes.data, 10, 6, 17, 1, 1)
    odd = yuv(9, 5, y_stride=9)                                                  # the Y plane of any size is a gray image
    assert lib.vj_yuv_luma(C.byref(odd), C.byref(out)) == 0 and (out.width, out.height, out.on_device) == (9, 5, 0)
    assert lib.vj_yuv_luma(None, C.byref(out)) == VJ_ERR_ARG and lib.vj_yuv_luma(C.byref(f), None) == VJ_ERR_ARG
    for bad, word in [(yuv(10, 6, y=False), "y plane"), (yuv(0, 6), "positive"), (yuv(10, -2), "positive"), (yuv(10, 6, y_stride=9), "y_stride")]:
        assert lib.vj_yuv_luma(C.byref(bad), C.byref(out)) == VJ_ERR_ARG and word in lib.vj_last_error().decode()


def test_the_python_twins(lib):
    frames = [np.zeros((h * 3 // 2, w), np.uint8) for w, h in yc.MIXED_SIZES[:4]]
    recs, nbytes = yuv_to_bgr_layout(frames, alpha=True)
    assert [(r[1], r[2], r[3]) for r in recs] == [(w, h, 4 * w) for w, h in yc.MIXED_SIZES[:4]] and nbytes == recs[-1][0] + recs[-1][3] * recs[-1][2]
    recs, nbytes = yuv_to_bgr_layout(np.zeros((3, 9, 6), np.uint8), layout="i420")
    assert recs == [(0, 6, 6, 20), (256, 6, 6, 20), (512, 6, 6, 20)] and nbytes == 632
    recs, nbytes = bgr_to_yuv_layout(np.zeros((2, 4, 6, 3), np.uint8), layout="i420")
    assert recs == [(0, 32, 40, 6, 4, 8, 4), (256, 288, 296, 6, 4, 8, 4)] and nbytes == 304
    recs, nbytes = bgr_to_yuv_layout([np.zeros((2, 2, 4), np.uint8), np.zeros((4, 8, 3), np.uint8)], layout="nv21")
    assert recs == [(0, 8, 0, 2, 2, 4, 4), (256, 288, 0, 8, 4, 8, 8)] and nbytes == 304
    with pytest.raises(ValueError):
        yuv_to_bgr_layout(frames, layout="yv12")
    with pytest.raises(VjError):
        yuv_to_bgr_layout(np.zeros((3, 3), np.uint8))                             # 3 x 2: an odd width
    with pytest.raises(VjError):
        bgr_to_yuv_layout([np.zeros((4, 4), np.uint8)])                           # gray


# ---------------------------------------------------------------------------------------------------------------- the errors
def test_decode_argument_errors(lib):
    ok = [yuv(8, 4), yuv(6, 2, VJ_YUV_I420)]
    p = params(lib)
    out = (_Image * 3)()
    n = C.c_uint64(0)
    arr = (_YuvImage * 2)(*ok)
    f = lib.vj_yuv_to_bgr_layout
    assert f(arr, 2, C.byref(p), out, C.byref(n)) == 0
    for args in [(None, 2, C.byref(p), out, C.byref(n)), (arr, 2, None, out, C.byref(n)), (arr, 2, C.byref(p), None, C.byref(n)),
                 (arr, 2, C.byref(p), out, None), (arr, -1, C.byref(p), out, C.byref(n))]:
        assert f(*args) == VJ_ERR_ARG
    bad = [(yuv(8, 4, y=False), "null y plane"), (yuv(8, 4, c0=False), "null c0 plane"), (yuv(8, 4, VJ_YUV_I420, c1=False), "null c1 plane"),
           (yuv(0, 4), "positive"), (yuv(8, -2), "positive"), (yuv(7, 4), "even"), (yuv(8, 3), "even"),
           (yuv(8, 4, y_stride=7), "y_stride"), (yuv(8, 4, c_stride=7), "c_stride"), (yuv(8, 4, VJ_YUV_I420, c_stride=3), "c_stride"),
           (yuv(8, 4, 3), "layout"), (yuv(8, 4, -1), "layout")]
    for im, word in bad:
        rc, _, nbytes, err = decode_layout(lib, ok + [im])
        assert rc == VJ_ERR_ARG and "frame 2" in err and word in err and nbytes == 0, (word, err)
    assert decode_layout(lib, [yuv(8, 4, c1=False), yuv(8, 4, VJ_YUV_NV21, c1=False)])[0] == 0    # NV12 / NV21 ignore c1
    assert decode_layout(lib, [yuv(8, 4, VJ_YUV_I420, c_stride=4)])[0] == 0                       # the chroma rows of I420 are w / 2 bytes
    for kw, word in [(dict(flags=2), "flags"), (dict(flags=VJ_YUV_RGB_ORDER | 1 << 31), "flags"), (dict(reserved=1), "reserved"),
                     (dict(channels=1), "channels"), (dict(channels=0), "channels"), (dict(channels=5), "channels"), (dict(channels=2), "channels")]:
        rc, _, nbytes, err = decode_layout(lib, ok, **kw)
        assert rc == VJ_ERR_ARG and word in err and nbytes == 0, kw
        assert decode_layout(lib, [], **kw)[0] == VJ_ERR_ARG                      # ... also without any frame


def test_encode_argument_errors(lib):
    ok = [bgr(8, 4), bgr(6, 2, 4)]
    p = params(lib)
    out = (_YuvImage * 3)()
    n = C.c_uint64(0)
    arr = (_Image * 2)(*ok)
    f = lib.vj_bgr_to_yuv_layout
    assert f(arr, 2, C.byref(p), VJ_YUV_I420, out, C.byref(n)) == 0
    for args in [(None, 2, C.byref(p), 0, out, C.byref(n)), (arr, 2, None, 0, out, C.byref(n)), (arr, 2, C.byref(p), 0, None, C.byref(n)),
                 (arr, 2, C.byref(p), 0, out, None), (arr, -1, C.byref(p), 0, out, C.byref(n))]:
        assert f(*args) == VJ_ERR_ARG
    bad = [(bgr(8, 4, data=False), "null data"), (bgr(8, 4, 1), "gray"), (bgr(8, 4, 0), "gray"), (bgr(8, 4, 2, stride=16), "channels"),
           (bgr(0, 4), "positive"), (bgr(8, -2), "positive"), (bgr(7, 4), "even"), (bgr(8, 3), "even"), (bgr(8, 4, stride=23), "stride"),
           (bgr(8, 4, 4, stride=31), "stride")]
    for im, word in bad:
        rc, _, nbytes, err = encode_layout(lib, ok + [im])
        assert rc == VJ_ERR_ARG and "frame 2" in err and word in err and nbytes == 0, (word, err)
    for lay in (3, -1, 99):
        rc, _, nbytes, err = encode_layout(lib, ok, lay)
        assert rc == VJ_ERR_ARG and "layout" in err and nbytes == 0
    for kw, word in [(dict(flags=2), "flags"), (dict(reserved=1), "reserved")]:
        rc, _, nbytes, err = encode_layout(lib, ok, **kw)
        assert rc == VJ_ERR_ARG and word in err and nbytes == 0
    assert encode_layout(lib, ok, channels=0)[0] == 0                             # every source says its own channel count


def test_limits(lib):
    # a side: 65534 passes, 65535 (odd) and 65536 are beyond the limit
    assert decode_layout(lib, [yuv(65534, 2), yuv(2, 65534, VJ_YUV_I420)], channels=4)[0] == 0
    assert encode_layout(lib, [bgr(65534, 2), bgr(2, 65534, 4)], VJ_YUV_I420)[0] == 0
    for w, h in [(65536, 2), (2, 65536), (65535, 2), (2, 65535)]:
        rc, _, nbytes, err = decode_layout(lib, [yuv(8, 4), yuv(w, h, y_stride=w, c_stride=w)])
        assert rc == VJ_ERR_LIMIT and "65534" in err and "frame 1" in err and nbytes == 0
        rc, _, nbytes, err = encode_layout(lib, [bgr(8, 4), bgr(w, h)])
        assert rc == VJ_ERR_LIMIT and "65534" in err and "frame 1" in err and nbytes == 0
    # work units beyond a 32-bit index: 256 x 2048 blocks of 256 x 32 pixels per 65534 x 65534 frame; 4095 frames pass, 4096 do not
    big = [yuv(65534, 65534)] * 4096
    rc, _, _, err = decode_layout(lib, big)
    assert rc == VJ_ERR_LIMIT and "work units" in err
    assert decode_layout(lib, big[:4095])[0] == 0
    big = [bgr(65534, 65534)] * 4096
    rc, _, _, err = encode_layout(lib, big)
    assert rc == VJ_ERR_LIMIT and "work units" in err
    assert encode_layout(lib, big[:4095])[0] == 0


# ---------------------------------------------------------------------------------- the premises of the GPU tests: the restatement
def test_known_answers():
    for (Y, U, V), bgr_ in yc.DECODE_KNOWN:
        assert tuple(int(c) for c in yc.decode_px(Y, U, V)) == bgr_, (Y, U, V)
    for (B, G, R), yuv_ in yc.ENCODE_KNOWN:
        assert tuple(int(c) for c in yc.encode_px(B, G, R)) == yuv_, (B, G, R)
    # through whole frames, every layout, both channel counts and orders
    for layout in (yc.NV12, yc.NV21, yc.I420):
        for (Y, U, V), (B, G, R) in yc.DECODE_KNOWN:
            planes = yc.join_chroma(np.full((2, 2), Y, np.uint8), np.full((1, 1), U, np.uint8), np.full((1, 1), V, np.uint8), layout)
            assert (yc.decode(planes, layout) == (B, G, R)).all() and (yc.decode(planes, layout, 4, True) == (R, G, B, 255)).all()
        for (B, G, R), (Y, U, V) in yc.ENCODE_KNOWN:
            y, u, v = yc.split_chroma(yc.encode(np.full((2, 2, 3), (B, G, R), np.uint8), layout), layout)
            assert (y == Y).all() and (u, v) == (U, V)
            y, u, v = yc.split_chroma(yc.encode(np.full((2, 2, 4), (R, G, B, 7), np.uint8), layout, rgb=True), layout)
            assert (y == Y).all() and (u, v) == (U, V)


def test_the_floor_matters_in_a_known_answer():
    """(81, 90, 240): G and B are negative before the shift — but both saturate to 0 under the floor and under truncation alike,
    so this known answer does not tell them apart.  No pixel can: sat() absorbs every negative quotient, and for t >= 0 the two
    agree.  The restatement says so for ALL 2^24 inputs; the variant stays in the list as one that no case can catch."""
    Y, U, V = 81, 90, 240
    yy = max(Y - 16, 0) * 1220542
    assert yy + yc.H + 2116026 * (U - 128) < 0 and yy + yc.H - 852492 * (V - 128) - 409993 * (U - 128) < 0
    assert tuple(int(c) for c in yc.decode_px(Y, U, V, floor=False)) == tuple(int(c) for c in yc.decode_px(Y, U, V))
    Ug, Vg = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for Yg in range(256):
        a, b = yc.decode_px(np.full_like(Ug, Yg), Ug, Vg), yc.decode_px(np.full_like(Ug, Yg), Ug, Vg, floor=False)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the encoder's sums are positive for every colour (the smallest: U of pure yellow), where the two shifts agree as well
    assert -155188 * 255 - 305135 * 255 + yc.H + (128 << 20) > 0 and -385875 * 255 - 74448 * 255 + yc.H + (128 << 20) > 0


def test_each_wrong_variant_differs_where_it_is_meant_to():
    frames = yc.exhaustive_frames(yc.NV12)
    right = [yc.decode(f, yc.NV12) for f in frames]
    for variant in ("swap_uv", "no_clamp"):
        assert any(not np.array_equal(yc.decode(f, yc.NV12, variant=variant), r) for f, r in zip(frames, right)), variant
    # no max(Y - 16, 0): Y below 16 with neutral chroma goes negative and saturates to 0 either way, but with chroma it shows
    assert tuple(int(c) for c in yc.decode_px(0, 255, 128, clamp_y=False)) != tuple(int(c) for c in yc.decode_px(0, 255, 128))
    # the layouts differ from each other on the same bytes
    f = yc.random_frame(8, 4, yc.NV12, 1)
    assert not np.array_equal(yc.decode(f, yc.NV12), yc.decode(f, yc.NV21))
    wild = yc.wild_image(66, 6, 5)
    good = yc.encode(wild, yc.I420)
    for variant in ("average", "bottom_right", "swap_uv"):
        bad = yc.encode(wild, yc.I420, variant=variant)
        assert np.array_equal(bad[0], good[0]) and not (np.array_equal(bad[1], good[1]) and np.array_equal(bad[2], good[2])), variant
    assert any(np.array_equal(im[..., :3], wild) for im in yc.encode_images(3))   # the GPU test sweeps this frame
    # R and B exchanged is seen by both directions
    assert not np.array_equal(yc.decode(f, yc.NV12, rgb=True), yc.decode(f, yc.NV12))
    assert not np.array_equal(yc.encode(wild, yc.NV12, rgb=True)[0], yc.encode(wild, yc.NV12)[0])


def test_gray_round_trips_within_one():
    x = np.arange(256)
    Y, U, V = yc.encode_px(x, x, x)
    assert (U == 128).all() and (V == 128).all()
    back = yc.decode_px(Y, U, V)
    assert all(np.abs(c - x).max() <= 1 for c in back)


def test_the_encoder_needs_no_clamp():
    corners = np.array([[(i & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255] for i in range(8)])
    rnd = np.random.default_rng(4096).integers(0, 256, (4096, 3))
    for colours in (corners, rnd):
        for c in yc.encode_px(colours[:, 0], colours[:, 1], colours[:, 2]):
            assert c.min() >= 16 and c.max() <= 240
    Y, U, V = yc.encode_px(corners[:, 0], corners[:, 1], corners[:, 2])
    assert (Y.min(), Y.max(), U.min(), U.max(), V.min(), V.max()) == (16, 235, 16, 240, 16, 240)


def test_the_random_decode_frames_saturate_at_both_ends():
    for layout in (yc.NV12, yc.NV21, yc.I420):
        f = yc.random_frame(66, 6, layout, 3)
        y, u, v = yc.split_chroma(f, layout)
        U, V = (np.repeat(np.repeat(c, 2, 0), 2, 1).astype(np.int64) for c in (u, v))
        yy = np.maximum(y.astype(np.int64) - 16, 0) * 1220542
        for t in (yy + yc.H + 2116026 * (U - 128), yy + yc.H - 852492 * (V - 128) - 409993 * (U - 128), yy + yc.H + 1673527 * (V - 128)):
            assert ((t >> 20) < 0).any() and ((t >> 20) > 255).any()


def test_the_stacked_form_round_trips():
    for layout in (yc.NV12, yc.I420):
        for w, h in [(6, 6), (8, 4), (2, 2)]:
            f = yc.random_frame(w, h, layout, 9)
            s = yc.stacked(f, layout)
            assert s.shape == (h * 3 // 2, w) and all(np.array_equal(a, b) for a, b in zip(yc.unstack(s, layout), f))
