"""vj_extract_layout through ctypes (host only, no device): the mapping of regions to source pixels (the ties of cvRound, the margin,
regions left outside their frame), the channel count and the byte count for every flag combination, every argument error and the
limits.  And the premises of tests/test_gpu_extract.py, with the restatements alone: the detector finds candidates in the frames the
many-regions test cuts from, and the crop-edge case tells clamping at the crop from clamping at the frame."""
import ctypes as C
import math

import numpy as np
import pytest

import extract_cases as ec
import prep_cases as pc
import scale_image_oracle as so
from clfacedetection_amd import ExtractParams, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VjError, extract_layout
from clfacedetection_amd.api import _Image

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(64, np.uint8)


def image(w, h, ch=1, stride=None, data=True, on_device=0):
    return _Image(PX.ctypes.data if data else None, w, h, w * max(ch, 1) if stride is None else stride, on_device, ch)


def layout(lib, images, rects, **kw):
    """-> (rc, mapped regions as tuples, channels, bytes, last error)"""
    p = ExtractParams()
    lib.vj_extract_default(C.byref(p))
    p.out_w, p.out_h = 24, 24
    for k, v in kw.items():
        setattr(p, k, v)
    n = len(images)
    arr = (_Image * max(n, 1))(*images)
    r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5))
    src = np.full((max(len(r), 1), 5), -7, np.int32)
    ch, nbytes = C.c_int(77), C.c_uint64(12345)
    rc = lib.vj_extract_layout(arr, n, r.ctypes.data, len(r), C.byref(p), src.ctypes.data, C.byref(ch), C.byref(nbytes))
    return rc, [tuple(int(v) for v in row) for row in src[:len(r)]], int(ch.value), int(nbytes.value), lib.vj_last_error().decode()


def test_default(lib):
    p = ExtractParams(1, 2, 3.0, 4.0, 5.0, 6, 7)
    lib.vj_extract_default(C.byref(p))
    assert (p.out_w, p.out_h, p.sx, p.sy, p.margin, p.flags, p.reserved) == (0, 0, 1.0, 1.0, 0.0, 0, 0)
    lib.vj_extract_default(None)


def test_mapping_with_the_ties_of_cv_round(lib):
    ims = [image(40, 30), image(9, 9)]
    rects = [(0, 5, 7, 5, 7), (0, 7, 5, 7, 5), (1, 1, 3, 1, 3), (0, 0, 0, 40, 30), (1, 9, 11, 13, 15)]
    rc, src, ch, nbytes, _ = layout(lib, ims, rects, sx=0.5, sy=0.5)
    assert rc == 0 and ch == 1 and nbytes == len(rects) * 24 * 24
    # 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 (a side: at least 1), 1.5 -> 2, 4.5 -> 4, 5.5 -> 6, 6.5 -> 6, 7.5 -> 8
    assert src == [(0, 2, 4, 2, 4), (0, 4, 2, 4, 2), (1, 0, 2, 1, 2), (0, 0, 0, 20, 15), (1, 4, 6, 6, 8)]
    for scale in [(1.0, 1.0), (0.5, 0.5), (1.8, 1.8), (3.0, 0.3), (0.0, 0.0), (1e-9, 2.5)]:
        rc, src, _, _, _ = layout(lib, ims, rects, sx=scale[0], sy=scale[1])
        assert rc == 0 and src == [ec.map_region(r, scale) for r in rects], scale
    # sx or sy equal to 0 means 1
    assert layout(lib, ims, rects, sx=0.0, sy=0.0)[1] == [tuple(r) for r in rects]


def test_margin_and_regions_left_outside_the_frame(lib):
    ims = [image(40, 30, 3), image(9, 9, 3)]
    rects = [(0, 10, 10, 10, 6), (0, -5, -5, 4, 4), (1, 100, 100, 7, 7), (0, 39, 29, 10, 10), (1, -50, 3, 9, 9), (0, 0, 0, 40, 30)]
    rc, src, ch, _, _ = layout(lib, ims, rects, margin=0.25)
    assert rc == 0 and ch == 3
    # cvRound(10 * 0.25) = 2 (2.5: the tie), cvRound(6 * 0.25) = 2 (1.5), cvRound(4 * 0.25) = 1, cvRound(7 * 0.25) = 2, cvRound(9 * 0.25) = 2
    assert src[0] == (0, 8, 8, 14, 10) and src[1] == (0, -6, -6, 6, 6) and src[2] == (1, 98, 98, 11, 11) and src[5] == (0, -10, -8, 60, 46)
    for scale, margin in [((1.0, 1.0), 0.25), ((1.8, 1.8), 0.1), ((0.5, 0.5), 0.5), ((1.0, 1.0), 3.0), ((2.5, 0.5), 0.0)]:
        rc, src, _, _, _ = layout(lib, ims, rects, sx=scale[0], sy=scale[1], margin=margin)
        assert rc == 0 and src == [ec.map_region(r, scale, margin) for r in rects], (scale, margin)


@pytest.mark.parametrize("flags", [0, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR])
def test_channels_and_bytes(lib, flags):
    rects = [(0, 1, 1, 5, 5), (0, 2, 2, 3, 3), (0, 0, 0, 8, 4)]
    for ch in (1, 3, 4):
        rc, _, c, nbytes, _ = layout(lib, [image(8, 4, ch), image(3, 3, 1)], rects, out_w=7, out_h=5, flags=flags)
        want = 1 if flags & VJ_EXTRACT_GRAY else ch
        assert rc == 0 and c == want and nbytes == 3 * 7 * 5 * want
    # mixed channel counts: only with VJ_EXTRACT_GRAY; a frame no region names does not count
    ims = [image(8, 4, 3), image(8, 4, 1), image(8, 4, 4)]
    rc, _, c, nbytes, err = layout(lib, ims, [(0, 0, 0, 2, 2), (2, 0, 0, 2, 2)], flags=flags)
    if flags & VJ_EXTRACT_GRAY:
        assert rc == 0 and c == 1 and nbytes == 2 * 24 * 24
    else:
        assert rc == VJ_ERR_ARG and "region 1" in err and "channels" in err and nbytes == 0
    rc, _, c, _, _ = layout(lib, ims, [(2, 0, 0, 2, 2), (2, 1, 1, 2, 2)], flags=flags)
    assert rc == 0 and c == (1 if flags & VJ_EXTRACT_GRAY else 4)
    # no region: VJ_OK, no bytes
    rc, _, _, nbytes, _ = layout(lib, ims, [], flags=flags)
    assert rc == 0 and nbytes == 0
    assert layout(lib, [], [], flags=flags)[0] == 0


def test_the_python_twin():
    frames = [np.zeros((30, 40, 3), np.uint8), np.zeros((9, 9, 3), np.uint8)]
    rects = np.array([(0, 5, 7, 5, 7), (1, 1, 3, 1, 3)], np.int32)
    src, ch, nbytes = extract_layout(frames, rects, (6, 4), scale=(0.5, 0.5))
    assert src.tolist() == [[0, 2, 4, 2, 4], [1, 0, 2, 1, 2]] and ch == 3 and nbytes == 2 * 6 * 4 * 3
    from clfacedetection_amd.api import RECT_DTYPE
    rr = np.zeros(2, RECT_DTYPE)
    for k, col in zip(("frame", "x", "y", "w", "h"), rects.T):
        rr[k] = col
    src2, ch, nbytes = extract_layout(frames, rr, (6, 4), scale=(0.5, 0.5), gray=True, planar=True)
    assert np.array_equal(src, src2) and ch == 1 and nbytes == 2 * 6 * 4
    src, ch, nbytes = extract_layout(np.zeros((2, 10, 12), np.uint8), [(1, 0, 0, 12, 10)], (3, 3), margin=0.25)
    assert src.tolist() == [[1, -3, -2, 18, 14]] and ch == 1 and nbytes == 9
    with pytest.raises(VjError):
        extract_layout(frames, rects, (6, 0))
    with pytest.raises(ValueError):
        extract_layout(frames, np.zeros((2, 5)), (6, 4))


def test_argument_errors(lib):
    ok = [image(8, 4), image(5, 3)]
    good = [(0, 0, 0, 4, 4), (1, 1, 1, 2, 2)]
    p = ExtractParams()
    lib.vj_extract_default(C.byref(p))
    p.out_w = p.out_h = 4
    arr = (_Image * 2)(*ok)
    r = np.array(good, np.int32)
    src = np.zeros((2, 5), np.int32)
    ch, n = C.c_int(0), C.c_uint64(0)
    f = lib.vj_extract_layout
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), src.ctypes.data, C.byref(ch), C.byref(n)) == 0
    # null arguments, negative counts
    assert f(None, 2, r.ctypes.data, 2, C.byref(p), src.ctypes.data, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, None, 2, C.byref(p), src.ctypes.data, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, None, src.ctypes.data, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), None, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), src.ctypes.data, None, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, 2, C.byref(p), src.ctypes.data, C.byref(ch), None) == VJ_ERR_ARG
    assert f(arr, -1, r.ctypes.data, 2, C.byref(p), src.ctypes.data, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, r.ctypes.data, -1, C.byref(p), src.ctypes.data, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    # a bad frame, by vj_detect_mixed's rules: the frame is named
    for bad in (image(8, 4, data=False), image(0, 4), image(8, -1), image(8, 4, stride=7), image(8, 4, 3, stride=23), image(8, 4, 2, stride=16)):
        rc, _, _, nbytes, err = layout(lib, ok + [bad], good)
        assert rc == VJ_ERR_ARG and "frame 2" in err and nbytes == 0
    # a region's frame index out of range, w <= 0, h <= 0: the row is named
    for bad in ((2, 0, 0, 4, 4), (-1, 0, 0, 4, 4), (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (1, 0, 0, -3, 4), (1, 0, 0, 4, -3)):
        rc, _, _, nbytes, err = layout(lib, ok, good + [bad])
        assert rc == VJ_ERR_ARG and "region 2" in err and nbytes == 0, bad
    # the fields: the field is named
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=0), "out_h"), (dict(out_w=-4), "out_w"), (dict(out_h=-1), "out_h"),
                     (dict(sx=-0.5), "sx"), (dict(sy=-0.5), "sy"), (dict(margin=-0.1), "margin"),
                     (dict(sx=math.inf), "sx"), (dict(sy=math.nan), "sy"), (dict(sx=math.nan), "sx"), (dict(margin=math.inf), "margin"),
                     (dict(margin=math.nan), "margin"),
                     (dict(flags=4), "flags"), (dict(flags=VJ_EXTRACT_GRAY | 1 << 31), "flags"), (dict(reserved=1), "reserved")]:
        rc, _, _, nbytes, err = layout(lib, ok, good, **kw)
        assert rc == VJ_ERR_ARG and word in err and nbytes == 0, kw
    # ... also without any region
    assert layout(lib, ok, [], reserved=1)[0] == VJ_ERR_ARG
    assert layout(lib, ok, [], out_w=0)[0] == VJ_ERR_ARG


def test_limits(lib):
    ims = [image(8, 4)]
    assert layout(lib, ims, [(0, 0, 0, 65535, 65535)], out_w=65535, out_h=1)[0] == 0
    assert layout(lib, ims, [(0, -(1 << 24), 1 << 23, 1, 1)])[0] == 0
    for rects, kw, word in [
            ([(0, 0, 0, 4, 4)], dict(out_w=65536), "65535"), ([(0, 0, 0, 4, 4)], dict(out_h=65536), "65535"),
            ([(0, 0, 0, 65536, 4)], {}, "65535"), ([(0, 0, 0, 4, 65536)], {}, "65535"),
            ([(0, 0, 0, 40000, 4)], dict(sx=2.0), "65535"), ([(0, 0, 0, 4, 4)], dict(sy=1e300), "65535"),
            ([(0, 0, 0, 40000, 4)], dict(margin=0.5), "65535"), ([(0, 0, 0, 4, 4)], dict(margin=1e300), "65535"),
            ([(0, (1 << 24) + 1, 0, 4, 4)], {}, "2^24"), ([(0, 0, -(1 << 24) - 1, 4, 4)], {}, "2^24"),
            ([(0, 1 << 23, 0, 4, 4)], dict(sx=3.0), "2^24"), ([(0, 1 << 24, 0, 4, 4)], {}, "2^24"),
            ([(0, -(1 << 24), 0, 4, 4)], dict(margin=0.5), "2^24")]:
        rc, _, _, nbytes, err = layout(lib, ims, [(0, 0, 0, 2, 2)] + rects, **kw)
        assert rc == VJ_ERR_LIMIT and word in err and nbytes == 0, (rects, kw)
        # the row or the field is named (a factor that takes every region beyond the limit names the first one)
        assert ("out_" if "out_w" in kw or "out_h" in kw else "region 0" if 1e300 in kw.values() else "region 1") in err, (rects, kw, err)
    # work units beyond a 32-bit index: a 65535 x 65535 output of 4 channels is 1024 x 4096 blocks of 64 slots x 16 rows
    many = [(0, 0, 0, 2, 2)] * 513
    rc, _, _, _, err = layout(lib, [image(8, 4, 4)], many, out_w=65535, out_h=65535)
    assert rc == VJ_ERR_LIMIT and "work units" in err
    assert layout(lib, [image(8, 4, 4)], many[:511], out_w=65535, out_h=65535)[0] == 0


# --------------------------------------------------------------------------------------------------- the premises of the GPU tests
def test_the_detector_finds_candidates_in_the_prepared_frames(oracle, cascades):
    """The many-regions test cuts every raw candidate of these frames; the colour sources it cuts from have them as their gray image."""
    c, a = cascades(pc.CASC)
    prepared = pc.e2e_prepared(oracle, True)
    counts = [len(oracle.detect_opencvlike(a, p)[0]) for p in prepared]
    print("raw candidates per frame:", counts)
    assert all(n > 0 for n in counts)
    assert counts == [69, 69, 40]                        # as tests/test_prep_cpu.py's premise finds them
    bgr = ec.e2e_bgr()
    assert bgr.shape == (3, pc.E2E_SRC_H, pc.E2E_SRC_W, 3)
    for f, g in zip(bgr, pc.e2e_frames()):
        assert np.array_equal(oracle.bgr2gray(np.ascontiguousarray(f)), g)
        assert (f[..., 0] != f[..., 2]).mean() > 0.5                         # ... and the channels differ


def test_the_crop_edge_case_tells_the_two_clamps_apart(oracle):
    """Clamping the taps at the crop against clamping them at the frame: the restatement on the crop differs from the same window
    of the resized whole frame, in the first and last columns and rows."""
    f = ec.edge_frame(1)
    _, x, y, w, h = ec.EDGE_RECT
    ow, oh = ec.EDGE_SIZE
    at_crop = ec.restate(oracle, [f], [ec.EDGE_RECT], ec.EDGE_SIZE)[0, :, :, 0]
    # the crop with 5 columns and 4 rows of the frame around it, at the crop's factors (1 / 3.2 = 5 / 16 and 1 / 2 are exact in binary,
    # so both resizes compute the same fractions): 30 x 25 -> 96 x 50, the crop's window at (16, 8)
    assert x - 5 >= 0 and y - 4 >= 0 and x + w + 5 <= ec.EDGE_FRAME_W and y + h + 4 <= ec.EDGE_FRAME_H
    whole = so.resize_linear(np.ascontiguousarray(f[y - 4:y + h + 4, x - 5:x + w + 5]), 96, 50)
    at_frame = whole[8:8 + oh, 16:16 + ow]
    assert at_crop.shape == at_frame.shape == (oh, ow)
    assert not np.array_equal(at_crop, at_frame)
    assert np.array_equal(at_crop[2:-2, 2:-2], at_frame[2:-2, 2:-2])          # the interior does not see the difference ...
    assert int(at_crop.max()) <= 60 < int(at_frame[0].max())                  # ... the edges do: the neighbours' pixels leak in
