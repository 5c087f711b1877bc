"""vj_extract_affine_layout, vj_affine_from_rect, vj_affine_from_eyes and align_transforms through ctypes (host only, no device): the
channel count and the byte count for every flag combination, every argument error and limit of DESIGN.md §4.19 with its message, the
two matrix helpers against their restatement bit for bit, the pairing rule on hand-made results.  And the premises of
tests/test_gpu_affine.py, with the restatement of tests/affine_cases.py alone: it agrees with three computations that do not share
its arithmetic; the tie family tells round-half-even from round-half-up; the rotation case has fractional positions and clamped
taps and depends on the +16; the end-to-end frames yield the stated faces and pairs."""
import ctypes as C
import math

import numpy as np
import pytest

import affine_cases as ac
import cv_rois_cases as cc
import extract_cases as ec
import prep_cases as pc
from clfacedetection_amd import (AFFINE_DTYPE, AffineParams, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VjError, affine_from_eyes, affine_from_rect,
                                 align_transforms, extract_affine_layout)
from clfacedetection_amd.api import _Image

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(64, np.uint8)
LIM = 2.0 ** 19


def image(w, h, ch=1, stride=None, data=True, on_device=0):
    return _Image(PX.ctypes.data if data else None, w, h, w * max(ch, 1) if stride is None else stride, on_device, ch)


def affines(rows):
    """rows of (frame, m0 .. m5) or (frame, reserved, m0 .. m5) -> AFFINE_DTYPE array"""
    a = np.zeros(len(rows), AFFINE_DTYPE)
    for i, r in enumerate(rows):
        a[i] = (r[0], 0, r[1:]) if len(r) == 7 else (r[0], r[1], r[2:])
    return a


def layout(lib, images, rows, **kw):
    """-> (rc, channels, bytes, last error)"""
    p = AffineParams()
    lib.vj_affine_default(C.byref(p))
    p.out_w, p.out_h = 24, 24
    for k, v in kw.items():
        setattr(p, k, v)
    n = len(images)
    arr = (_Image * max(n, 1))(*images)
    a = affines(rows)
    ch, nbytes = C.c_int(77), C.c_uint64(12345)
    rc = lib.vj_extract_affine_layout(arr, n, a.ctypes.data, len(a), C.byref(p), C.byref(ch), C.byref(nbytes))
    return rc, int(ch.value), int(nbytes.value), lib.vj_last_error().decode()


ID = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def test_default_and_the_struct_sizes(lib):
    p = AffineParams(1, 2, 3, 4)
    lib.vj_affine_default(C.byref(p))
    assert (p.out_w, p.out_h, p.flags, p.reserved) == (0, 0, 0, 0)
    lib.vj_affine_default(None)
    assert AFFINE_DTYPE.itemsize == 56 and C.sizeof(AffineParams) == 16


@pytest.mark.parametrize("flags", [0, VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, VJ_EXTRACT_GRAY | VJ_EXTRACT_PLANAR])
def test_channels_and_bytes(lib, flags):
    rows = [(0,) + ID, (0,) + tuple(ac.ROT), (0,) + tuple(ac.SHEAR)]
    for ch in (1, 3, 4):
        rc, c, nbytes, _ = layout(lib, [image(8, 4, ch), image(3, 3, 1)], rows, out_w=7, out_h=5, flags=flags)
        want = 1 if flags & VJ_EXTRACT_GRAY else ch
        assert rc == 0 and c == want and nbytes == 3 * 7 * 5 * want
    # mixed channel counts: only with VJ_EXTRACT_GRAY; a frame no affine names does not count
    ims = [image(8, 4, 3), image(8, 4, 1), image(8, 4, 4)]
    rc, c, nbytes, err = layout(lib, ims, [(0,) + ID, (2,) + ID], flags=flags)
    if flags & VJ_EXTRACT_GRAY:
        assert rc == 0 and c == 1 and nbytes == 2 * 24 * 24
    else:
        assert rc == VJ_ERR_ARG and "affine 1" in err and "channels" in err and nbytes == 0
    rc, c, _, _ = layout(lib, ims, [(2,) + ID, (2,) + ID], flags=flags)
    assert rc == 0 and c == (1 if flags & VJ_EXTRACT_GRAY else 4)
    # no affine: VJ_OK, no bytes
    rc, _, nbytes, _ = layout(lib, ims, [], flags=flags)
    assert rc == 0 and nbytes == 0
    assert layout(lib, [], [], flags=flags)[0] == 0


def test_the_python_twin():
    frames = [np.zeros((30, 40, 3), np.uint8), np.zeros((9, 9, 3), np.uint8)]
    rows = np.array([(0,) + ID, (1,) + tuple(ac.ROT)], np.float64)
    assert extract_affine_layout(frames, rows, (6, 4)) == (3, 2 * 6 * 4 * 3)
    assert extract_affine_layout(frames, affines([tuple(r) for r in rows]), (6, 4), gray=True, planar=True) == (1, 2 * 6 * 4)
    assert extract_affine_layout(np.zeros((2, 10, 12), np.uint8), [(1,) + ID], (3, 3)) == (1, 9)
    with pytest.raises(VjError):
        extract_affine_layout(frames, rows, (6, 0))
    with pytest.raises(ValueError):
        extract_affine_layout(frames, [(0.5,) + ID], (6, 4))


def test_argument_errors(lib):
    ok = [image(8, 4), image(5, 3)]
    good = [(0,) + ID, (1,) + tuple(ac.ROT)]
    p = AffineParams(4, 4, 0, 0)
    arr = (_Image * 2)(*ok)
    a = affines(good)
    ch, n = C.c_int(0), C.c_uint64(0)
    f = lib.vj_extract_affine_layout
    assert f(arr, 2, a.ctypes.data, 2, C.byref(p), C.byref(ch), C.byref(n)) == 0 and n.value == 32
    # null arguments, negative counts
    assert f(None, 2, a.ctypes.data, 2, C.byref(p), C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, None, 2, C.byref(p), C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, a.ctypes.data, 2, None, C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, a.ctypes.data, 2, C.byref(p), None, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, a.ctypes.data, 2, C.byref(p), C.byref(ch), None) == VJ_ERR_ARG
    assert f(arr, -1, a.ctypes.data, 2, C.byref(p), C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, a.ctypes.data, -1, C.byref(p), C.byref(ch), C.byref(n)) == VJ_ERR_ARG
    assert "null" in lib.vj_last_error().decode()
    # a bad frame, by vj_detect_mixed's rules: the frame is named
    for bad in (image(8, 4, data=False), image(0, 4), image(8, -1), image(8, 4, stride=7), image(8, 4, 3, stride=23), image(8, 4, 2, stride=16)):
        rc, _, nbytes, err = layout(lib, ok + [bad], good)
        assert rc == VJ_ERR_ARG and "frame 2" in err and nbytes == 0
    # a frame index out of range, reserved != 0: the row and the field are named
    for bad, word in (((2,) + ID, "frame"), ((-1,) + ID, "frame"), ((0, 5) + ID, "reserved")):
        rc, _, nbytes, err = layout(lib, ok, good + [bad])
        assert rc == VJ_ERR_ARG and "affine 2" in err and word in err and nbytes == 0, bad
    # a non-finite matrix entry: the row and the entry are named
    for i in range(6):
        for v in (math.nan, math.inf, -math.inf):
            m = list(ID)
            m[i] = v
            rc, _, nbytes, err = layout(lib, ok, good + [(1,) + tuple(m)])
            assert rc == VJ_ERR_ARG and "affine 2" in err and f"m[{i}]" in err and "finite" in err and nbytes == 0, (i, v)
    # the fields: the field is named
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=0), "out_h"), (dict(out_w=-4), "out_w"), (dict(out_h=-1), "out_h"),
                     (dict(flags=4), "flags"), (dict(flags=VJ_EXTRACT_GRAY | 1 << 31), "flags"), (dict(reserved=1), "reserved")]:
        rc, _, nbytes, err = layout(lib, ok, good, **kw)
        assert rc == VJ_ERR_ARG and word in err and nbytes == 0, kw
    # ... also without any affine
    assert layout(lib, ok, [], reserved=1)[0] == VJ_ERR_ARG
    assert layout(lib, ok, [], out_w=0)[0] == VJ_ERR_ARG


def test_limits(lib):
    ims = [image(8, 4)]
    assert layout(lib, ims, [(0,) + ID], out_w=65535, out_h=1)[0] == 0
    for kw in (dict(out_w=65536), dict(out_h=65536), dict(out_w=2**31 - 1, out_h=2**31 - 1)):
        rc, _, nbytes, err = layout(lib, ims, [(0,) + ID], **kw)
        assert rc == VJ_ERR_LIMIT and "65535" in err and nbytes == 0, kw
    # each magnitude at 2^19 passes, one step above it does not.  out_w = out_h = 17, so out_w - 1 = out_h - 1 = 16 and every
    # product below is exact: |m0| 16, |m3| 16, |m2|, |m5|, |m1 16 + m2|, |m4 16 + m5|
    up, s, s_up = math.nextafter(LIM, math.inf), 2.0 ** 15, math.nextafter(2.0 ** 15, math.inf)
    for i, (at, over, word) in enumerate([
            ((s, 0, 0, 0, 1, 0), (s_up, 0, 0, 0, 1, 0), "m[0]"),
            ((1, 0, 0, -s, 1, 0), (1, 0, 0, -s_up, 1, 0), "m[3]"),
            ((1, 0, LIM, 0, 1, 0), (1, 0, up, 0, 1, 0), "m[2]"),
            ((1, 0, 0, 0, 1, -LIM), (1, 0, 0, 0, 1, -up), "m[5]"),
            ((1, 1, LIM - 16, 0, 1, 0), (1, 1, LIM - 15, 0, 1, 0), "m[1]"),
            ((1, 0, 0, 0, -2, -LIM + 32), (1, 0, 0, 0, -2, -LIM + 31), "m[4]"),
            ((1, -s, 0, 0, 1, 0), (1, -s, -1, 0, 1, 0), "m[1]")]):
        assert layout(lib, ims, [(0,) + ID, (0,) + tuple(float(v) for v in at)], out_w=17, out_h=17)[0] == 0, (i, at)
        rc, _, nbytes, err = layout(lib, ims, [(0,) + ID, (0,) + tuple(float(v) for v in over)], out_w=17, out_h=17)
        assert rc == VJ_ERR_LIMIT and "affine 1" in err and word in err and "2^19" in err and nbytes == 0, (i, over, err)
    # at the bound itself the restatement's sums stay inside int32 (positions() asserts it)
    ac.positions([s, 0.0, LIM, -s, 0.0, -LIM], (17, 17))
    ac.positions([-s, s, -LIM, s, -s, LIM], (17, 17))
    # work units beyond a 32-bit index: a 65535 x 65535 output of 4 channels is 1024 x 4096 blocks of 64 slots x 16 rows
    many = [(0,) + ID] * 513
    rc, _, _, err = layout(lib, [image(8, 4, 4)], many, out_w=65535, out_h=65535)
    assert rc == VJ_ERR_LIMIT and "work units" in err
    assert layout(lib, [image(8, 4, 4)], many[:511], out_w=65535, out_h=65535)[0] == 0


# ------------------------------------------------------------------------------------------------------------ the matrix helpers
def bits(m):
    return np.asarray(m, np.float64).view(np.uint64).tolist()


def test_affine_from_rect_bit_for_bit(lib):
    for x, y, w, h, size in [(0, 0, 37, 29, (37, 29)), (8, 6, 20, 17, (64, 34)), (-3.5, 2.25, 10.1, 7.3, (3, 7)), (100, 50, 300, 300, (112, 112)),
                             (1e5, -1e5, 1e-3, 1e3, (5, 9)), (0.1, 0.2, 0.3, 0.7, (1, 1)), (33, 44, 97, 97, (32, 32)), (12, 13, 50, 60, (224, 224)),
                             (7, 7, 1, 1, (9, 9)), (1 / 3, 2 / 3, 100 / 7, 100 / 9, (11, 13)), (5, 5, 24, 24, (24, 24)), (0, 0, 1920, 1080, (1920, 1080))]:
        assert bits(affine_from_rect(x, y, w, h, size)) == bits(ac.from_rect(x, y, w, h, size)), (x, y, w, h, size)
    m = affine_from_rect(5, 6, 24, 20, (24, 20))
    assert m.tolist() == [1.0, 0.0, 5.0, 0.0, 1.0, 6.0]                       # a box of the output's size: an integer translation
    out = (C.c_double * 6)()
    f = lib.vj_affine_from_rect
    assert f(0.0, 0.0, 4.0, 4.0, 4, 4, None) == VJ_ERR_ARG
    for bad in [(math.nan, 0, 4, 4, 4, 4), (0, math.inf, 4, 4, 4, 4), (0, 0, 0, 4, 4, 4), (0, 0, 4, -1, 4, 4), (0, 0, math.inf, 4, 4, 4), (0, 0, 4, 4, 0, 4),
                (0, 0, 4, 4, 4, -2)]:
        assert f(*[float(v) for v in bad[:4]], bad[4], bad[5], out) == VJ_ERR_ARG, bad
        assert "vj_affine_from_rect" in lib.vj_last_error().decode()


def test_affine_from_eyes_bit_for_bit(lib):
    cases = [((30, 40, 70, 40), (112, 112), (0.3, 0.7, 0.35)), ((30, 40, 70, 52), (112, 112), (0.3, 0.7, 0.35)), ((30, 52, 70, 40), (112, 112), (0.3, 0.7, 0.35)),   # level, ry > ly, ry < ly
             ((50, 20, 50, 60), (32, 32), (0.3, 0.7, 0.35)),                                          # a vertical eye line
             ((50, 60, 50, 20), (32, 32), (0.25, 0.75, 0.4)), ((70, 40, 30, 40), (64, 48), (0.3, 0.7, 0.35)),   # upside down, mirrored
             ((100.25, 200.5, 180.75, 190.125), (224, 224), (0.35, 0.65, 0.3)), ((1 / 3, 2 / 3, 10 / 3, 1 / 7), (7, 5), (0.1, 0.9, 0.5)),
             ((1e4, -1e4, 1e4 + 1e-3, -1e4), (96, 112), (0.3, 0.7, 0.35)), ((0, 0, 1, 0), (1, 1), (0.0, 1.0, 0.0)),
             ((12.5, 13.5, 40.5, 14.5), (32, 32), (0.3, 0.7, 0.35)), ((300, 300, 500, 380), (160, 160), (0.31, 0.69, 0.36))]
    assert len(cases) == 12
    for eyes, size, pos in cases:
        got = affine_from_eyes(*eyes, size, pos)
        assert bits(got) == bits(ac.from_eyes(*eyes, size, pos)), (eyes, size, pos)
        # the eyes land where they should: m maps the output places onto them
        for (ox, oy), (ex, ey) in zip(((pos[0] * size[0], pos[2] * size[1]), (pos[1] * size[0], pos[2] * size[1])), (eyes[:2], eyes[2:])):
            assert abs(got[0] * ox + got[1] * oy + got[2] - ex) <= 1e-9 * max(1.0, abs(ex)) and abs(got[3] * ox + got[4] * oy + got[5] - ey) <= 1e-9 * max(1.0, abs(ey))
    out = (C.c_double * 6)()
    f = lib.vj_affine_from_eyes
    assert f(0.0, 0.0, 1.0, 0.0, 4, 4, 0.3, 0.7, 0.35, None) == VJ_ERR_ARG
    for bad, word in [((math.nan, 0, 1, 0, 4, 4, 0.3, 0.7, 0.35), "finite"), ((0, 0, 1, math.inf, 4, 4, 0.3, 0.7, 0.35), "finite"),
                      ((0, 0, 1, 0, 4, 4, 0.3, math.nan, 0.35), "finite"), ((0, 0, 1, 0, 0, 4, 0.3, 0.7, 0.35), "out_w"),
                      ((0, 0, 1, 0, 4, 4, 0.7, 0.3, 0.35), "ex_r"), ((0, 0, 1, 0, 4, 4, 0.5, 0.5, 0.35), "ex_r"), ((3, 4, 3, 4, 4, 4, 0.3, 0.7, 0.35), "coincide")]:
        assert f(*[float(v) for v in bad[:4]], bad[4], bad[5], *[float(v) for v in bad[6:]], out) == VJ_ERR_ARG, bad
        assert word in lib.vj_last_error().decode(), bad


# ---------------------------------------------------------------------------------------------------------------- the pairing rule
def check_align(faces, eyes, size, **kw):
    got, paired = align_transforms(ac.rects(faces), ac.rects(eyes), size, **kw)
    want, want_paired = ac.align(ac.rects(faces), ac.rects(eyes), size, **kw)
    assert got.dtype == AFFINE_DTYPE and paired.dtype == bool and len(got) == len(faces)
    assert paired.tolist() == want_paired
    assert bits(ac.as_rows(got)) == bits(want)
    return got, paired


def test_pairing_rule_on_hand_made_results():
    face = (0, 60, 40, 80, 80, 0.0)
    le, re_, low = (0, 12, 18, 20, 16, 2.0), (0, 46, 22, 20, 16, 3.0), (0, 30, 60, 20, 16, 9.0)
    # no eyes: the box
    got, paired = check_align([face], [], (32, 32))
    assert paired.tolist() == [False] and got["m"][0].tolist() == ac.from_rect(60, 40, 80, 80, (32, 32))
    # one eye: the box
    assert check_align([face], [le], (32, 32))[1].tolist() == [False]
    # two eyes on one side: the box
    assert check_align([face], [le, (0, 2, 20, 20, 16, 5.0)], (32, 32))[1].tolist() == [False]
    # both eyes: the similarity through their centres, (60 + 12 + 10, 40 + 18 + 8) and (60 + 46 + 10, 40 + 22 + 8)
    got, paired = check_align([face], [le, re_], (32, 32))
    assert paired.tolist() == [True] and got["m"][0].tolist() == ac.from_eyes(82.0, 66.0, 116.0, 70.0, (32, 32))
    # an eye in the lower half does not count, whatever its weight: centre y = 60 + 8 = 68 >= 40
    assert check_align([face], [le, low], (32, 32))[1].tolist() == [False]
    got2, paired = check_align([face], [low, le, re_], (32, 32))
    assert paired.tolist() == [True] and bits(got2["m"]) == bits(got["m"])
    # the greatest weight wins; a weight tie goes to the lowest index
    heavy = (0, 50, 10, 20, 16, 7.0)
    got, _ = check_align([face], [le, re_, heavy], (32, 32))
    assert got["m"][0].tolist() == ac.from_eyes(82.0, 66.0, 120.0, 58.0, (32, 32))
    tie_a, tie_b = (0, 46, 22, 20, 16, 3.0), (0, 50, 10, 20, 16, 3.0)
    assert check_align([face], [le, tie_a, tie_b], (32, 32))[0]["m"][0].tolist() == ac.from_eyes(82.0, 66.0, 116.0, 70.0, (32, 32))
    assert check_align([face], [le, tie_b, tie_a], (32, 32))[0]["m"][0].tolist() == ac.from_eyes(82.0, 66.0, 120.0, 58.0, (32, 32))
    # a centre exactly at w / 2 is a right eye; exactly at h / 2 it is not in the upper half
    assert check_align([face], [le, (0, 30, 20, 20, 16, 1.0)], (32, 32))[1].tolist() == [True]
    assert check_align([face], [le, (0, 46, 32, 20, 16, 1.0)], (32, 32))[1].tolist() == [False]
    # eyes belong to the face their `frame` names; the affine's frame is the face's; scale and eye_pos reach the matrices
    faces = [face, (2, 10, 10, 40, 40, 0.0)]
    eyes = [(1, 4, 6, 10, 8, 1.0), (1, 24, 6, 10, 8, 1.0), (0, 12, 18, 20, 16, 2.0)]
    got, paired = check_align(faces, eyes, (48, 40), scale=(3.0, 1.8), eye_pos=(0.25, 0.75, 0.4))
    assert paired.tolist() == [False, True] and got["frame"].tolist() == [0, 2]
    assert got["m"][0].tolist() == ac.from_rect(180.0, 72.0, 240.0, 144.0, (48, 40))
    assert got["m"][1].tolist() == ac.from_eyes(19.0 * 3.0, 20.0 * 1.8, 39.0 * 3.0, 20.0 * 1.8, (48, 40), (0.25, 0.75, 0.4))
    # the hand-made case of the GPU test has both branches
    assert check_align(ac.HAND_FACES, ac.HAND_EYES, ac.E2E_SIZE, scale=ec.MANY_SCALE)[1].tolist() == [True, False, True]
    # no faces
    got, paired = align_transforms(ac.rects([]), ac.rects([]), (32, 32))
    assert len(got) == 0 and len(paired) == 0


# --------------------------------------------------------------------------------------------------- the premises of the GPU tests
@pytest.fixture(scope="module")
def frame():
    return np.random.default_rng(5).integers(1, 256, (ac.H, ac.W, 3), dtype=np.uint8)


def test_identity_translation_and_quarter_turn(oracle, frame):
    """Three computations that do not share the restatement's arithmetic."""
    assert np.array_equal(ac.warp(oracle, frame, ac.identity(), (ac.W, ac.H)), frame)
    assert np.array_equal(ac.warp(oracle, frame[:, :, 0], ac.identity(), (ac.W, ac.H))[:, :, 0], frame[:, :, 0])
    for tx, ty, w, h in [(3, 4, 10, 8), (-5, 8, 10, 10), (30, 8, 10, 10), (8, -5, 10, 10), (8, 25, 10, 10), (-3, -3, 10, 10), (30, 22, 10, 10),
                         (100, 100, 6, 6), (-40, 3, 6, 6), (-4, -4, ac.W + 8, ac.H + 8)]:
        assert np.array_equal(ac.warp(oracle, frame, ac.translation(tx, ty), (w, h)), ec.padded_crop(frame, tx, ty, w, h)), (tx, ty)
    for x0, y0, ow, oh in [(5, 3, 12, 9), (0, 0, ac.H, ac.W), (20, 15, 14, 20), (-4, -2, 10, 10)]:
        got = ac.warp(oracle, frame, ac.quarter_turn(x0, y0, ow), (ow, oh))
        crop = ec.padded_crop(frame, x0, y0, oh, ow)                      # oh columns, ow rows of the source
        want = crop[::-1].transpose(1, 0, 2)                              # out[y][x] = crop[ow - 1 - x][y]
        assert np.array_equal(got, want), (x0, y0)
    # gray: the taps through BGR2GRAY
    assert np.array_equal(ac.warp(oracle, frame, ac.translation(-3, 2), (20, 20), gray=True)[:, :, 0],
                          ec.padded_crop(oracle.bgr2gray(frame), -3, 2, 20, 20))


def test_the_tie_family_tells_half_even_from_half_up(oracle, frame):
    differ = [int((ac.warp(oracle, frame, m, ac.TIE_SIZE) != ac.warp(oracle, frame, m, ac.TIE_SIZE, rnd=ac.half_up)).sum()) for m in ac.tie_family()]
    print("bytes that differ per member:", differ, "in all:", sum(differ))
    assert len(differ) == 32 and max(differ) >= 1


def test_the_rotation_case_has_fractions_clamped_taps_and_needs_the_offset(oracle, frame):
    frac, clamped = ac.touches(ac.ROT, ac.ROT_SIZE, ac.W, ac.H)
    print(f"rotation case: {frac} of {ac.ROT_SIZE[0] * ac.ROT_SIZE[1]} samples with a fractional position, {clamped} with a clamped tap")
    assert frac > 0 and clamped > 0 and clamped < ac.ROT_SIZE[0] * ac.ROT_SIZE[1]
    a, b = ac.warp(oracle, frame, ac.ROT, ac.ROT_SIZE), ac.warp(oracle, frame, ac.ROT, ac.ROT_SIZE, offset=0)
    assert not np.array_equal(a, b)
    for m in ac.edge_matrices()[:8]:
        f, c = ac.touches(m, (12, 10), ac.W, ac.H)
        assert f > 0 and 0 < c < 120                                       # across the border, not wholly outside
    for m in ac.edge_matrices()[8:]:
        assert ac.touches(m, (12, 10), ac.W, ac.H)[1] == 120               # wholly outside


def e2e_oracle_results(oracle, cascades):
    """(faces, eyes) of the end-to-end case as RECT-like arrays, from the oracle: the grouped faces and, per face, the raw candidates
    of the eye cascade in the library's order (scale_idx, y, x), weight 0 as the library leaves it for raw results."""
    c1, a1 = cascades(pc.CASC)
    c2, a2 = cascades("eye")
    regions, res = pc.once("cv_chain", lambda: cc.oracle_chain(oracle, a1, a2, pc.e2e_prepared(oracle), 3))
    faces = ac.rects([(int(f), int(x), int(y), int(w), int(h), 0.0) for f, x, y, w, h in regions])
    eyes = []
    for i, (r, _) in enumerate(res):
        r = r[np.lexsort((r["x"], r["y"], r["scale_idx"]))]
        eyes += [(i, int(v["x"]), int(v["y"]), int(v["w"]), int(v["h"]), 0.0) for v in r]
    return faces, ac.rects(eyes)


def test_the_end_to_end_frames_yield_faces_and_pairs(oracle, cascades):
    faces, eyes = e2e_oracle_results(oracle, cascades)
    rows, paired = ac.align(faces, eyes, ac.E2E_SIZE, scale=ec.MANY_SCALE)
    print(f"end to end: {len(faces)} faces, {len(eyes)} eye candidates, {sum(paired)} faces paired")
    assert len(faces) == ac.E2E_FACES and sum(paired) == ac.E2E_PAIRED
    got, got_paired = align_transforms(faces, eyes, ac.E2E_SIZE, scale=ec.MANY_SCALE)
    assert got_paired.tolist() == paired and bits(ac.as_rows(got)) == bits(rows)
    # every matrix is inside the limits: the call is accepted
    assert extract_affine_layout(list(ec.e2e_bgr()), got, ac.E2E_SIZE) == (3, len(faces) * 32 * 32 * 3)
