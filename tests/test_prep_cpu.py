"""vj_preprocess_layout through ctypes (host only, no device): destination sizes from dst_w / dst_h, from factors (cvRound ties
included) and without a resize; strides, offsets and the byte count; every argument error and the limits.  And the premise of the
end-to-end tests of tests/test_gpu_prep.py, with the existing oracles alone: preprocessing changes what the detector finds in the
frames chosen there, and the detector finds something in them."""
import ctypes as C
import math

import numpy as np
import pytest

import mixed_cases as mc
import prep_cases as pc
from clfacedetection_amd import Prep, VJ_PREP_EQUALIZE, VjError, preprocess_layout
from clfacedetection_amd.api import _Image

VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
PX = np.zeros(64, np.uint8)


def image(w, h, ch=1, stride=None, data=True, on_device=0):
    return _Image(PX.ctypes.data if data else None, w, h, w * max(ch, 1) if stride is None else stride, on_device, ch)


def layout(lib, images, **kw):
    """-> (rc, [(offset, w, h, stride, on_device, channels)], bytes, last error)"""
    p = Prep()
    lib.vj_prep_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    n = len(images)
    arr = (_Image * max(n, 1))(*images)
    out = (_Image * max(n, 1))()
    nbytes = C.c_uint64(12345)
    rc = lib.vj_preprocess_layout(arr, n, C.byref(p), out, C.byref(nbytes))
    return rc, [(int(o.data or 0), o.width, o.height, o.stride, o.on_device, o.channels) for o in out[:n]], int(nbytes.value), lib.vj_last_error().decode()


def check_geometry(recs, sizes):
    """Strides rounded to 4, offsets at multiples of 256, no overlap, in order; returns the exact byte count."""
    end = 0
    for (off, w, h, stride, dev, ch), (dw, dh) in zip(recs, sizes):
        assert (w, h) == (dw, dh) and stride == (dw + 3) // 4 * 4 and dev == 1 and ch == 1
        assert off % 256 == 0 and off >= end and off - end < 256
        end = off + stride * h
    return end


def test_default_is_all_zero(lib):
    p = Prep(1, 2, 3.0, 4.0, 5, 6)
    lib.vj_prep_default(C.byref(p))
    assert (p.dst_w, p.dst_h, p.fx, p.fy, p.flags, p.reserved) == (0, 0, 0.0, 0.0, 0, 0)
    lib.vj_prep_default(None)


def test_sizes_from_dst_w_and_dst_h(lib):
    ims = [image(w, h, ch) for (w, h), ch in zip(mc.SIZES, [1, 3, 4] * 4)]
    for dw, dh in [(1, 1), (5, 3), (240, 180), (257, 2), (65535, 1)]:
        rc, recs, nbytes, _ = layout(lib, ims, dst_w=dw, dst_h=dh, flags=VJ_PREP_EQUALIZE)
        assert rc == 0
        assert check_geometry(recs, [(dw, dh)] * len(ims)) == nbytes


def test_sizes_from_factors_and_the_ties_of_cv_round(lib):
    rc, recs, nbytes, _ = layout(lib, [image(5, 7), image(7, 5), image(1, 1), image(3, 9, 3), image(300, 200)], fx=0.5, fy=0.5)
    assert rc == 0
    want = [(2, 4), (4, 2), (1, 1), (2, 4), (150, 100)]       # 2.5 -> 2, 3.5 -> 4, 0.5 -> 0 -> at least 1, 1.5 -> 2, 4.5 -> 4
    assert check_geometry(recs, want) == nbytes
    ims = [image(w, h) for w, h in mc.SIZES]
    for fx, fy in [(0.5, 0.5), (1.0, 1.0), (0.3, 1.7), (2.0, 0.01), (1e-9, 1e-9)]:
        rc, recs, nbytes, _ = layout(lib, ims, fx=fx, fy=fy)
        assert rc == 0
        want = [pc.dst_size(w, h, fx=fx, fy=fy) for w, h in mc.SIZES]
        assert check_geometry(recs, want) == nbytes
        assert all(min(s) >= 1 for s in want)
    # dst_w / dst_h come first when both pairs are set
    rc, recs, _, _ = layout(lib, ims, dst_w=9, dst_h=8, fx=0.5, fy=0.5)
    assert rc == 0 and all(r[1:3] == (9, 8) for r in recs)


def test_no_resize_and_no_frames(lib):
    sizes = list(mc.SIZES) + [(w, 1 + w % 5) for w in range(1, 10)]
    rc, recs, nbytes, _ = layout(lib, [image(w, h) for w, h in sizes])
    assert rc == 0 and check_geometry(recs, sizes) == nbytes
    assert nbytes == recs[-1][0] + recs[-1][3] * recs[-1][2]           # exact: the end of the last image
    rc, recs, nbytes, _ = layout(lib, [])
    assert rc == 0 and nbytes == 0
    p = Prep()
    n = C.c_uint64(7)
    assert lib.vj_preprocess_layout(None, 0, C.byref(p), None, C.byref(n)) == 0 and n.value == 0


def test_the_python_twin(lib):
    frames = [np.zeros((h, w), np.uint8) for w, h in mc.SIZES[:4]] + [np.zeros((9, 7, 3), np.uint8)]
    recs, nbytes = preprocess_layout(frames, fx=0.5, fy=0.5)
    want = [pc.dst_size(w, h, fx=0.5, fy=0.5) for w, h in mc.SIZES[:4]] + [(4, 4)]
    assert [(r[1], r[2]) for r in recs] == want and nbytes == recs[-1][0] + recs[-1][3] * recs[-1][2]
    recs, nbytes = preprocess_layout(np.zeros((3, 10, 12), np.uint8), size=(6, 5), equalize=True)
    assert recs == [(0, 6, 5, 8), (256, 6, 5, 8), (512, 6, 5, 8)] and nbytes == 552
    with pytest.raises(ValueError):
        preprocess_layout(frames, fx=0.5)
    with pytest.raises(VjError):
        preprocess_layout(frames, size=(4, 0))


def test_argument_errors(lib):
    ok = [image(8, 4), image(5, 3, 3)]
    p = Prep()
    out = (_Image * 2)()
    n = C.c_uint64(0)
    arr = (_Image * 2)(*ok)
    f = lib.vj_preprocess_layout
    assert f(arr, 2, C.byref(p), out, C.byref(n)) == 0
    # null arguments, a negative count
    assert f(None, 2, C.byref(p), out, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, None, out, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, C.byref(p), None, C.byref(n)) == VJ_ERR_ARG
    assert f(arr, 2, C.byref(p), out, None) == VJ_ERR_ARG
    assert f(arr, -1, C.byref(p), out, C.byref(n)) == VJ_ERR_ARG
    # a bad frame, by vj_detect_mixed's rules: the frame is named
    for bad in (image(8, 4, data=False), image(0, 4), image(8, -1), image(8, 4, stride=7), image(8, 4, 3, stride=23), image(8, 4, 2, stride=16)):
        rc, _, nbytes, err = layout(lib, ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err and nbytes == 0
    # one of a pair without the other, negative sizes, non-finite or negative factors: the field is named
    for kw, word in [(dict(dst_w=5), "dst_w"), (dict(dst_h=5), "dst_h"), (dict(dst_w=-5, dst_h=-5), "dst_w"), (dict(dst_w=5, dst_h=-1), "dst_h"),
                     (dict(fx=0.5), "fx"), (dict(fy=0.5), "fy"), (dict(fx=-0.5, fy=-0.5), "fx"), (dict(fx=0.5, fy=-0.5), "fy"),
                     (dict(fx=math.inf, fy=1.0), "fx"), (dict(fx=1.0, fy=math.nan), "fy"), (dict(fx=math.nan, fy=math.nan), "fx"),
                     (dict(dst_w=5, dst_h=5, fx=math.nan, fy=1.0), "fx"),
                     (dict(flags=2), "flags"), (dict(flags=VJ_PREP_EQUALIZE | 1 << 31), "flags"), (dict(reserved=1), "reserved")]:
        rc, _, nbytes, err = layout(lib, ok, **kw)
        assert rc == VJ_ERR_ARG and word in err and nbytes == 0, kw
    # ... also without any frame
    assert layout(lib, [], reserved=1)[0] == VJ_ERR_ARG


def test_limits(lib):
    assert layout(lib, [image(65535, 1, stride=65535)], dst_w=65535, dst_h=65535)[0] == 0
    for ims, kw in [([image(65536, 1, stride=65536)], {}), ([image(1, 65536, stride=1)], {}),
                    ([image(8, 4)], dict(dst_w=65536, dst_h=1)), ([image(8, 4)], dict(dst_w=1, dst_h=65536)),
                    ([image(8, 4), image(40000, 4, stride=40000)], dict(fx=2.0, fy=1.0)), ([image(8, 4)], dict(fx=1.0, fy=1e300))]:
        rc, _, nbytes, err = layout(lib, ims, **kw)
        assert rc == VJ_ERR_LIMIT and "65535" in err and "frame %d" % (len(ims) - 1) in err and nbytes == 0
    # work units beyond a 32-bit index: 256 x 2048 blocks of 256 x 32 pixels per 65535 x 65535 image
    ims = [image(4, 4)] * 4097
    rc, _, _, err = layout(lib, ims, dst_w=65535, dst_h=65535)
    assert rc == VJ_ERR_LIMIT and "work units" in err
    assert layout(lib, ims[:4095], dst_w=65535, dst_h=65535)[0] == 0


# --------------------------------------------------------------------------------------- the premise of the end-to-end GPU tests
def test_preprocessing_changes_what_the_detector_finds(oracle, cascades):
    c, a = cascades(pc.CASC)
    frames = pc.e2e_frames()
    prepared = pc.e2e_prepared(oracle, True)
    plain = pc.e2e_prepared(oracle, False)
    assert prepared.shape == (3, pc.E2E_SIZE[1], pc.E2E_SIZE[0])
    found = 0
    for f, g, p in zip(frames, plain, prepared):
        assert not np.array_equal(g, p)                                   # equalization changes the resized image ...
        for detect in (lambda x: oracle.detect_opencvlike(a, x)[0], lambda x: oracle.detect(a, x)[0]):
            on_prepared = mc.rows(detect(p))
            assert on_prepared != mc.rows(detect(f))                      # ... the result differs from the frame's as it is ...
            assert on_prepared != mc.rows(detect(g))                      # ... and from the resized frame's without equalization
            found += len(on_prepared) > 0
    assert found == 6                                                     # not empty, all three frames, both profiles


def test_the_mixed_frames_at_half_size(oracle, cascades):
    c, a = cascades(pc.CASC)
    prepared = pc.mixed_prepared(oracle, True)
    assert [p.shape for p in prepared] == [(pc.cv_round(h * 0.5), pc.cv_round(w * 0.5)) for w, h in mc.SIZES]
    n = [len(oracle.detect_opencvlike(a, p)[0]) for p in prepared]
    was = [len(r) for r, _ in mc.oracle_cv(oracle, pc.CASC, a)]
    assert sum(1 for x in n if x > 0) >= 3 and n != was
