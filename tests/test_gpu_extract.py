"""vj_extract on the device: the bytes of Environment.extract, downloaded, against the composition of the existing
restatements — the crop padded by clamping, then resize_linear per channel, bgr2gray first for gray=True (tests/extract_cases.py) —
with np.array_equal.  The smallest shapes at which the kernel can still go wrong: 37 x 29 sources, output rows of every length
mod 4, the three modes inside and across the frame's edges, every flag, every kind of source; then every raw candidate of the
detector cut in one call, in slices and into a caller's tensor; the trivial and the error cases.  The premises (the detector finds
candidates there; the crop-edge case tells the two clamps apart) are checked on the CPU in tests/test_extract_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import mixed_cases as mc
import prep_cases as pc
from cases import tunables
from clfacedetection_amd import VJ_EXTRACT_GRAY, VJ_EXTRACT_PLANAR, ExtractParams, VjError
from clfacedetection_amd.api import RECT_DTYPE, _Image
from test_gpu_mixed import _color, _device_frame, _strided_view
from test_gpu_prep import download

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
W, H = 37, 29


def check(env, oracle, items, sources, rects, size, **kw):
    """One extract() call against the restatement of every region; returns the downloaded result."""
    got = env.extract(items, rects, size, color=kw.pop("color", False), **kw).cpu().numpy()
    want = ec.restate(oracle, sources, rects, size, **kw)
    assert got.shape == want.shape, (got.shape, want.shape, size, kw)
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (k, tuple(ec.as_rows(rects)[k]), size, kw)
    return got


def sources(seed):
    """Random 37 x 29 frames: gray, BGR, BGRA."""
    rng = np.random.default_rng(seed)
    return [_color(rng, H, W, ch) for ch in (1, 3, 4)]


# ----------------------------------------------------------------------------------------------------- 1. crop and output sizes
@pytest.mark.parametrize("h", [1, 2, 5])
def test_crop_and_output_sizes(env, oracle, h):
    """Crops of 1 x 1, 2 x 3, 5 x 5 and 20 x 17 to widths around 4 bytes, a wave and a block, up-scaling included; with three
    channels the rows are 1, 2, 3 bytes mod 4 long."""
    rects = [(0, 3, 4, 1, 1), (0, 5, 5, 2, 3), (0, 4, 7, 5, 5), (0, 8, 6, 20, 17)]
    for src in sources(h):
        for w in list(range(1, 10)) + [21, 63, 64, 65, 255, 256, 257]:
            check(env, oracle, [src], [src], rects, (w, h))
    src = sources(h)[1]
    assert {(w * 3) % 4 for w in (1, 2, 3)} == {1, 2, 3}
    for w in (5, 21, 85, 86):
        check(env, oracle, [src], [src], rects, (w, h), planar=True)
        check(env, oracle, [src], [src], rects, (w, h), gray=True)


# --------------------------------------------------------------------------------------------------------------- 2. the three modes
@pytest.mark.parametrize("where", ["inside_even", "inside_odd", "left_top", "right_bottom"])
def test_mean_bilinear_and_copy(env, oracle, where):
    """The crop exactly twice the output (the 2 x 2 mean), twice on one axis only (bilinear) and equal to it (the copy): wholly
    inside the frame at even and odd x — the wide loads aligned and not — and across a frame edge (the clamped byte path), from
    host frames (staged at a multiple of 4) and from device frames at addresses 0 .. 3 mod 4.  Both paths give the same bytes."""
    x, y = {"inside_even": (4, 2), "inside_odd": (5, 3), "left_top": (-3, -2), "right_bottom": (30, 25)}[where]
    ow, oh = 8, 6
    rects = [(0, x, y, 2 * ow, 2 * oh), (0, x, y, 2 * ow, oh), (0, x, y, ow, 2 * oh), (0, x, y, ow, oh),
             (0, x + 1, y, 2 * ow, 2 * oh), (0, x + 2, y + 1, ow, oh), (0, x + 3, y, ow, oh)]
    keep = []
    for src in sources(7):
        for kw in (dict(), dict(planar=True), dict(gray=True)):
            check(env, oracle, [src], [src], rects, (ow, oh), **kw)
        for off, pad in [(0, 0), (1, 3), (2, 1), (3, 0), (4, 4)]:
            d, t = _device_frame(src, off, pad)
            keep.append(t)
            check(env, oracle, [d], [src], rects, (ow, oh))
            check(env, oracle, [d], [src], rects, (ow, oh), gray=True, planar=True)
    # a larger mean and copy: more than one block of rows and of slots (rows of 300 bytes, 40 rows)
    rng = np.random.default_rng(8)
    for ch in (1, 3):
        big = _color(rng, 90, 620, ch)
        out = (300 // ch, 40)
        bx, by = (x, y) if where.startswith("inside") else (x * 10, y * 2)
        r = [(0, bx, by, 2 * out[0], 2 * out[1]), (0, bx, by, out[0], out[1]), (0, bx + 1, by + 1, 2 * out[0], 2 * out[1])]
        check(env, oracle, [big], [big], r, out)
        d, t = _device_frame(big, 0, 0)
        keep.append(t)
        check(env, oracle, [d], [big], r, out)


# ----------------------------------------------------------------------------------------------------------------- 3. crop edges
def test_taps_clamp_at_the_crop_not_at_the_frame(env, oracle):
    for ch in (1, 3, 4):
        f = ec.edge_frame(ch)
        got = check(env, oracle, [f], [f], [ec.EDGE_RECT], ec.EDGE_SIZE)
        assert int(got.max()) <= 60                                       # no pixel from outside the crop (they are >= 200) leaks in
        got = check(env, oracle, [f], [f], [ec.EDGE_RECT], (10, 17))      # down-scaling by 2 on one axis: bilinear
        assert int(got.max()) <= 60


# ---------------------------------------------------------------------------------------------------------------- 4. frame edges
def test_regions_over_sides_and_corners_and_outside(env, oracle):
    rects = [(0, -5, 8, 10, 10), (0, 30, 8, 10, 10), (0, 8, -5, 10, 10), (0, 8, 25, 10, 10),               # each side
             (0, -3, -3, 10, 10), (0, 30, -3, 10, 10), (0, -3, 22, 10, 10), (0, 30, 22, 10, 10),           # each corner
             (0, 100, 100, 6, 6), (0, -40, 3, 6, 6), (0, 5, -30, 6, 6),                                    # wholly outside
             (0, 0, 0, W, H), (0, -4, -4, W + 8, H + 8)]                                                   # the frame, and more
    keep = []
    for src in sources(9):
        for size in [(10, 10), (5, 5), (7, 9), (24, 24)]:
            check(env, oracle, [src], [src], rects, size)
        check(env, oracle, [src], [src], [(0, 0, 0, W, H)], (W, H), margin=0.25)      # the whole frame plus a margin, as a copy of
        check(env, oracle, [src], [src], [(0, 0, 0, W, H)], (W + 18, H + 14), margin=0.25)   # its size and as a copy of the crop's
        check(env, oracle, [src], [src], [(0, 0, 0, W, H)], (20, 20), margin=1.0)
        d, t = _device_frame(src, 0, 0)                                               # the buffer ends with the frame's last row
        keep.append(t)
        for size in [(10, 10), (5, 5), (W, H), (24, 24)]:
            check(env, oracle, [d], [src], rects, size)
        d, t = _device_frame(src, 3, 0)
        keep.append(t)
        check(env, oracle, [d], [src], rects, (5, 5))
        check(env, oracle, [d], [src], rects, (10, 10), planar=True)


# ---------------------------------------------------------------------------------------------------------------------- 5. flags
def test_gray_planar_and_the_whole_frame_against_preprocess(env, oracle):
    gray, bgr, bgra = sources(10)
    rects = [(0, 2, 3, 20, 17), (1, -2, 5, 12, 9), (2, 20, 15, 30, 30), (1, 0, 0, W, H), (0, 6, 6, 16, 12)]
    for size in [(8, 6), (10, 9), (33, 7)]:
        check(env, oracle, [gray, bgr, bgra], [gray, bgr, bgra], rects, size, gray=True)          # mixed channel counts: gray only
        check(env, oracle, [gray, bgr, bgra], [gray, bgr, bgra], rects, size, gray=True, planar=True)
        for src in (bgr, bgra):
            r = [(0,) + q[1:] for q in rects]
            a = check(env, oracle, [src], [src], r, size)
            b = check(env, oracle, [src], [src], r, size, planar=True)
            assert np.array_equal(b, a.transpose(0, 3, 1, 2))                                     # planar is the interleaved result permuted
            g = check(env, oracle, [src], [src], r, size, gray=True)
            assert g.shape == (len(r), size[1], size[0], 1)
    with pytest.raises(VjError) as ei:
        env.extract([gray, bgr], rects[:2], (8, 6))
    assert ei.value.code == VJ_ERR_ARG and "channels" in str(ei.value)
    # a whole-frame region with gray=True and no margin is preprocess() without equalization, byte for byte
    for src in (gray, bgr, bgra):
        for size in [(18, 14), (W, H), (40, 33), (W // 2, H // 2)]:
            got = env.extract([src], [(0, 0, 0, W, H)], size, gray=True).cpu().numpy()[0, :, :, 0]
            img, w = download(env.preprocess([src], size=size))[0]
            assert np.array_equal(got, img[:, :w]), (src.shape, size)
    even = _color(np.random.default_rng(3), 28, 36, 3)                                            # exactly half: the 2 x 2 mean
    got = env.extract([even], [(0, 0, 0, 36, 28)], (18, 14), gray=True).cpu().numpy()[0, :, :, 0]
    img, w = download(env.preprocess([even], size=(18, 14)))[0]
    assert np.array_equal(got, img[:, :w])


# -------------------------------------------------------------------------------------------------------------------- 6. sources
def test_strided_host_views_and_device_frames_at_odd_addresses(env, oracle):
    rects = [(0, 2, 3, 20, 17), (0, -2, 5, 12, 9), (0, 20, 15, 30, 30), (0, 0, 0, W, H), (0, 3, 3, 10, 8), (0, 4, 4, 20, 16)]
    keep = []
    for i, src in enumerate(sources(11)):
        ch = 1 if src.ndim == 2 else src.shape[2]
        v, base = _strided_view(src, 7 if (W * ch) % 2 == 0 else 8)
        assert v.strides[0] % 2 == 1
        d, t = _device_frame(src, 1 + 2 * (i % 2), 0 if (W * ch) % 2 else 3)
        assert d.ptr % 2 == 1 and d.stride % 2 == 1
        keep.append(t)
        for size in [(10, 8), (7, 5), (W, H)]:
            check(env, oracle, v, [src], rects, size, color=ch > 1)
            check(env, oracle, [v, d], [src, src], rects + [(1,) + q[1:] for q in rects], size)
            check(env, oracle, d, [src], rects, size)


def test_the_eleven_mixed_frames_in_one_call(env, oracle):
    frames = mc.frames()
    rects = []
    for i, (w, h) in enumerate(mc.SIZES):
        rects += [(i, w // 4, h // 4, w // 2, h // 2), (i, -3, h - 10, 24, 24), (i, 0, 0, w, h), (i, w // 3, 1, 48, 48)]
    check(env, oracle, frames, frames, rects, (24, 24))
    check(env, oracle, frames, frames, rects, (24, 24), planar=True, margin=0.1)
    with tunables(env, ("max_subbatch", "3")):                                                    # four slices
        check(env, oracle, frames, frames, rects, (12, 12))
    keep, items = [], []
    for i, f in enumerate(frames):                                                                # host and device frames in one call
        if i % 2:
            d, t = _device_frame(f, i % 4, i % 3)
            keep.append(t)
            items.append(d)
        else:
            items.append(f)
    check(env, oracle, items, frames, rects, (24, 24))


# -------------------------------------------------------------------------------------------------------------------- 7. mapping
def test_scale_with_ties_and_a_margin(env, oracle):
    src = sources(12)[1]
    rects = [(0, 5, 7, 5, 7), (0, 7, 5, 7, 5), (0, 1, 3, 1, 3), (0, 9, 11, 13, 15), (0, 30, 20, 40, 30), (0, -9, -7, 25, 25)]
    for scale, margin in [((0.5, 0.5), 0.0), ((0.5, 0.5), 0.25), ((1.0, 1.0), 0.25), ((1.5, 2.5), 0.25), ((0.0, 0.0), 0.0)]:
        mapped, ch, nbytes = env.extract_layout([src], rects, (9, 9), scale=scale, margin=margin)
        assert [tuple(r) for r in mapped.tolist()] == [ec.map_region(r, scale, margin) for r in rects] and ch == 3 and nbytes == len(rects) * 243
        got = check(env, oracle, [src], [src], rects, (9, 9), scale=scale, margin=margin)
        # ... and the regions extract_layout reports, cut as they are, give the same bytes
        assert np.array_equal(env.extract([src], mapped, (9, 9)).cpu().numpy(), got)
    assert ec.map_region(rects[0], (0.5, 0.5)) == (0, 2, 4, 2, 4) and ec.map_region(rects[1], (0.5, 0.5)) == (0, 4, 2, 4, 2)


# --------------------------------------------------------------------------------------------------------------- 8. many regions
def test_every_raw_candidate_of_the_detector(env, oracle, cascades):
    """detect_opencv on the prepared 240 x 180 frames, every raw candidate cut from the 432 x 324 colour sources (factor 1.8) to
    24 x 24 in one call; the same list in slices; the same into a caller's tensor, twice (the environment's buffers are reused)."""
    import torch
    c, a = cascades(pc.CASC)
    bgr = ec.e2e_bgr()
    small = env.preprocess(bgr, size=pc.E2E_SIZE, equalize=True, color=True)[0]
    rects = env.detect_opencv(c, small).rects
    per_frame = [int((rects["frame"] == i).sum()) for i in range(3)]
    print("raw candidates per frame:", per_frame)
    assert rects.dtype == RECT_DTYPE and all(n > 0 for n in per_frame) and len(rects) >= 100
    want = pc.once("extract_many", lambda: ec.restate(oracle, list(bgr), rects, ec.MANY_SIZE, scale=ec.MANY_SCALE))
    got = env.extract(bgr, rects, ec.MANY_SIZE, scale=ec.MANY_SCALE, color=True)
    assert got.shape == (len(rects), 24, 24, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert env.extract_timing() > 0
    with tunables(env, ("max_subbatch", "1")):                                                    # one slice per frame
        assert np.array_equal(env.extract(bgr, rects, ec.MANY_SIZE, scale=ec.MANY_SCALE, color=True).cpu().numpy(), want)
    with tunables(env, ("max_subbatch", "2")):
        assert np.array_equal(env.extract(list(bgr), rects[::-1], ec.MANY_SIZE, scale=ec.MANY_SCALE).cpu().numpy(), want[::-1])
    out = torch.zeros(want.size + 1, dtype=torch.uint8, device="cuda")[1:]                        # a caller's tensor, at an odd address
    assert out.data_ptr() % 2 == 1
    for _ in range(2):
        res = env.extract(bgr, rects, ec.MANY_SIZE, scale=ec.MANY_SCALE, color=True, out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(res.cpu().numpy(), want)
    res = env.extract(bgr, rects, ec.MANY_SIZE, scale=ec.MANY_SCALE, color=True, planar=True, out=out)
    assert res.shape == (len(rects), 3, 24, 24) and np.array_equal(res.cpu().numpy(), want.transpose(0, 3, 1, 2))
    for bad in (out[:-1], torch.zeros(want.size, dtype=torch.uint8), torch.zeros(want.size, dtype=torch.int8, device="cuda"),
                torch.zeros(2 * want.size, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError):
            env.extract(bgr, rects, ec.MANY_SIZE, scale=ec.MANY_SCALE, color=True, out=bad)


# ------------------------------------------------------------------------------------------------------ 9. trivial and error cases
def test_no_region(env):
    src = sources(13)[1]
    got = env.extract([src], np.zeros((0, 5), np.int32), (24, 24))
    assert got.shape == (0, 24, 24, 3)
    assert env.extract([src], np.zeros(0, RECT_DTYPE), (24, 24), planar=True, gray=True).shape == (0, 1, 24, 24)


def test_argument_errors_leave_the_environment_usable(env, lib, oracle, cascades):
    import torch
    c, a = cascades(pc.CASC)
    plain = mc.frames()[0]
    base = env.detect(c, plain)
    assert len(base.rects) >= 10
    src = torch.from_numpy(np.array(mc.frames()[1])).cuda()
    h, w = src.shape
    dst = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    host = np.ascontiguousarray(mc.frames()[3])
    ok = [_Image(src.data_ptr(), w, h, w, 1, 1), _Image(host.ctypes.data, host.shape[1], host.shape[0], host.strides[0], 0, 1)]
    good = [(0, 5, 5, 40, 40), (1, -3, 2, 30, 20)]
    f = lib.vj_extract

    def call(images=ok, n=None, rects=good, nr=None, p=True, d=dst.data_ptr(), nbytes=dst.numel(), e=env._h, **kw):
        q = ExtractParams()
        lib.vj_extract_default(C.byref(q))
        q.out_w, q.out_h = 24, 24
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images) if images is not None else None
        r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 5)) if rects is not None else None
        rc = f(e, arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if r is not None else None,
               (len(r) if r is not None else 2) if nr is None else nr, C.byref(q) if p else None, C.c_void_p(d), nbytes)
        err = lib.vj_last_error().decode()
        after = env.detect(c, plain)                                              # every error is followed by a plain detect
        assert np.array_equal(after.rects, base.rects)
        return rc, err

    assert call()[0] == 0
    need = 2 * 24 * 24
    # null arguments, negative counts
    for kw in (dict(e=None), dict(images=None), dict(rects=None), dict(p=False), dict(d=None), dict(n=-1), dict(nr=-1)):
        assert call(**kw)[0] == VJ_ERR_ARG, kw
    # bad frames
    for bad in (_Image(None, 8, 4, 8, 1, 1), _Image(src.data_ptr(), 0, 4, 8, 1, 1), _Image(src.data_ptr(), 8, 4, 7, 1, 1), _Image(src.data_ptr(), 8, 4, 16, 1, 2)):
        rc, err = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err
    # bad regions
    for bad in ((2, 0, 0, 4, 4), (-1, 0, 0, 4, 4), (0, 0, 0, 0, 4), (0, 0, 0, 4, 0), (1, 0, 0, -3, 4)):
        rc, err = call(rects=good + [bad])
        assert rc == VJ_ERR_ARG and "region 2" in err
    # the fields of vj_extract_params
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=-1), "out_h"), (dict(sx=-1.0), "sx"), (dict(sy=float("nan")), "sy"),
                     (dict(sx=float("inf")), "sx"), (dict(margin=-0.5), "margin"), (dict(margin=float("inf")), "margin"),
                     (dict(flags=4), "flags"), (dict(reserved=7), "reserved")]:
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    # mixed channel counts without VJ_EXTRACT_GRAY
    bgr = np.zeros((20, 20, 3), np.uint8)
    rc, err = call(images=ok + [_Image(bgr.ctypes.data, 20, 20, 60, 0, 3)], rects=good + [(2, 0, 0, 4, 4)])
    assert rc == VJ_ERR_ARG and "region 2" in err and "channels" in err
    assert call(images=ok + [_Image(bgr.ctypes.data, 20, 20, 60, 0, 3)], rects=good + [(2, 0, 0, 4, 4)], flags=VJ_EXTRACT_GRAY)[0] == 0
    # the limits
    for kw, rects, word in [(dict(out_w=65536), good, "65535"), (dict(), good + [(0, 0, 0, 65536, 4)], "65535"), (dict(margin=1e4), good, "65535"),
                            (dict(), good + [(0, (1 << 24) + 1, 0, 4, 4)], "2^24"), (dict(sy=1e7), good, "2^24")]:
        rc, err = call(rects=rects, **kw)
        assert rc == VJ_ERR_LIMIT and word in err, kw
    # dst_bytes too small, by one byte
    rc, err = call(nbytes=need - 1)
    assert rc == VJ_ERR_ARG and "dst_bytes" in err
    assert call(nbytes=need)[0] == 0
    # a device-resident source that overlaps the destination: its first byte and its last byte
    end = src.data_ptr() + h * w
    for d0 in (src.data_ptr() - need + 1, end - 1):
        rc, err = call(d=d0, nbytes=need)
        assert rc == VJ_ERR_ARG and "frame 0" in err and "overlaps" in err
    assert np.array_equal(src.cpu().numpy(), mc.frames()[1])                      # nothing was written
    # zero regions
    assert call(rects=[])[0] == 0
    assert f(env._h, None, 0, None, 0, C.byref(ExtractParams(4, 4, 1.0, 1.0, 0.0, 0, 0)), None, 0) == 0
    # and the environment still extracts
    fr = [mc.frames()[1], mc.frames()[3]]
    check(env, oracle, fr, fr, good, (24, 24))
