"""vj_extract_affine on the device: the bytes of Environment.extract_affine, downloaded, against the numpy
restatement of the definition (tests/affine_cases.py) with np.array_equal.  The smallest shapes at which the kernel can still go
wrong: 37 x 29 sources, output rows of every length mod 4, a partial last row block and a second one, matrices whose positions are
ties of the rounding, fractional and clamped taps, every flag, every kind of source; then every face of the two-cascade call cut
aligned in one call, in slices and into a caller's tensor; the trivial and the error cases.  The premises (the restatement agrees
with three independent computations; the tie family tells the roundings apart; the rotation case has fractions and clamped taps;
the end-to-end frames yield the stated faces) are checked on the CPU in tests/test_affine_cpu.py."""
import ctypes as C
import math

import numpy as np
import pytest

import affine_cases as ac
import extract_cases as ec
import mixed_cases as mc
import prep_cases as pc
from cases import tunables
from clfacedetection_amd import AFFINE_DTYPE, VJ_EXTRACT_GRAY, AffineParams, VjError, align_transforms
from clfacedetection_amd.api import _Image
from test_gpu_mixed import _device_frame, _strided_view

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
W, H = ac.W, ac.H


def check(env, oracle, items, sources, rows, size, **kw):
    """One extract_affine() call against the restatement of every region; returns the downloaded result."""
    got = env.extract_affine(items, rows, size, color=kw.pop("color", False), **kw).cpu().numpy()
    want = ac.restate(oracle, sources, rows, size, **kw)
    assert got.shape == want.shape, (got.shape, want.shape, size, kw)
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), (k, ac.as_rows(rows)[k].tolist(), size, kw, int((got[k] != want[k]).sum()))
    return got


# ------------------------------------------------------------------------------------------------- 1. the independent cross-checks
def test_identity_translation_and_quarter_turn(env, oracle):
    for src in ac.sources(1):
        got = check(env, oracle, [src], [src], ac.rows_for(0, [ac.identity()]), (W, H))
        assert np.array_equal(got[0].reshape(src.shape), src)
        boxes = [(3, 4, 10, 10), (-5, 8, 10, 10), (30, 8, 10, 10), (8, -5, 10, 10), (8, 25, 10, 10), (-3, -3, 10, 10), (30, 22, 10, 10),
                 (100, 100, 10, 10), (-40, 3, 10, 10)]
        got = check(env, oracle, [src], [src], ac.rows_for(0, [ac.translation(x, y) for x, y, _, _ in boxes]), (10, 10))
        for g, (x, y, w, h) in zip(got, boxes):
            assert np.array_equal(g.reshape((h, w) + src.shape[2:]), ec.padded_crop(src, x, y, w, h)), (x, y)
        for x0, y0, ow, oh in [(5, 3, 12, 9), (0, 0, H, W), (-4, -2, 10, 10)]:
            got = check(env, oracle, [src], [src], ac.rows_for(0, [ac.quarter_turn(x0, y0, ow)]), (ow, oh))
            crop = ec.padded_crop(src, x0, y0, oh, ow)
            want = crop[::-1].swapaxes(0, 1)                                # out[y][x] = crop[ow - 1 - x][y]
            assert np.array_equal(got[0].reshape(want.shape), want), (x0, y0)


# ------------------------------------------------------------------------------------------------------------ 2. the arithmetic
def test_the_tie_family(env, oracle):
    for src in ac.sources(2):
        check(env, oracle, [src], [src], ac.rows_for(0, ac.tie_family()), ac.TIE_SIZE)
    bgr = ac.sources(2)[1]
    up = ac.restate(oracle, [bgr], ac.rows_for(0, ac.tie_family()), ac.TIE_SIZE, rnd=ac.half_up)
    got = env.extract_affine([bgr], ac.rows_for(0, ac.tie_family()), ac.TIE_SIZE).cpu().numpy()
    assert not np.array_equal(got, up)                                      # (the premise again, against the device's bytes)


def test_rotation_mirror_shear_and_scalings(env, oracle):
    ms = [ac.ROT, ac.mirrored(ac.ROT, ac.ROT_SIZE[0]), ac.SHEAR, ac.DOWN5, ac.UP4, ac.rotation(-75.0, 0.7, (10.0, 20.0), ac.ROT_SIZE),
          ac.rotation(180.0, 1.0, (18.0, 14.0), ac.ROT_SIZE), ac.rotation(45.0, 2.5, (18.0, 14.0), ac.ROT_SIZE)]
    for src in ac.sources(3):
        for size in (ac.ROT_SIZE, (8, 6), (40, 32)):
            check(env, oracle, [src], [src], ac.rows_for(0, ms), size)
        check(env, oracle, [src], [src], ac.rows_for(0, [ac.rotation(15.0, 1.0, ((W - 1) / 2, (H - 1) / 2), (W, H))]), (W, H))   # a whole frame turned
    bgr = ac.sources(3)[1]
    no_offset = ac.restate(oracle, [bgr], ac.rows_for(0, [ac.ROT]), ac.ROT_SIZE, offset=0)
    assert not np.array_equal(env.extract_affine([bgr], ac.rows_for(0, [ac.ROT]), ac.ROT_SIZE).cpu().numpy(), no_offset)


def test_regions_over_sides_and_corners_and_outside(env, oracle):
    keep = []
    for src in ac.sources(4):
        for size in [(12, 10), (5, 5), (7, 9)]:
            check(env, oracle, [src], [src], ac.rows_for(0, ac.edge_matrices()), size)
        d, t = _device_frame(src, 0, 0)                                     # the buffer ends with the frame's last row
        keep.append(t)
        check(env, oracle, [d], [src], ac.rows_for(0, ac.edge_matrices()), (12, 10))
        d, t = _device_frame(src, 3, 0)
        keep.append(t)
        check(env, oracle, [d], [src], ac.rows_for(0, ac.edge_matrices()), (12, 10), planar=True)
    # at the limit: positions 2^19 pixels away, on every side
    L, s = 2.0 ** 19, 2.0 ** 15
    far = [[s, 0.0, -L, 0.0, 1.0, 3.0], [1.0, 0.0, 5.0, -s, 0.0, L], [-s, 0.0, L, s, 0.0, -L], [1.0, 1.0, L - 16, 1.0, -1.0, -L + 16]]
    src = ac.sources(4)[1]
    check(env, oracle, [src], [src], ac.rows_for(0, far), (17, 17))


# ---------------------------------------------------------------------------------------------------------------- 3. output shapes
@pytest.mark.parametrize("h", [1, 2, 5, 17])
def test_output_sizes(env, oracle, h):
    """Widths around 4 bytes, a wave and a block of slots; heights up to a partial last row block (5), a second block (17); with
    three channels the rows are 1, 2, 3 bytes mod 4 long."""
    ms = [ac.ROT, ac.SHEAR, ac.translation(-2, 3), ac.UP4]
    for src in ac.sources(10 + h):
        for w in list(range(1, 10)) + [21, 63, 64, 65, 255, 256, 257]:
            check(env, oracle, [src], [src], ac.rows_for(0, ms), (w, h))
    src = ac.sources(10 + h)[1]
    assert {(w * 3) % 4 for w in (1, 2, 3)} == {1, 2, 3}
    for w in (5, 21, 85, 86):
        check(env, oracle, [src], [src], ac.rows_for(0, ms), (w, h), planar=True)
        check(env, oracle, [src], [src], ac.rows_for(0, ms), (w, h), gray=True)


# ------------------------------------------------------------------------------------------------------------ 4. flags and sources
def test_gray_and_planar(env, oracle):
    gray, bgr, bgra = ac.sources(20)
    ms = [ac.ROT, ac.SHEAR, ac.DOWN5, ac.translation(-2, 5), ac.identity()]
    rows = np.concatenate([ac.rows_for(f, ms) for f in (0, 1, 2)])
    for size in [(8, 6), (10, 9), (33, 7)]:
        check(env, oracle, [gray, bgr, bgra], [gray, bgr, bgra], rows, size, gray=True)          # mixed channel counts: gray only
        check(env, oracle, [gray, bgr, bgra], [gray, bgr, bgra], rows, size, gray=True, planar=True)
        for src in (bgr, bgra):
            a = check(env, oracle, [src], [src], ac.rows_for(0, ms), size)
            b = check(env, oracle, [src], [src], ac.rows_for(0, ms), size, planar=True)
            assert np.array_equal(b, a.transpose(0, 3, 1, 2))                                     # planar is the interleaved result permuted
            g = check(env, oracle, [src], [src], ac.rows_for(0, ms), size, gray=True)
            assert g.shape == (len(ms), size[1], size[0], 1)
    with pytest.raises(VjError) as ei:
        env.extract_affine([gray, bgr], rows[:10], (8, 6))
    assert ei.value.code == VJ_ERR_ARG and "channels" in str(ei.value)
    # a structured array is the same call
    st = np.zeros(len(ms), AFFINE_DTYPE)
    st["m"] = ms
    assert np.array_equal(env.extract_affine([bgr], st, (8, 6)).cpu().numpy(), ac.restate(oracle, [bgr], ac.rows_for(0, ms), (8, 6)))


def test_strided_host_views_and_device_frames_at_every_address(env, oracle):
    ms = [ac.ROT, ac.SHEAR, ac.DOWN5, ac.translation(-2, 5), ac.identity(), ac.UP4]
    keep = []
    for i, src in enumerate(ac.sources(21)):
        ch = 1 if src.ndim == 2 else src.shape[2]
        v, base = _strided_view(src, 7 if (W * ch) % 2 == 0 else 8)
        assert v.strides[0] % 2 == 1
        for size in [(10, 8), (W, H)]:
            check(env, oracle, v, [src], ac.rows_for(0, ms), size, color=ch > 1)
        for off, pad in [(0, 0), (1, 3), (2, 1), (3, 0)]:
            d, t = _device_frame(src, off, pad)
            assert d.ptr % 4 == off
            keep.append(t)
            check(env, oracle, d, [src], ac.rows_for(0, ms), (10, 8))
            check(env, oracle, [v, d], [src, src], np.concatenate([ac.rows_for(0, ms), ac.rows_for(1, ms)]), (7, 5))


def test_the_eleven_mixed_frames_in_one_call_and_in_slices(env, oracle):
    import torch
    frames = mc.frames()
    rows = []
    for i, (w, h) in enumerate(mc.SIZES):
        rows += [[i] + ac.rotation(20.0, 1.5, (w / 2, h / 2), (24, 24)), [i] + ac.from_rect(-3, h - 10, 24, 24, (24, 24)), [i] + ac.from_rect(0, 0, w, h, (24, 24)),
                 [i] + ac.rotation(-40.0, 0.8, (w / 3, 1.0), (24, 24))]
    rows = np.array(rows, np.float64)
    want = check(env, oracle, frames, frames, rows, (24, 24))
    check(env, oracle, frames, frames, rows, (24, 24), planar=True)
    with tunables(env, ("max_subbatch", "3")):                                                    # four slices
        assert np.array_equal(check(env, oracle, frames, frames, rows, (24, 24)), want)
    with tunables(env, ("max_subbatch", "1")):
        assert np.array_equal(env.extract_affine(frames, rows[::-1], (24, 24)).cpu().numpy(), want[::-1])
    keep, items = [], []
    for i, f in enumerate(frames):                                                                # host and device frames in one call
        if i % 2:
            d, t = _device_frame(f, i % 4, i % 3)
            keep.append(t)
            items.append(d)
        else:
            items.append(f)
    check(env, oracle, items, frames, rows, (24, 24))
    out = torch.zeros(want.size + 1, dtype=torch.uint8, device="cuda")[1:]                        # a caller's tensor, at an odd address
    assert out.data_ptr() % 2 == 1
    for _ in range(2):
        res = env.extract_affine(frames, rows, (24, 24), out=out)
        assert res.data_ptr() == out.data_ptr() and np.array_equal(res.cpu().numpy(), want)
    for bad in (out[:-1], torch.zeros(want.size, dtype=torch.uint8), torch.zeros(want.size, dtype=torch.int8, device="cuda"),
                torch.zeros(2 * want.size, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError):
            env.extract_affine(frames, rows, (24, 24), out=bad)


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
def test_faces_of_the_two_cascade_call_cut_aligned(env, oracle, cascades):
    """preprocess -> detect_opencv_chain(frontalface_alt, eye) -> align_transforms(scale = 1.8) -> extract_affine, every face cut from
    the 432 x 324 colour sources to 32 x 32 in one call; then the hand-made paired case, so both branches run on the device."""
    import torch
    c1, _ = cascades(pc.CASC)
    c2, _ = cascades("eye")
    bgr = ec.e2e_bgr()
    small = env.preprocess(bgr, size=pc.E2E_SIZE, equalize=True, color=True)[0]
    faces, eyes = env.detect_opencv_chain(c1, c2, small, min_neighbors=3)
    affines, paired = align_transforms(faces, eyes, ac.E2E_SIZE, scale=ec.MANY_SCALE)
    print(f"end to end: {len(faces.rects)} faces, {len(eyes.rects)} eye candidates, {int(paired.sum())} faces paired")
    assert len(affines) == ac.E2E_FACES and int(paired.sum()) == ac.E2E_PAIRED
    rows, want_paired = ac.align(faces.rects, eyes.rects, ac.E2E_SIZE, scale=ec.MANY_SCALE)
    assert paired.tolist() == want_paired and np.array_equal(ac.as_rows(affines).view(np.uint64), rows.view(np.uint64))
    got = env.extract_affine(bgr, affines, ac.E2E_SIZE, color=True)
    assert got.shape == (len(affines), 32, 32, 3) and got.dtype == torch.uint8 and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), ac.restate(oracle, list(bgr), rows, ac.E2E_SIZE))
    assert env.extract_affine_timing() > 0
    # the hand-made case: faces 0 and 2 by their eyes (turned), face 1 by its box
    hf, he = ac.rects(ac.HAND_FACES), ac.rects(ac.HAND_EYES)
    affines, paired = align_transforms(hf, he, ac.E2E_SIZE, scale=ec.MANY_SCALE)
    assert paired.tolist() == [True, False, True] and affines["m"][0][1] != 0.0 and affines["m"][1][1] == 0.0
    for kw in (dict(), dict(gray=True), dict(planar=True)):
        got = env.extract_affine(bgr, affines, ac.E2E_SIZE, color=True, **kw).cpu().numpy()
        assert np.array_equal(got, ac.restate(oracle, list(bgr), affines, ac.E2E_SIZE, **kw)), kw


# ------------------------------------------------------------------------------------------------------ 6. trivial and error cases
def test_no_affine(env):
    src = ac.sources(30)[1]
    assert env.extract_affine([src], np.zeros((0, 7)), (24, 24)).shape == (0, 24, 24, 3)
    assert env.extract_affine([src], np.zeros(0, AFFINE_DTYPE), (24, 24), planar=True, gray=True).shape == (0, 1, 24, 24)


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
    good = [(0, 0) + tuple(ac.rotation(30.0, 1.3, (40.0, 40.0), (24, 24))), (1, 0) + tuple(ac.translation(-3, 2))]
    f = lib.vj_extract_affine

    def call(images=ok, n=None, rows=good, nr=None, p=True, d=dst.data_ptr(), nbytes=dst.numel(), e=env._h, **kw):
        q = AffineParams()
        lib.vj_affine_default(C.byref(q))
        q.out_w, q.out_h = 24, 24
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images) if images is not None else None
        r = None
        if rows is not None:
            r = np.zeros(len(rows), AFFINE_DTYPE)
            for i, row in enumerate(rows):
                r[i] = (row[0], row[1], row[2:])
        rc = f(e, arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if r is not None else None,
               (len(r) if r is not None else 2) if nr is None else nr, C.byref(q) if p else None, C.c_void_p(d), nbytes)
        err = lib.vj_last_error().decode()
        after = env.detect(c, plain)                                              # every error is followed by a plain detect
        assert np.array_equal(after.rects, base.rects)
        return rc, err

    assert call()[0] == 0
    need = 2 * 24 * 24
    # null arguments, negative counts
    for kw in (dict(e=None), dict(images=None), dict(rows=None), dict(p=False), dict(d=None), dict(n=-1), dict(nr=-1)):
        assert call(**kw)[0] == VJ_ERR_ARG, kw
    # bad frames
    for bad in (_Image(None, 8, 4, 8, 1, 1), _Image(src.data_ptr(), 0, 4, 8, 1, 1), _Image(src.data_ptr(), 8, 4, 7, 1, 1), _Image(src.data_ptr(), 8, 4, 16, 1, 2)):
        rc, err = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err
    # bad affines: the frame index, reserved, a non-finite entry
    ident = tuple(ac.identity())
    for bad, word in (((2, 0) + ident, "frame"), ((-1, 0) + ident, "frame"), ((0, 1) + ident, "reserved"),
                      ((0, 0, math.nan) + ident[1:], "m[0]"), ((0, 0) + ident[:5] + (math.inf,), "m[5]"), ((0, 0) + ident[:3] + (-math.inf,) + ident[4:], "m[3]")):
        rc, err = call(rows=good + [bad])
        assert rc == VJ_ERR_ARG and "affine 2" in err and word in err, bad
    # the fields of vj_affine_params
    for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=-1), "out_h"), (dict(flags=4), "flags"), (dict(reserved=7), "reserved")]:
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    # mixed channel counts without VJ_EXTRACT_GRAY
    bgr = np.zeros((20, 20, 3), np.uint8)
    rc, err = call(images=ok + [_Image(bgr.ctypes.data, 20, 20, 60, 0, 3)], rows=good + [(2, 0) + ident])
    assert rc == VJ_ERR_ARG and "affine 2" in err and "channels" in err
    assert call(images=ok + [_Image(bgr.ctypes.data, 20, 20, 60, 0, 3)], rows=good + [(2, 0) + ident], flags=VJ_EXTRACT_GRAY)[0] == 0
    # the limits
    big = 2.0 ** 19
    for kw, rows, word in [(dict(out_w=65536), good, "65535"), (dict(), good + [(0, 0, big / 23 * 1.001, 0.0, 0.0, 0.0, 1.0, 0.0)], "m[0]"),
                           (dict(), good + [(0, 0, 1.0, 0.0, 0.0, -big / 23 * 1.001, 1.0, 0.0)], "m[3]"),
                           (dict(), good + [(0, 0, 1.0, 0.0, big + 1, 0.0, 1.0, 0.0)], "m[2]"), (dict(), good + [(0, 0, 1.0, 0.0, 0.0, 0.0, 1.0, -big - 1)], "m[5]"),
                           (dict(), good + [(0, 0, 1.0, 1.0, big - 22, 0.0, 1.0, 0.0)], "m[1]"), (dict(), good + [(0, 0, 1.0, 0.0, 0.0, 0.0, -1.0, -big + 22)], "m[4]")]:
        rc, err = call(rows=rows, **kw)
        assert rc == VJ_ERR_LIMIT and word in err, (kw, rows[-1], err)
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
    # zero affines
    assert call(rows=[])[0] == 0
    assert f(env._h, None, 0, None, 0, C.byref(AffineParams(4, 4, 0, 0)), None, 0) == 0
    # and the environment still cuts
    fr = [mc.frames()[1], mc.frames()[3]]
    check(env, oracle, fr, fr, np.array([(g[0],) + g[2:] for g in good], np.float64), (24, 24))
