"""vj_extract_yuv / vj_extract_affine_yuv on the device: the downloaded bytes of every call against the restatement of
tests/extract_yuv_cases.py — yuv_cases.decode, then extract_cases.restate or affine_cases.restate — with np.array_equal, on random
full-range frames of 38 x 30 and 66 x 34 in all three layouts; and against code that already ships: extract() / extract_affine() of
yuv_to_bgr() of the same frames give the same tensor.  The premises (the tap-level reading equals the sentence, the wrong readings
differ on these cases, the frames saturate, the sizes straddle the work units) are checked on the CPU in tests/test_extract_yuv_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import affine_cases as ac
import extract_cases as ec
import extract_yuv_cases as eyc
import mixed_cases as mc
import prep_cases as pc
import yuv_cases as yc
from cases import tunables
from clfacedetection_amd import AFFINE_DTYPE, AffineParams, ExtractParams, VjError, YuvFrames, YuvParams, align_transforms
from clfacedetection_amd.api import _YuvImage
from test_gpu_yuv import Planes, first_bad, once

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
LAYOUTS = eyc.LAYOUTS
NAME = yc.LAYOUT_NAMES


# ------------------------------------------------------------------------------------------------------------------- helpers
def frames_of(layout):
    return once(("extract_yuv frames", layout), lambda: eyc.frames(layout))


def decoded_of(layout, alpha, rgb):
    return once(("extract_yuv decoded", layout, alpha, rgb), lambda: eyc.decoded(frames_of(layout), layout, alpha, rgb))


def route_frames(env, items, host_layout, alpha, rgb):
    return env.yuv_to_bgr(items, alpha=alpha, rgb=rgb, layout=host_layout)


def check(env, oracle, items, frames, layouts, rects, size, host_layout="nv12", decoded=None, scale=(1.0, 1.0), margin=0.0, gray=False, planar=False,
          alpha=False, rgb=False):
    """One extract_yuv() call against the restatement, and against extract() of yuv_to_bgr() of the same frames; returns the bytes."""
    got = env.extract_yuv(items, rects, size, scale=scale, margin=margin, gray=gray, planar=planar, alpha=alpha, rgb=rgb, layout=host_layout).cpu().numpy()
    dec = eyc.decoded(frames, layouts, alpha, rgb) if decoded is None else decoded
    want = ec.restate(oracle, dec, rects, size, scale, margin, gray, planar)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (size, dict(gray=gray, planar=planar, alpha=alpha, rgb=rgb), first_bad(got.reshape(-1), want.reshape(-1)))
    via = env.extract(route_frames(env, items, host_layout, alpha, rgb), rects, size, scale=scale, margin=margin, gray=gray, planar=planar).cpu().numpy()
    assert np.array_equal(got, via), "extract(yuv_to_bgr()) differs"
    return got


def check_affine(env, oracle, items, frames, layouts, rows, size, host_layout="nv12", gray=False, planar=False, alpha=False, rgb=False):
    got = env.extract_affine_yuv(items, rows, size, gray=gray, planar=planar, alpha=alpha, rgb=rgb, layout=host_layout).cpu().numpy()
    want = eyc.restate_affine(oracle, frames, layouts, rows, size, gray, planar, alpha, rgb)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (size, dict(gray=gray, planar=planar, alpha=alpha, rgb=rgb), first_bad(got.reshape(-1), want.reshape(-1)))
    via = env.extract_affine(route_frames(env, items, host_layout, alpha, rgb), rows, size, gray=gray, planar=planar).cpu().numpy()
    assert np.array_equal(got, via), "extract_affine(yuv_to_bgr()) differs"
    return got


def both_frames_rects():
    """Crops on both frames: every size, parity, side and corner on the 38 x 30 one, a few on the 66 x 34 one."""
    return eyc.crops(0) + [(1, 9, 7, 20, 17), (1, 57, 25, 20, 17), (1, -3, -2, 5, 5), (1, 0, 0, 66, 34)]


# ------------------------------------------------------------------------------------------------------------------- 1. extract_yuv
@pytest.mark.parametrize("out_h", eyc.OUT_HEIGHTS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_output_width_at_this_height(env, oracle, layout, out_h):
    """Widths 1 .. 9, 21, 63 .. 65 and 255 .. 257: rows shorter than a slot, around a block's 64 slots and beyond them, of three bytes
    a pixel and (planar) of one, beginning at every address mod 4 — crops of 1 x 1, 2 x 3, 5 x 5 and 20 x 17 at odd and even origins,
    over a corner and outside the frame."""
    fr = frames_of(layout)
    rects = [r for r in eyc.crops(0) if (r[1], r[2]) in ((8, 6), (9, 7), (-1, -1), (58, 41), (-50, 3))]
    assert len(rects) == 20
    for i, w in enumerate(eyc.OUT_WIDTHS):
        alpha, planar = i % 3 == 1, i % 4 == 3
        check(env, oracle, fr, fr, layout, rects, (w, out_h), NAME[layout], decoded_of(layout, alpha, False), alpha=alpha, planar=planar)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_mean_the_bilinear_path_and_the_copy_at_every_parity_side_and_corner(env, oracle, layout):
    fr = frames_of(layout)
    for k, (rects, size) in enumerate(eyc.resize_cases()):
        alpha, rgb = k % 2 == 1, k % 3 == 2
        check(env, oracle, fr, fr, layout, rects, size, NAME[layout], decoded_of(layout, alpha, rgb), alpha=alpha, rgb=rgb)
    assert env.extract_yuv_timing() > 0
    # every crop size at every placement, on both frames; wholly outside; the whole frame, and the whole frame plus a margin
    for size in [(5, 5), (10, 10), (33, 17)]:
        check(env, oracle, fr, fr, layout, both_frames_rects(), size, NAME[layout], decoded_of(layout, False, False))
    whole = [(0, 0, 0, 38, 30), (1, 0, 0, 66, 34)]
    check(env, oracle, fr, fr, layout, whole, (38, 30), NAME[layout], margin=0.1)
    check(env, oracle, fr, fr, layout, whole, (19, 15), NAME[layout])
    check(env, oracle, fr, fr, layout, whole, (21, 17), NAME[layout], margin=0.25, scale=(0.5, 0.5))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_flags_and_their_combinations(env, oracle, layout):
    fr = frames_of(layout)
    rects = both_frames_rects()[::3]
    for flags in eyc.FLAG_CASES:
        dec = decoded_of(layout, flags["alpha"], flags["rgb"])
        check(env, oracle, fr, fr, layout, rects, (21, 17), NAME[layout], dec, **flags)
        check(env, oracle, fr, fr, layout, rects, (10, 10), NAME[layout], dec, **flags)      # copies and means among them
        check(env, oracle, fr, fr, layout, rects, (5, 5), NAME[layout], dec, **flags)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_crop_edge_case_with_chroma_that_differs(env, oracle, layout):
    p = eyc.edge_planes(layout)
    got = check(env, oracle, [p], [p], layout, [ec.EDGE_RECT], ec.EDGE_SIZE, NAME[layout])
    assert int(got.max()) < 200                                                   # nothing from outside the crop


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_frame_placement(env, oracle, layout):
    """Device planes at addresses 0 .. 3 mod 4 with padded strides (the pair plane at odd addresses included), separately allocated;
    stacked tensors and stacked host arrays; strided host views; and a list mixing all of these."""
    import torch
    fr = frames_of(layout)
    rects = both_frames_rects()[::2]
    for variant in range(4):
        for kind in ("dev", "host"):
            holders = [Planes(f, kind, ((i + variant) % 4, (i + variant + 1) % 4, (3 * i + variant) % 4), ((i + variant) % 3, (2 * i + variant) % 5))
                       for i, f in enumerate(fr)]
            items = [h.yuv_item(layout) for h in holders]
            check(env, oracle, items, fr, layout, rects, (21, 17), NAME[layout], decoded_of(layout, variant % 2 == 1, variant >= 2), alpha=variant % 2 == 1,
                  rgb=variant >= 2)
            check_affine(env, oracle, items, fr, layout, ac.rows_for(0, [eyc.REPRESENTATIVE]), (21, 17), NAME[layout], alpha=variant % 2 == 1)
    # equal-size frames as ONE stacked device tensor and as one stacked host array
    same = [yc.random_frame(38, 30, layout, 80 + i) for i in range(3)]
    stack = np.stack([yc.stacked(f, layout) for f in same])
    t = torch.from_numpy(stack).cuda()
    torch.cuda.synchronize()
    r3 = eyc.crops(0)[::5] + eyc.crops(1)[1::5] + eyc.crops(2)[2::5]
    check(env, oracle, YuvFrames.from_torch(t, NAME[layout]), same, layout, r3, (21, 17))
    check(env, oracle, stack, same, layout, r3, (21, 17), NAME[layout])
    # a list mixing a stacked tensor, separately placed device planes, a stacked host array and strided host views
    items = [YuvFrames.from_torch(t[:1], NAME[layout]), Planes(same[1], "dev", (1, 3, 2), (2, 3)).yuv_item(layout), yc.stacked(same[2], layout),
             Planes(fr[1], "host", (3, 1, 2), (1, 4)).yuv_item(layout)]
    check(env, oracle, items, same + [fr[1]], layout, r3 + [(3, 50, 20, 20, 17)], (21, 17), NAME[layout], gray=True)


def test_mixed_sizes_layouts_and_residence_whole_and_in_slices(env, oracle):
    """yuv_cases.MIXED_SIZES: eleven frames, the three layouts and host / device frames mixed in one call; then in slices of 1, 2, 3."""
    rects = []
    for i, (w, h) in enumerate(yc.MIXED_SIZES):
        rects += [(i, 1, 1, max(w // 2, 1), max(h // 2, 1)), (i, -3, h - 9, 14, 12), (i, 0, 0, w, h)]
    rects = [rects[k] for k in np.random.default_rng(5).permutation(len(rects))]     # slices of regions, not of frames
    rows = np.array([[r[0]] + ac.from_rect(r[1], r[2], r[3], r[4], (12, 10)) for r in rects], np.float64)
    for lay in LAYOUTS:
        # host frames take the call's layout; the device frames carry theirs
        layouts = [lay if i % 2 else LAYOUTS[i % 3] for i in range(len(yc.MIXED_SIZES))]
        fr = [yc.random_frame(w, h, L, 18) for (w, h), L in zip(yc.MIXED_SIZES, layouts)]
        items = [f if i % 2 else Planes(f, "dev", (i % 4, (i + 1) % 4, (i + 2) % 4), (i % 3, i % 2)).yuv_item(L) for i, (f, L) in enumerate(zip(fr, layouts))]
        check(env, oracle, items, fr, layouts, rects, (12, 10), NAME[lay])
        for k in (1, 2, 3):
            with tunables(env, ("max_subbatch", str(k))):
                check(env, oracle, items, fr, layouts, rects, (12, 10), NAME[lay], alpha=k == 2, planar=k == 3)
                check_affine(env, oracle, items, fr, layouts, rows, (12, 10), NAME[lay], gray=k == 1)
    # two calls in a row with different sizes: the environment's block is reused
    check(env, oracle, items[:3], fr[:3], layouts[:3], [r for r in rects if r[0] < 3], (7, 3), NAME[lay])
    check(env, oracle, items, fr, layouts, rects, (24, 24), NAME[lay])


def test_a_callers_tensor_at_an_odd_address_and_no_regions(env, oracle):
    import torch
    fr = frames_of(yc.NV12)
    rects = both_frames_rects()[::4]
    want = eyc.restate(oracle, fr, yc.NV12, rects, (21, 17))
    rows = ac.rows_for(1, [eyc.REPRESENTATIVE, ac.identity()])
    awant = eyc.restate_affine(oracle, fr, yc.NV12, rows, (21, 17), alpha=True)
    for w, call in ((want, lambda o: env.extract_yuv(fr, rects, (21, 17), out=o)), (awant, lambda o: env.extract_affine_yuv(fr, rows, (21, 17), alpha=True, out=o))):
        buf = torch.full((w.size + 2,), 0xA5, dtype=torch.uint8, device="cuda")
        out = buf[1:-1]
        assert out.data_ptr() % 2 == 1
        for _ in range(2):
            res = call(out)
            assert res.data_ptr() == out.data_ptr() and np.array_equal(res.cpu().numpy(), w)
        assert int(buf[0]) == 0xA5 and int(buf[-1]) == 0xA5                       # not a byte outside it
        for bad in (out[:-1], torch.zeros(w.size, dtype=torch.uint8), torch.zeros(w.size, dtype=torch.int8, device="cuda"),
                    torch.zeros(2 * w.size, dtype=torch.uint8, device="cuda")[::2]):
            with pytest.raises(ValueError):
                call(bad)
    assert env.extract_yuv(fr, np.zeros((0, 5), np.int32), (24, 24)).shape == (0, 24, 24, 3)
    assert env.extract_yuv(fr, [], (24, 24), planar=True, alpha=True).shape == (0, 4, 24, 24)
    assert env.extract_affine_yuv(fr, np.zeros((0, 7)), (24, 24), gray=True).shape == (0, 24, 24, 1)
    assert env.extract_affine_yuv([], np.zeros(0, AFFINE_DTYPE), (24, 24), planar=True).shape == (0, 3, 24, 24)


# ------------------------------------------------------------------------------------------------------------------- 2. the affine call
@pytest.mark.parametrize("layout", LAYOUTS)
def test_affine_families(env, oracle, layout):
    """Identity, integer translations, the rotation and its mirror, the shear and the scales, the tie family, the edge matrices."""
    fr = frames_of(layout)
    for k, (name, ms, size) in enumerate(eyc.affine_matrices()):
        got = check_affine(env, oracle, fr, fr, layout, ac.rows_for(0, ms), size, NAME[layout], alpha=k % 2 == 1, rgb=k % 3 == 1)
        if name == "identity":
            assert np.array_equal(got[0][..., :3], decoded_of(layout, False, False)[0])
        if name == "translation":                                               # an integer translation is the replicated-border crop
            assert np.array_equal(got[1][..., :3], ec.padded_crop(decoded_of(layout, False, True)[0], -4, 5, 20, 17))
    check_affine(env, oracle, fr, fr, layout, ac.rows_for(1, ac.edge_matrices() + [ac.ROT]), (33, 21), NAME[layout])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_affine_flags_and_output_sizes(env, oracle, layout):
    fr = frames_of(layout)
    rows = np.concatenate([ac.rows_for(0, [eyc.REPRESENTATIVE, ac.mirrored(eyc.REPRESENTATIVE, 21)]), ac.rows_for(1, [eyc.REPRESENTATIVE])])
    for flags in eyc.FLAG_CASES:
        check_affine(env, oracle, fr, fr, layout, rows, (21, 17), NAME[layout], **flags)
    for i, w in enumerate(eyc.OUT_WIDTHS):
        check_affine(env, oracle, fr, fr, layout, rows[:2], (w, eyc.OUT_HEIGHTS[i % len(eyc.OUT_HEIGHTS)]), NAME[layout], alpha=i % 3 == 1, planar=i % 4 == 3)


# ------------------------------------------------------------------------------------------------------------------- 3. end to end
def test_faces_cut_from_decoder_frames(env, oracle, cascades):
    """The NV12 that yuv_cases.encode makes of the 432 x 324 colour sources: detect_opencv_chain(frontalface_alt, eye) on the Y planes,
    align_transforms, then the boxes through extract_yuv and the aligned crops through extract_affine_yuv — no BGR frame anywhere."""
    import torch
    c1, _ = cascades(pc.CASC)
    c2, _ = cascades("eye")
    nv12 = eyc.e2e_nv12()
    t = torch.from_numpy(np.stack([yc.stacked(f, yc.NV12) for f in nv12])).cuda()
    torch.cuda.synchronize()
    yuv = YuvFrames.from_torch(t)
    faces, eyes = env.detect_opencv_chain(c1, c2, yuv.luma(), min_neighbors=3)
    print(f"end to end: {len(faces.rects)} faces, {len(eyes.rects)} eye candidates")
    assert len(faces.rects) >= 3
    crops = env.extract_yuv(yuv, faces.rects, (112, 112), margin=0.1)
    assert crops.shape == (len(faces.rects), 112, 112, 3) and crops.dtype == torch.uint8 and crops.is_cuda
    assert np.array_equal(crops.cpu().numpy(), eyc.restate(oracle, nv12, yc.NV12, faces.rects, (112, 112), margin=0.1))
    affines, paired = align_transforms(faces, eyes, (32, 32))
    for kw in (dict(), dict(gray=True), dict(planar=True, alpha=True, rgb=True)):
        got = env.extract_affine_yuv(yuv, affines, (32, 32), **kw).cpu().numpy()
        assert np.array_equal(got, eyc.restate_affine(oracle, nv12, yc.NV12, affines, (32, 32), **kw)), kw
    # the hand-made paired case of affine_cases: the branch through the eyes, turned
    affines, paired = align_transforms(ac.rects(ac.HAND_FACES), ac.rects(ac.HAND_EYES), (32, 32), scale=ec.MANY_SCALE)
    assert paired.tolist() == [True, False, True]
    check_affine(env, oracle, yuv, nv12, yc.NV12, ac.as_rows(affines), (32, 32))


# ------------------------------------------------------------------------------------------------------------------- 4. the errors
def test_argument_errors_leave_the_destination_and_the_environment_untouched(env, lib, oracle, cascades):
    import torch
    c, _ = cascades(pc.CASC)
    plain = mc.frames()[0]
    base = env.detect(c, plain)
    assert len(base.rects) >= 10
    fr = frames_of(yc.NV12)
    holder = Planes(fr[0], "dev")
    host = Planes(fr[1], "host", (1, 2, 0), (3, 1))
    dev_item = holder.yuv_item(yc.NV12)
    hy, hc = host.views
    ok = [_YuvImage(dev_item.ptr_y, dev_item.ptr_c0, None, 38, 30, dev_item.y_stride, dev_item.c_stride, yc.NV12, 1),
          _YuvImage(hy.ctypes.data, hc.ctypes.data, None, 66, 34, hy.strides[0], hc.strides[0], yc.NV12, 0)]
    dst = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    good = [(0, 3, 4, 20, 17), (1, 40, 10, 30, 30)]
    agood = [(0, 0) + tuple(eyc.REPRESENTATIVE), (1, 0) + tuple(ac.translation(-3, 2))]
    need = 2 * 24 * 24 * 3

    def call(affine, images=ok, n=None, rows=None, nr=None, p=True, yp=True, d=dst.data_ptr(), nbytes=dst.numel(), e=env._h, channels=3, yflags=0, yreserved=0,
             expect_clean=True, **kw):
        rows = (agood if affine else good) if rows is None else rows
        if affine:
            q = AffineParams()
            lib.vj_affine_default(C.byref(q))
            r = np.zeros(len(rows), AFFINE_DTYPE)
            for i, row in enumerate(rows):
                r[i] = (row[0], row[1], row[2:])
        else:
            q = ExtractParams()
            lib.vj_extract_default(C.byref(q))
            r = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 5))
        q.out_w, q.out_h = 24, 24
        for k, v in kw.items():
            setattr(q, k, v)
        y = YuvParams()
        lib.vj_yuv_default(C.byref(y))
        y.channels, y.flags, y.reserved = channels, yflags, yreserved
        arr = (_YuvImage * max(len(images), 1))(*images) if images is not None else None
        f = lib.vj_extract_affine_yuv if affine else lib.vj_extract_yuv
        rc = f(e, arr, (len(images) if images is not None else 2) if n is None else n, r.ctypes.data if len(r) else None,
               len(r) if nr is None else nr, C.byref(q) if p else None, C.byref(y) if yp else None, C.c_void_p(d), nbytes)
        err = lib.vj_last_error().decode()
        if rc != 0 and expect_clean:
            assert bool((dst == 0x5A).all()), "an error wrote into the destination"
        after = env.detect(c, plain)                                              # every error is followed by a plain detect
        assert np.array_equal(after.rects, base.rects)
        return rc, err

    for affine in (False, True):
        assert call(affine)[0] == 0
        dst.fill_(0x5A)
        torch.cuda.synchronize()
        # null arguments, negative counts
        for kw in (dict(e=None), dict(images=None), dict(p=False), dict(yp=False), dict(d=None), dict(n=-1), dict(nr=-1)):
            assert call(affine, **kw)[0] == VJ_ERR_ARG, kw
        # the frames by vj_yuv_to_bgr's rules
        y0, c0 = ok[0].y, ok[0].c0
        for bad, word in ((_YuvImage(None, c0, None, 8, 4, 8, 8, 0, 1), "null y"), (_YuvImage(y0, None, None, 8, 4, 8, 8, 0, 1), "null c0"),
                          (_YuvImage(y0, c0, None, 8, 4, 8, 4, 2, 1), "null c1"), (_YuvImage(y0, c0, None, 7, 4, 8, 8, 0, 1), "even"),
                          (_YuvImage(y0, c0, None, 8, 0, 8, 8, 0, 1), "positive"), (_YuvImage(y0, c0, None, 8, 4, 7, 8, 0, 1), "y_stride"),
                          (_YuvImage(y0, c0, None, 8, 4, 8, 7, 0, 1), "c_stride"), (_YuvImage(y0, c0, None, 8, 4, 8, 8, 5, 1), "layout")):
            rc, err = call(affine, images=ok + [bad])
            assert rc == VJ_ERR_ARG and "frame 2" in err and word in err, err
        rc, err = call(affine, images=ok + [_YuvImage(y0, c0, None, 65536, 2, 65536, 65536, 0, 1)])
        assert rc == VJ_ERR_LIMIT and "frame 2" in err and "65534" in err
        # yp
        for kw, word in ((dict(channels=1), "channels"), (dict(channels=5), "channels"), (dict(yflags=2), "flags"), (dict(yreserved=1), "reserved")):
            rc, err = call(affine, **kw)
            assert rc == VJ_ERR_ARG and "vj_yuv_params" in err and word in err, kw
        # the fields of the call's own parameters
        for kw, word in [(dict(out_w=0), "out_w"), (dict(out_h=-1), "out_h"), (dict(flags=4), "flags"), (dict(reserved=7), "reserved")]:
            rc, err = call(affine, **kw)
            assert rc == VJ_ERR_ARG and word in err, kw
        rc, err = call(affine, out_w=65536)
        assert rc == VJ_ERR_LIMIT and "65535" in err
        # dst_bytes too small, by one byte
        rc, err = call(affine, nbytes=need - 1)
        assert rc == VJ_ERR_ARG and "dst_bytes" in err
        assert call(affine, nbytes=need)[0] == 0
        dst.fill_(0x5A)
        torch.cuda.synchronize()
        # a device-resident source plane that overlaps the destination: the Y plane's first byte, the pair plane's last byte
        before = holder.t.cpu().numpy().copy()
        cend = ok[0].c0 + 14 * ok[0].c_stride + 38
        for d0, word in ((ok[0].y - need + 1, "y plane"), (cend - 1, "c0 plane")):
            rc, err = call(affine, d=d0, nbytes=need, expect_clean=False)
            assert rc == VJ_ERR_ARG and "frame 0" in err and "overlaps" in err and word in err, err
        assert np.array_equal(holder.t.cpu().numpy(), before) and bool((dst == 0x5A).all())    # nothing was written
        # zero rows
        assert call(affine, rows=[])[0] == 0
    # the rows of each call
    for bad, word in (((2, 0, 0, 4, 4), "frame 2"), ((-1, 0, 0, 4, 4), "frame -1"), ((0, 0, 0, 0, 4), "w and h"), ((0, 0, 0, 65536, 4), "65535"),
                      ((0, (1 << 24) + 1, 0, 4, 4), "2^24")):
        rc, err = call(False, rows=good + [bad])
        assert rc == (VJ_ERR_LIMIT if word in ("65535", "2^24") else VJ_ERR_ARG) and "region 2" in err and word in err, err
    for kw, word in [(dict(sx=-1.0), "sx"), (dict(sy=float("nan")), "sy"), (dict(margin=float("inf")), "margin")]:
        rc, err = call(False, **kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    ident = tuple(ac.identity())
    for bad, word, code in (((2, 0) + ident, "frame", VJ_ERR_ARG), ((0, 1) + ident, "reserved", VJ_ERR_ARG), ((0, 0, float("nan")) + ident[1:], "m[0]", VJ_ERR_ARG),
                            ((0, 0, 1.0, 0.0, 2.0 ** 19 + 1, 0.0, 1.0, 0.0), "m[2]", VJ_ERR_LIMIT)):
        rc, err = call(True, rows=agood + [bad])
        assert rc == code and "affine 2" in err and word in err, err
    # and the environment still cuts: the same two frames, one resident on the device, one a strided host view
    items = [dev_item, host.yuv_item(yc.NV12)]
    check(env, oracle, items, fr, yc.NV12, good, (24, 24))
    check_affine(env, oracle, items, fr, yc.NV12, np.array([(g[0],) + g[2:] for g in agood], np.float64), (24, 24))
    with pytest.raises(VjError):
        env.extract_yuv(items, [(2, 0, 0, 4, 4)], (24, 24))
