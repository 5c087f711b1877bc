"""vj_yuv_to_bgr / vj_bgr_to_yuv on the device: the WHOLE destination buffer of every call, downloaded — the pad
bytes inside the pitches, the gaps between the frames and a sentinel margin behind the layout's bytes included — against the numpy
restatement of tests/yuv_cases.py with np.array_equal.  The premises (the known answers, the wrong variants, the ranges the frames
reach) are checked on the CPU in tests/test_yuv_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import mixed_cases as mc
import paint_cases as pcs
import prep_cases as pc
import yuv_cases as yc
from cases import tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, DeviceFrames, VjError, YuvFrames, YuvParams
from clfacedetection_amd.api import _Image, _YuvImage
from test_gpu_equalize import _against

pytestmark = pytest.mark.gpu
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8
SENTINEL, MARGIN = 0xA5, 96
LAYOUTS = [yc.NV12, yc.NV21, yc.I420]
NAME = yc.LAYOUT_NAMES
SHAPES = [(w, h) for h in yc.HEIGHTS for w in yc.WIDTHS]


# ------------------------------------------------------------------------------------------------------------------- helpers
class Planes:
    """Planes (or one interleaved image) in a buffer of their own, each `offsets[k]` bytes behind a multiple of 4 and with rows
    `pads[k]` bytes further apart than they are long, everything that is no pixel holding the sentinel: strided host views, or
    device memory.  The chroma planes of I420 share one stride, as vj_yuv_image asks."""

    def __init__(self, planes, kind, offsets=(0, 0, 0), pads=(0, 0, 0)):
        import torch
        rows = [np.asarray(p).reshape(p.shape[0], -1) for p in planes]
        strides = [rows[0].shape[1] + pads[0]] + [r.shape[1] + pads[1] for r in rows[1:]]
        at, starts = 0, []
        for r, s, o in zip(rows, strides, offsets):
            at = yc.align(at, 4) + o
            starts.append(at)
            at += r.shape[0] * s
        self.base = np.full(at, SENTINEL, np.uint8)
        self.views = []
        for r, s, st in zip(rows, strides, starts):
            v = np.lib.stride_tricks.as_strided(self.base[st:], shape=r.shape, strides=(s, 1), writeable=True)
            v[:] = r
            self.views.append(v)
        self.strides, self.starts, self.kind = strides, starts, kind
        if kind == "dev":
            self.t = torch.from_numpy(self.base).cuda()
            torch.cuda.synchronize()

    def ptr(self, k):
        return self.t.data_ptr() + self.starts[k]

    def yuv_item(self, layout):
        h, w = self.views[0].shape
        if self.kind == "host":
            return tuple(self.views)
        return YuvFrames(self.ptr(0), self.ptr(1), self.ptr(2) if layout == yc.I420 else 0, 1, h, w, self.strides[0], self.strides[1], layout, 0, self.t)

    def bgr_item(self, img):
        h, w, ch = img.shape
        if self.kind == "host":
            return np.lib.stride_tricks.as_strided(self.base[self.starts[0]:], shape=(h, w, ch), strides=(self.strides[0], ch, 1))
        return DeviceFrames(self.ptr(0), 1, h, w, self.strides[0], ch, 0, self.t)


def first_bad(got, want):
    bad = np.flatnonzero(got != want)
    return ("first bad byte", int(bad[0]), "of", len(bad), "got", int(got[bad[0]]), "want", int(want[bad[0]]))


def check_decode(env, items, frames, layouts, alpha, rgb, host_layout="nv12"):
    """One yuv_to_bgr() call into a sentinel-filled buffer of the caller's, every byte of it against the restatement."""
    import torch
    ch = 4 if alpha else 3
    recs, nbytes = env.yuv_to_bgr_layout(items, alpha=alpha, rgb=rgb, layout=host_layout)
    want, wrecs, wbytes = yc.decode_buffer(frames, layouts, ch, rgb, nbytes + MARGIN, SENTINEL)
    assert nbytes == wbytes and recs == wrecs
    buf = torch.full((nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    outs = env.yuv_to_bgr(items, alpha=alpha, rgb=rgb, out=buf, layout=host_layout)
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), (alpha, rgb, first_bad(got, want))
    flat = [(d.frame_ptr(i) - buf.data_ptr(), d.width, d.height, d.stride) for d in outs for i in range(d.n)]
    assert flat == recs and all(d.channels == ch and d.owner is buf for d in outs)
    return outs


def check_encode(env, items, images, layout, rgb):
    import torch
    recs, nbytes = env.bgr_to_yuv_layout(items, layout=NAME[layout], rgb=rgb)
    want, wrecs, wbytes = yc.encode_buffer(images, layout, rgb, nbytes + MARGIN, SENTINEL)
    assert nbytes == wbytes and [r[:3] if layout == yc.I420 else r[:2] for r in recs] == wrecs
    buf = torch.full((nbytes + MARGIN,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    outs = env.bgr_to_yuv(items, layout=NAME[layout], rgb=rgb, out=buf)
    got = buf.cpu().numpy()
    assert np.array_equal(got, want), (layout, rgb, first_bad(got, want))
    outs = outs if isinstance(outs, list) else [outs]
    flat = [(d.ptr_y + i * d.frame_bytes - buf.data_ptr(), d.width, d.height) for d in outs for i in range(d.n)]
    assert flat == [(r[0], r[3], r[4]) for r in recs] and all(d.layout == layout and d.owner is buf for d in outs)
    return outs


_ONCE = {}


def once(key, build):
    if key not in _ONCE:
        _ONCE[key] = build()
    return _ONCE[key]


def shape_frames(layout):
    return once(("frames", layout), lambda: [yc.random_frame(w, h, layout, 11) for w, h in SHAPES])


def shape_images(ch):
    return once(("images", ch), lambda: [yc.random_image(w, h, ch, 12) for w, h in SHAPES])


# ------------------------------------------------------------------------------------------------------------------- 1. decode
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_every_shape(env, layout, alpha, rgb):
    """Widths around a lane, a wave's row and two blocks at heights around a row pair and one and two blocks: one call of host planes."""
    frames = shape_frames(layout)
    check_decode(env, frames, frames, layout, alpha, rgb, NAME[layout])
    assert env.yuv_timing() > 0


@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_every_term(env, layout, alpha):
    """All (Y, U) with V in {0, 127, 128, 129, 255} and all (Y, V) with U in the same set, as ONE stacked device tensor."""
    import torch
    frames = once(("exhaustive", layout), lambda: yc.exhaustive_frames(layout))
    t = torch.from_numpy(np.stack([yc.stacked(f, layout) for f in frames])).cuda()
    torch.cuda.synchronize()
    y = YuvFrames.from_torch(t, NAME[layout])
    assert (y.n, y.width, y.height) == (10, 256, 256)
    for rgb in (False, True):
        outs = check_decode(env, y, frames, layout, alpha, rgb)
        assert len(outs) == 1 and outs[0].n == 10                                 # equal sizes: one DeviceFrames, as preprocess() returns
    # the same frames as a stacked host array
    check_decode(env, np.stack([yc.stacked(f, layout) for f in frames[:2]]), frames[:2], layout, alpha, False, NAME[layout])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decode_every_address_and_stride(env, layout):
    """Separately placed planes at addresses 0 .. 3 mod 4 with padded strides, in device memory and as strided host views: the byte
    path of every plane, and the dword path beside it in the same call."""
    sizes = [(2, 2), (6, 4), (8, 6), (66, 6), (258, 4), (64, 34)]
    frames = [yc.random_frame(w, h, layout, 13 + i) for i, (w, h) in enumerate(sizes)]
    for variant in range(4):
        for kind in ("dev", "host"):
            holders = [Planes(f, kind, ((i + variant) % 4, (i + 2 * variant + 1) % 4, (3 * i + variant) % 4), ((i + variant) % 3, (2 * i + variant) % 5))
                       for i, f in enumerate(frames)]
            items = [h.yuv_item(layout) for h in holders]
            check_decode(env, items, frames, layout, variant % 2 == 1, variant >= 2, NAME[layout])


def test_decode_mixed_sizes_layouts_and_residence_whole_and_in_slices(env):
    """Eleven frames of differing even sizes, the three layouts and host / device frames mixed in one call; then in slices."""
    layouts = [LAYOUTS[i % 3] for i in range(len(yc.MIXED_SIZES))]
    frames = [yc.random_frame(w, h, lay, 17) for (w, h), lay in zip(yc.MIXED_SIZES, layouts)]
    dev = [Planes(f, "dev", (i % 4, (i + 1) % 4, (i + 2) % 4), (i % 3, i % 2)).yuv_item(lay) for i, (f, lay) in enumerate(zip(frames, layouts))]
    outs = check_decode(env, dev, frames, layouts, False, False)
    assert len(outs) == len(frames)                                               # differing sizes: one DeviceFrames per frame
    # host frames take the call's layout: per layout, host and device frames alternating
    for lay in LAYOUTS:
        fr = [yc.random_frame(w, h, lay, 18) for w, h in yc.MIXED_SIZES]
        items = [f if i % 2 else Planes(f, "dev").yuv_item(lay) for i, f in enumerate(fr)]
        check_decode(env, items, fr, lay, True, True, NAME[lay])
        for k in (1, 2, 3):
            with tunables(env, ("max_subbatch", str(k))):
                check_decode(env, items, fr, lay, k == 2, k == 3, NAME[lay])
    # two calls in a row with different sizes: the environment's block is reused
    check_decode(env, dev[:3], frames[:3], layouts[:3], True, False)
    check_decode(env, dev, frames, layouts, False, True)
    assert env.yuv_to_bgr([]) == [] and env.bgr_to_yuv([]) == []                  # n = 0


# ------------------------------------------------------------------------------------------------------------------- 2. encode
@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_every_shape(env, layout, ch, rgb):
    images = shape_images(ch)
    check_encode(env, images, images, layout, rgb)
    assert env.yuv_timing() > 0


@pytest.mark.parametrize("ch", [3, 4])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_corners_ramps_and_wild_frames(env, layout, ch):
    """The cube's corners, gray ramps, per-channel ramps with the others at 0 and 255, and a frame whose odd rows and columns differ
    wildly from the even ones — where averaged or bottom-right chroma would differ (tests/test_yuv_cpu.py)."""
    images = once(("sweeps", ch), lambda: yc.encode_images(ch))
    for rgb in (False, True):
        outs = check_encode(env, images, images, layout, rgb)
        assert len(outs) == len(images)
    # frames of one size come back as ONE YuvFrames; its luma() is the Y planes
    same = [yc.wild_image(66, 6, s)[..., :3] for s in (5, 6, 7)]
    import torch
    out = env.bgr_to_yuv(np.stack(same), layout=NAME[layout])
    assert isinstance(out, YuvFrames) and out.n == 3 and out.frame_bytes % 256 == 0
    g = out.luma()
    assert (g.ptr, g.n, g.width, g.height, g.stride, g.channels, g.frame_bytes) == (out.ptr_y, 3, 66, 6, 68, 1, out.frame_bytes)
    host = out.owner.cpu().numpy()
    for i, im in enumerate(same):
        y = host[i * out.frame_bytes: i * out.frame_bytes + 68 * 6].reshape(6, 68)
        assert np.array_equal(y[:, :66], yc.encode(im, layout)[0]) and not y[:, 66:].any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_encode_every_address_and_stride_mixed_channels_and_slices(env, layout):
    """Sources at addresses 0 .. 3 mod 4 with padded strides, device and host, BGR and BGRA mixed in one call; the eleven sizes in
    slices."""
    sizes = [(2, 2), (6, 4), (8, 6), (66, 6), (258, 4), (64, 34)]
    images = [yc.random_image(w, h, 3 + i % 2, 21) for i, (w, h) in enumerate(sizes)]
    for variant in range(4):
        for kind in ("dev", "host"):
            items = [Planes([im], kind, ((i + variant) % 4,), ((2 * i + variant) % 5,)).bgr_item(im) for i, im in enumerate(images)]
            check_encode(env, items, images, layout, variant >= 2)
    images = [yc.random_image(w, h, 4 - i % 2, 22) for i, (w, h) in enumerate(yc.MIXED_SIZES)]
    items = [im if i % 2 else Planes([im], "dev", (i % 4,), (i % 3,)).bgr_item(im) for i, im in enumerate(images)]
    check_encode(env, items, images, layout, False)
    for k in (1, 2, 3):
        with tunables(env, ("max_subbatch", str(k))):
            check_encode(env, items, images, layout, k == 2)


# --------------------------------------------------------------------------------------------------------------- 3. end to end
def test_decoder_to_encoder_around_the_detector(env, oracle, cascades):
    """The NV12 the restatement makes of the 432 x 324 colour sources of tests/test_gpu_paint.py: detect on luma(), cut the boxes
    out of yuv_to_bgr()'s frames, blur them there and encode again — each step against the restatements applied in the same order."""
    import torch
    c, a = cascades(pc.CASC)
    bgr = ec.e2e_bgr()
    nv12 = [yc.encode(f, yc.NV12) for f in bgr]
    t = torch.from_numpy(np.stack([yc.stacked(f, yc.NV12) for f in nv12])).cuda()
    torch.cuda.synchronize()
    y = YuvFrames.from_torch(t)
    # detect on the Y plane: rectangles, order and counters
    cv = once("e2e_cv", lambda: [oracle.detect_opencvlike(a, np.ascontiguousarray(f[0])) for f in nv12])
    _against(env.detect_opencv(c, y.luma(), flags=VJ_FLAG_COUNTERS), cv, a)
    rects = env.detect_opencv(c, y.luma(), min_neighbors=3).rects
    assert len(rects) >= 3
    # the colour frames the boxes are cut from and painted into
    frames = env.yuv_to_bgr(y)[0]
    decoded = [yc.decode(f, yc.NV12) for f in nv12]
    got = frames.owner.cpu().numpy()
    for i, d in enumerate(decoded):
        off = frames.frame_ptr(i) - frames.owner.data_ptr()
        assert np.array_equal(got[off:off + d.size].reshape(d.shape), d)
    crops = env.extract(frames, rects, ec.MANY_SIZE, margin=0.1, color=True)
    assert np.array_equal(crops.cpu().numpy(), ec.restate(oracle, decoded, rects, ec.MANY_SIZE, margin=0.1))
    kw = dict(margin=0.1)
    painted = pcs.restate(decoded, rects, "blur", **kw)
    assert any(not np.array_equal(p, d) for p, d in zip(painted, decoded))
    assert env.paint(frames, rects, "blur", **kw) is frames
    out = check_encode(env, frames, painted, yc.NV12, False)[0]
    assert out.n == 3 and (out.width, out.height) == (432, 324)
    # ... and the encoder's output decodes again on the device
    check_decode(env, out, [yc.encode(p, yc.NV12) for p in painted], yc.NV12, False, False)


# ------------------------------------------------------------------------------------------------------------- 4. the error cases
def test_argument_errors_leave_the_environment_as_it_was(env, lib, cascades):
    import torch
    c, a = cascades(pc.CASC)
    plain = mc.frames()[0]
    base = env.detect(c, plain)
    assert len(base.rects) >= 10
    src = torch.zeros(8 * 6 + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s, d = src.data_ptr(), dst.data_ptr()
    good_y = _YuvImage(s, s + 32, s + 40, 8, 4, 8, 8, yc.NV12, 1)
    good_b = _Image(s, 4, 2, 12, 1, 3)

    def settled(rc, want, word=None):
        err = lib.vj_last_error().decode()
        assert rc == want and (word is None or word in err), (rc, err)
        assert (dst.cpu().numpy() == SENTINEL).all()                              # nothing was written ...
        assert np.array_equal(env.detect(c, plain).rects, base.rects)             # ... and a plain detect still matches

    def decode(images=(good_y,), n=None, e=env._h, p=True, dptr=d, dbytes=4096, out=True, **kw):
        q = YuvParams()
        lib.vj_yuv_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_YuvImage * max(len(images), 1))(*images) if images is not None else None
        res = (_Image * 4)()
        return lib.vj_yuv_to_bgr(e, arr, (len(images) if images is not None else 1) if n is None else n, C.byref(q) if p else None, dptr, dbytes,
                                 res if out else None)

    def encode(images=(good_b,), n=None, e=env._h, p=True, layout=yc.NV12, dptr=d, dbytes=4096, out=True, **kw):
        q = YuvParams()
        lib.vj_yuv_default(C.byref(q))
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images) if images is not None else None
        res = (_YuvImage * 4)()
        return lib.vj_bgr_to_yuv(e, arr, (len(images) if images is not None else 1) if n is None else n, C.byref(q) if p else None, layout, dptr,
                                 dbytes, res if out else None)

    for call in (decode, encode):
        for kw in (dict(e=None), dict(images=None), dict(p=False), dict(n=-1), dict(dptr=None), dict(out=False)):
            settled(call(**kw), VJ_ERR_ARG)
        settled(call(flags=2), VJ_ERR_ARG, "flags")
        settled(call(reserved=1), VJ_ERR_ARG, "reserved")
        settled(call(dptr=d + 2), VJ_ERR_ARG, "multiple of 4")
        settled(call(dbytes=8), VJ_ERR_ARG, "dst_bytes")
    settled(decode(channels=1), VJ_ERR_ARG, "channels")
    settled(decode(dbytes=8 * 4 * 3 - 1), VJ_ERR_ARG, "dst_bytes")
    settled(encode(dbytes=4 * 2 + 4 * 1 - 1), VJ_ERR_ARG, "dst_bytes")
    settled(encode(layout=3), VJ_ERR_ARG, "layout")
    for bad, word in [(_YuvImage(None, s, s, 8, 4, 8, 8, 0, 1), "null y"), (_YuvImage(s, None, s, 8, 4, 8, 8, 0, 1), "null c0"),
                      (_YuvImage(s, s, None, 8, 4, 8, 4, 2, 1), "null c1"), (_YuvImage(s, s, s, 7, 4, 8, 8, 0, 1), "even"),
                      (_YuvImage(s, s, s, 8, 0, 8, 8, 0, 1), "positive"), (_YuvImage(s, s, s, 8, 4, 7, 8, 0, 1), "y_stride"),
                      (_YuvImage(s, s, s, 8, 4, 8, 3, 2, 1), "c_stride"), (_YuvImage(s, s, s, 8, 4, 8, 8, 5, 1), "layout")]:
        settled(decode(images=(good_y, bad)), VJ_ERR_ARG, "frame 1")
        assert word in lib.vj_last_error().decode()
    settled(decode(images=(_YuvImage(s, s, s, 65536, 2, 65536, 65536, 0, 1),), dbytes=1 << 40), VJ_ERR_LIMIT, "65534")
    for bad, word in [(_Image(None, 4, 2, 12, 1, 3), "null data"), (_Image(s, 4, 2, 4, 1, 1), "gray"), (_Image(s, 3, 2, 12, 1, 3), "even"),
                      (_Image(s, 4, 2, 11, 1, 3), "stride")]:
        settled(encode(images=(good_b, bad)), VJ_ERR_ARG, "frame 1")
        assert word in lib.vj_last_error().decode()
    settled(encode(images=(_Image(s, 2, 65536, 6, 1, 3),), dbytes=1 << 40), VJ_ERR_LIMIT, "65534")
    # a device-resident source plane inside the destination: each plane is looked at
    for k, word in enumerate(("y plane", "c0 plane", "c1 plane")):
        ptrs = [s, s + 32, s + 40]
        ptrs[k] = d + 16                                                          # inside the 96 bytes the layout needs
        settled(decode(images=(_YuvImage(*ptrs, 8, 4, 8, 4, yc.I420, 1),)), VJ_ERR_ARG, word)
    settled(encode(images=(_Image(d + 8, 4, 2, 12, 1, 3),)), VJ_ERR_ARG, "overlaps")
    # the wrapper's own refusals
    with pytest.raises(ValueError):
        env.yuv_to_bgr(np.zeros((6, 4), np.uint8), layout="yuy2")
    with pytest.raises(VjError):
        env.yuv_to_bgr(np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError):
        env.yuv_to_bgr(np.zeros((6, 4), np.uint8), out=torch.zeros(4096, dtype=torch.uint8))
    # ... and after all of it both directions still work
    f = yc.random_frame(8, 4, yc.NV12, 1)
    check_decode(env, [f], [f], yc.NV12, False, False)
