"""vj_preprocess on the device: the bytes of Environment.preprocess, downloaded, against the composition of the
existing restatements — equalize(resize_linear(gray)), tests/prep_cases.py — with np.array_equal, pad columns 0; then every detect
entry point on its output against the oracles on the restatement's frames, with rectangles, order and counters.  The premise of the
end-to-end part (preprocessing changes what the detector finds in these frames, and it finds something) is checked on the CPU in
tests/test_prep_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import clod_window_oracle as cw
import cv_rois_cases as cc
import mixed_cases as mc
import prep_cases as pc
import run_window_oracle as rw
from cases import tunables
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CHAIN_DEVICE, VJ_FLAG_EQUALIZE_HIST, VJ_PREP_EQUALIZE, DeviceFrames, Prep,
                                 VjError, default_params, run_windows, run_windows_opencv)
from clfacedetection_amd.api import _Image
from test_gpu_equalize import _against
from test_gpu_mixed import _color, _device_frame, _strided_view

pytestmark = pytest.mark.gpu
CNT = VJ_FLAG_COUNTERS
VJ_ERR_ARG, VJ_ERR_LIMIT = 1, 8


def download(outs):
    """Every output image of a preprocess() result, with its pad columns: a list of (h, stride) arrays and their widths."""
    imgs = []
    for d in outs:
        host = d.owner.cpu().numpy()
        for i in range(d.n):
            off = d.frame_ptr(i) - d.owner.data_ptr()
            assert off % 256 == 0 and d.stride == (d.width + 3) // 4 * 4 and d.channels == 1
            imgs.append((host[off:off + d.stride * d.height].reshape(d.height, d.stride), d.width))
    return imgs


def check(env, oracle, items, sources=None, color=False, **kw):
    """One preprocess() call against the restatement of every source; returns the call's result."""
    sources = items if sources is None else sources
    if isinstance(sources, np.ndarray) and sources.ndim == (3 if color else 2):
        sources = [sources]
    outs = env.preprocess(items, color=color, **kw)
    got = download(outs)
    assert len(got) == len(sources)
    for i, ((img, w), src) in enumerate(zip(got, sources)):
        want = pc.restate(oracle, src, **kw)
        assert img.shape[0] == want.shape[0] and w == want.shape[1], (i, kw)
        assert np.array_equal(img[:, :w], want), (i, src.shape, kw)
        assert not img[:, w:].any(), (i, src.shape, kw)                      # pad columns are written as 0
    return outs


# ----------------------------------------------------------------------------------------------------------------- 1. the bytes
@pytest.mark.parametrize("h", [1, 2, 5])
def test_small_and_block_edge_widths(env, oracle, h):
    """37 x 29 sources to widths around 4, a wave and a block, up-scaling included; gray, BGR and BGRA in one call."""
    rng = np.random.default_rng(h)
    srcs = [_color(rng, 29, 37, ch) for ch in (1, 3, 4)]
    for w in list(range(1, 10)) + [63, 64, 65, 255, 256, 257]:
        check(env, oracle, srcs, size=(w, h), equalize=True)
        check(env, oracle, srcs, size=(w, h))


def test_exact_halves_take_the_2x2_mean(env, oracle):
    rng = np.random.default_rng(11)
    keep = []
    for (w, h) in [(64, 48), (520, 66), (6, 2), (2, 2), (10, 6)]:
        srcs = [_color(rng, h, w, ch) for ch in (1, 3, 4)]
        for size in [(w // 2, h // 2), (w // 2, h), (w, h // 2)]:              # a half in one direction only is bilinear
            check(env, oracle, srcs, size=size, equalize=True)
        check(env, oracle, srcs, fx=0.5, fy=0.5)
        # device-resident sources: dword loads where a row starts at a multiple of 4, byte loads where it does not
        for off, pad in [(0, 0), (1, 3), (2, 1), (4, 4)]:
            items = []
            for s in srcs:
                d, t = _device_frame(s, off, pad)
                items.append(d)
                keep.append(t)
            check(env, oracle, items, srcs, size=(w // 2, h // 2), equalize=True)


def test_identity_and_no_resize(env, oracle):
    rng = np.random.default_rng(12)
    for (w, h) in [(37, 29), (5, 3), (1, 1), (257, 35), (64, 4)]:
        srcs = [_color(rng, h, w, ch) for ch in (1, 3, 4)]
        for kw in (dict(), dict(size=(w, h)), dict(fx=1.0, fy=1.0)):
            outs = check(env, oracle, srcs, **kw)
            check(env, oracle, srcs, equalize=True, **kw)
            assert len(outs) == 1 and outs[0].n == 3                           # one entry of n frames when all outputs share a size
            assert np.array_equal(download(outs)[0][0][:, :w], srcs[0])


def test_a_large_source_to_one_pixel(env, oracle):
    rng = np.random.default_rng(13)
    srcs = [_color(rng, 200, 300, ch) for ch in (1, 3)]
    check(env, oracle, srcs, size=(1, 1))
    check(env, oracle, srcs, size=(1, 1), equalize=True)
    check(env, oracle, srcs, fx=1e-6, fy=1e-6, equalize=True)


def test_color_strided_device_and_sources_that_end_with_their_last_row(env, oracle):
    rng = np.random.default_rng(5)
    keep = []
    for i, (h, w, ch) in enumerate([(37, 61, 3), (37, 61, 4), (5, 7, 3), (61, 131, 1), (2, 257, 4), (33, 64, 1)]):
        img = _color(rng, h, w, ch)
        for kw in (dict(fx=0.5, fy=0.5, equalize=True), dict(size=(w + 3, h + 2)), dict(equalize=True), dict(fx=0.7, fy=1.3)):
            check(env, oracle, np.ascontiguousarray(img), img, color=ch > 1, **kw)            # ends with its last row
            v, base = _strided_view(img, 7 if (w * ch) % 2 == 0 else 8)                       # a strided host view
            assert v.strides[0] % 2 == 1
            check(env, oracle, v, img, color=ch > 1, **kw)
            d, t = _device_frame(img, 1 + 2 * (i % 2), 0 if (w * ch) % 2 else 3)              # an odd address, stride > width
            assert d.ptr % 2 == 1 and d.stride % 2 == 1
            keep.append(t)
            check(env, oracle, d, [img], **kw)
            d, t = _device_frame(img, 0, 0)                                                   # tight rows: ends with the last row
            keep.append(t)
            check(env, oracle, d, [img], **kw)


# ------------------------------------------------------------------------------------------------------- 2. the histogram's edges
def test_pad_bytes_are_not_counted(env, oracle):
    """5 x 3: the three pad bytes of every row are 0 and would be the lowest bin of an image whose pixels are all >= 1."""
    rng = np.random.default_rng(21)
    for src in (_color(rng, 29, 37, 1), _color(rng, 3, 5, 1), _color(rng, 6, 10, 3)):
        for kw in (dict(size=(5, 3)), dict(size=(7, 2)), dict(size=(253, 3))):
            outs = check(env, oracle, [src], equalize=True, **kw)
            want = pc.restate(oracle, src, **kw)
            assert want.min() >= 1 and download(outs)[0][0][:, :kw["size"][0]].min() == 0     # the lowest value present maps to 0


@pytest.mark.parametrize("kind", ["constant0", "constant200", "two_valued", "rows_of_one_value", "all_values"])
def test_contents(env, oracle, kind):
    rng = np.random.default_rng(22)
    for w, h in [(256, 40), (512, 36), (130, 70)]:
        if kind.startswith("constant"):
            g = np.full((h, w), int(kind[8:]), np.uint8)
        elif kind == "two_valued":
            g = np.where(rng.random((h, w)) < 0.3, 17, 230).astype(np.uint8)
        elif kind == "rows_of_one_value":                                         # whole waves of one value: the ballot's branch
            g = np.repeat(rng.integers(0, 256, (h, 1), dtype=np.uint8), w, axis=1)
            g[-1, -1] ^= 0x55                                                     # ... and one pixel that is not
        else:
            g = rng.permutation(np.arange(h * w) % 256).astype(np.uint8).reshape(h, w)
            assert len(np.unique(g)) == 256
        outs = check(env, oracle, [g], equalize=True)                             # the result is the content's own kind
        if kind.startswith("constant"):
            assert np.array_equal(download(outs)[0][0][:, :w], g)                 # an image of one value is returned unchanged
        check(env, oracle, [g], size=(w // 2, h // 2), equalize=True)             # the 2 x 2 mean of constant rows is constant rows
        check(env, oracle, [np.repeat(g[..., None], 3, axis=2)], size=(w, h - 1), equalize=True)


# ------------------------------------------------------------------------------------------------- 3. mixed sizes, slices, reuse
def _mixed_items():
    """The eleven frames; frames 2 and 7 as BGR / BGRA on the host (their gray images are the frames: 1868 + 9617 + 4899 = 16384),
    frame 6 device-resident at an odd address."""
    items, keep = list(mc.frames()), []
    items[2] = np.repeat(items[2][..., None], 3, axis=2)
    items[7] = np.repeat(items[7][..., None], 4, axis=2)
    d, t = _device_frame(items[6], 3, 5)
    items[6] = d
    keep.append(t)
    return items, keep


@pytest.mark.parametrize("equalize", [False, True])
def test_eleven_frames_of_differing_sizes_in_one_call(env, oracle, equalize):
    items, keep = _mixed_items()
    outs = check(env, oracle, items, mc.frames(), fx=0.5, fy=0.5, equalize=equalize)
    assert len(outs) == len(mc.SIZES) and all(d.n == 1 for d in outs)
    assert [(d.width, d.height) for d in outs] == [pc.dst_size(w, h, fx=0.5, fy=0.5) for w, h in mc.SIZES]
    assert env.preprocess_timing() > 0
    with tunables(env, ("max_subbatch", "3")):                                    # four slices
        check(env, oracle, items, mc.frames(), fx=0.5, fy=0.5, equalize=equalize)
        check(env, oracle, items, mc.frames(), size=(33, 17), equalize=equalize)
    # two calls in a row with different sizes: the environment's buffers are reused
    check(env, oracle, items[:3], mc.frames()[:3], size=(300, 200), equalize=equalize)
    check(env, oracle, items, mc.frames(), fx=0.25, fy=0.75, equalize=equalize)
    check(env, oracle, items[:1], mc.frames()[:1], equalize=equalize)


def test_a_buffer_of_the_callers(env, oracle):
    import torch
    frames = list(mc.frames()[:4])
    recs, nbytes = env.preprocess_layout(frames, fx=0.5, fy=0.5, equalize=True)
    buf = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    outs = env.preprocess(frames, fx=0.5, fy=0.5, equalize=True, out=buf)
    assert [d.ptr - buf.data_ptr() for d in outs] == [r[0] for r in recs] and all(d.owner is buf for d in outs)
    host = buf.cpu().numpy()
    assert (host[nbytes:] == 0xAB).all()                                          # nothing beyond the layout's bytes is written
    for (off, w, h, stride), f in zip(recs, frames):
        img = host[off:off + stride * h].reshape(h, stride)
        assert np.array_equal(img[:, :w], pc.restate(oracle, f, fx=0.5, fy=0.5, equalize=True)) and not img[:, w:].any()
    assert env.preprocess([], size=(4, 4)) == []


# ------------------------------------------------------------------------------------------------------------- 4. end to end
def _prepared(env, equalize=True):
    outs = env.preprocess(pc.e2e_frames(), size=pc.E2E_SIZE, equalize=equalize)
    assert len(outs) == 1 and outs[0].n == len(pc.E2E_SEEDS)
    return outs[0]


def _regions_against(r, res, a, windows_too=True):
    """Per region: the rectangles against the oracle's on the crop; order; the counters as sums over the regions (windows_too: the
    OpenCV profile's visited positions; the clod profile's region passes are compared by the stages entered, as their own tests do)."""
    windows, entered = 0, np.zeros(a.n_stages, np.int64)
    for i, (want, st) in enumerate(res):
        assert cc.rows(r.rects[r.rects["frame"] == i]) == cc.rows(want), f"region {i}"
        windows += st["windows"]
        entered += np.array(st["stage_entered"], np.int64)
    assert len(r.rects) == sum(len(want) for want, _ in res)
    key = [(int(x["frame"]), int(x["scale_idx"]), int(x["y"]), int(x["x"])) for x in r.rects]
    assert key == sorted(key)
    assert r.stage_entered[:a.n_stages] == entered.tolist()
    if windows_too:
        assert r.windows == windows


def test_detect_and_detect_opencv(env, oracle, cascades):
    c, a = cascades(pc.CASC)
    want = pc.e2e_prepared(oracle)
    d = _prepared(env)
    clod = pc.once("clod", lambda: [oracle.detect(a, f) for f in want])
    cv = pc.once("cv", lambda: [oracle.detect_opencvlike(a, f) for f in want])
    r = env.detect(c, d, default_params(flags=CNT))
    _against(r, clod, a)
    assert np.array_equal(env.detect(c, d).rects, r.rects)
    r = env.detect_opencv(c, d, flags=CNT)
    _against(r, cv, a)
    assert np.array_equal(env.detect_opencv(c, d).rects, r.rects)


def test_flag_on_resized_output_equals_equalized_output(env, cascades):
    """VJ_FLAG_EQUALIZE_HIST on un-equalized preprocess(size=...) output is the call without it on preprocess(size=..., equalize=True)."""
    c, a = cascades(pc.CASC)
    plain, eq = _prepared(env, False), _prepared(env, True)
    for call in (lambda d, fl: env.detect(c, d, default_params(flags=CNT | fl)), lambda d, fl: env.detect_opencv(c, d, flags=CNT | fl)):
        x, y = call(plain, VJ_FLAG_EQUALIZE_HIST), call(eq, 0)
        assert np.array_equal(x.rects, y.rects) and len(x.rects) >= 10
        assert x.windows == y.windows and x.stage_entered == y.stage_entered
        assert not np.array_equal(call(plain, 0).rects, y.rects)


@pytest.mark.parametrize("device", [False, True])
def test_detect_opencv_chain(env, oracle, cascades, device):
    """The sample's second half: eyes inside faces, on the equalized image, without leaving the device."""
    c1, a1 = cascades(pc.CASC)
    c2, a2 = cascades("eye")
    want = pc.e2e_prepared(oracle)
    d = _prepared(env)
    flags = CNT | (VJ_FLAG_CV_CHAIN_DEVICE if device else 0)
    r1, r2 = env.detect_opencv_chain(c1, c2, d, min_neighbors=3, flags=flags, flags_second=CNT)
    regions, res = pc.once("cv_chain", lambda: cc.oracle_chain(oracle, a1, a2, want, 3))
    got = np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)
    assert np.array_equal(got, regions) and len(regions) >= 3
    _regions_against(r2, res, a2)
    assert env.cv_chain_info().handoff == (1 if device else 2)


def test_detect_chain(env, oracle, cascades):
    c1, a1 = cascades(pc.CASC)
    c2, a2 = cascades("eye")
    want = pc.e2e_prepared(oracle)
    d = _prepared(env)
    r1, r2 = env.detect_chain(c1, c2, d, default_params(min_neighbors=3), default_params(flags=CNT))
    regions = []
    for f, (raw, _) in enumerate(pc.once("clod", lambda: [oracle.detect(a1, x) for x in want])):
        raw = raw[np.lexsort((raw["x"], raw["y"], raw["scale_idx"]))]
        xywh, _ = oracle.group_rectangles(np.array([[v["x"], v["y"], v["w"], v["h"]] for v in raw], np.int32).reshape(-1, 4), 3)
        regions += [(f, *map(int, q)) for q in xywh]
    got = [(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects]
    assert got == regions and len(regions) >= 3
    res = [oracle.detect(a2, np.ascontiguousarray(cc.crop(want, q))) for q in regions]
    _regions_against(r2, res, a2, windows_too=False)


def test_region_calls(env, oracle, cascades):
    c, a = cascades(pc.CASC)
    want = pc.e2e_prepared(oracle)
    d = _prepared(env)
    rois = np.array([(f, *r) for r in cc.REGIONS for f in range(len(want))], np.int32)      # REGIONS are regions of a 240 x 180 frame
    r = env.detect_opencv_rois(c, d, rois, flags=CNT)
    _regions_against(r, pc.once("cv_rois", lambda: cc.oracle_rois(oracle, a, want, rois)), a)
    assert len(r.rects) >= 10
    r = env.detect_rois(c, d, rois, default_params(flags=CNT))
    _regions_against(r, pc.once("clod_rois", lambda: [oracle.detect(a, np.ascontiguousarray(cc.crop(want, q))) for q in rois]), a, windows_too=False)
    assert len(r.rects) >= 10


def test_window_lists(env, oracle, cascades):
    c, a = cascades(pc.CASC)
    want = pc.e2e_prepared(oracle)
    d = _prepared(env)
    assert (rw.FRAME_W, rw.FRAME_H) == pc.E2E_SIZE == (cw.FRAME_W, cw.FRAME_H)
    w = np.concatenate([rw.full_list(a, frame=f)[:1500] for f in range(len(want))])
    res, sums = run_windows_opencv(d, c, env, w, rw.case_scales())
    want_res, want_sums = rw.run_windows(a, want, w, rw.case_scales())
    assert np.array_equal(res, want_res) and np.array_equal(sums.view(np.uint64), want_sums.view(np.uint64)) and (res == 1).any() and (res <= 0).any()
    w = np.concatenate([cw.full_list(a, frame=f)[:1500] for f in range(len(want))])
    res, sums, var = run_windows(d, c, env, w, cw.case_scales())
    want_res, want_sums, want_var = cw.run_windows(a, want, w, cw.case_scales())
    assert np.array_equal(res, want_res) and (want_res == 1).any() and (want_res <= 0).any()
    assert np.array_equal(sums.view(np.uint32), want_sums.view(np.uint32))
    assert np.array_equal(var.view(np.uint32), want_var.view(np.uint32))


def test_detect_mixed_on_the_eleven_outputs(env, oracle, cascades):
    c, a = cascades(pc.CASC)
    items, keep = _mixed_items()
    want = pc.mixed_prepared(oracle, True)
    outs = env.preprocess(items, fx=0.5, fy=0.5, equalize=True)
    cv = pc.once("mixed_cv", lambda: [oracle.detect_opencvlike(a, f) for f in want])
    clod = pc.once("mixed_clod", lambda: [oracle.detect(a, f) for f in want])
    _against(env.detect_opencv_mixed(c, outs, flags=CNT), cv, a, least=10)
    _against(env.detect_mixed(c, outs, default_params(flags=CNT)), clod, a, least=10)
    assert env.mixed_info().frames == len(mc.SIZES)


# ------------------------------------------------------------------------------------------------------------------ 5. the errors
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
    f = lib.vj_preprocess

    def call(images=ok, n=None, p=None, d=dst.data_ptr(), nbytes=dst.numel(), e=env._h, out=True, **kw):
        q = Prep(0, 0, 0.5, 0.5, VJ_PREP_EQUALIZE, 0) if p is None and not kw else Prep()
        for k, v in kw.items():
            setattr(q, k, v)
        arr = (_Image * max(len(images), 1))(*images)
        res = (_Image * max(len(images), 1))()
        rc = f(e, arr if images is not None else None, len(images) if n is None else n, C.byref(q) if p is None else p,
               C.c_void_p(d), nbytes, res if out else None)
        err = lib.vj_last_error().decode()
        after = env.detect(c, plain)                                              # every error is followed by a plain detect
        assert np.array_equal(after.rects, base.rects)
        return rc, err

    assert call()[0] == 0
    need = env.preprocess_layout([mc.frames()[1], mc.frames()[3]], fx=0.5, fy=0.5)[1]
    # null arguments
    assert call(e=None)[0] == VJ_ERR_ARG and call(out=False)[0] == VJ_ERR_ARG and call(d=None)[0] == VJ_ERR_ARG
    assert f(env._h, None, 2, C.byref(Prep()), C.c_void_p(dst.data_ptr()), dst.numel(), (_Image * 2)()) == VJ_ERR_ARG
    assert f(env._h, (_Image * 2)(*ok), 2, None, C.c_void_p(dst.data_ptr()), dst.numel(), (_Image * 2)()) == VJ_ERR_ARG
    assert call(n=-1)[0] == VJ_ERR_ARG
    # bad frames
    for bad in (_Image(None, 8, 4, 8, 1, 1), _Image(src.data_ptr(), 0, 4, 8, 1, 1), _Image(src.data_ptr(), 8, 4, 7, 1, 1), _Image(src.data_ptr(), 8, 4, 16, 1, 2)):
        rc, err = call(images=ok + [bad])
        assert rc == VJ_ERR_ARG and "frame 2" in err
    # the fields of vj_prep
    for kw, word in [(dict(dst_w=5), "dst_w"), (dict(dst_h=5), "dst_h"), (dict(fx=0.5), "fx"), (dict(fy=0.5), "fy"), (dict(fx=-1.0, fy=-1.0), "fx"),
                     (dict(fx=float("inf"), fy=1.0), "fx"), (dict(fx=1.0, fy=float("nan")), "fy"), (dict(flags=2), "flags"), (dict(reserved=7), "reserved")]:
        rc, err = call(**kw)
        assert rc == VJ_ERR_ARG and word in err, kw
    # the limit
    rc, err = call(dst_w=65536, dst_h=2)
    assert rc == VJ_ERR_LIMIT and "65535" in err
    # dst_bytes too small, by one byte
    rc, err = call(nbytes=need - 1)
    assert rc == VJ_ERR_ARG and "dst_bytes" in err
    assert call(nbytes=need)[0] == 0
    # a device-resident source that overlaps the destination: its first byte, its last byte, and one byte past each end
    end = src.data_ptr() + h * w
    for d0, overlaps in [(src.data_ptr() - need + 4, True), (src.data_ptr() - (need + 3) // 4 * 4, False), (end - 4, True)]:
        if d0 % 4:
            d0 -= d0 % 4
        if not overlaps:
            continue                                                              # (memory next to the source is not ours to write)
        rc, err = call(d=d0, nbytes=need)
        assert rc == VJ_ERR_ARG and "frame 0" in err and "overlaps" in err
    same = torch.from_numpy(np.array(plain)).cuda()                               # 240 x 180: the output needs exactly the source's bytes
    with pytest.raises(VjError) as ei:
        env.preprocess(DeviceFrames.from_torch(same[None]), equalize=True, out=same.reshape(-1))   # in place is refused
    assert ei.value.code == VJ_ERR_ARG and "overlaps" in str(ei.value)
    assert np.array_equal(same.cpu().numpy(), plain)                             # nothing was written
    # zero frames
    assert f(env._h, None, 0, C.byref(Prep()), None, 0, None) == 0
    # and the environment still preprocesses
    check(env, oracle, [mc.frames()[1], mc.frames()[3]], fx=0.5, fy=0.5, equalize=True)
