"""The numpy restatement of vj_yuv_to_bgr / vj_bgr_to_yuv (include/vj.h) and the cases tests/test_yuv_cpu.py and
tests/test_gpu_yuv.py share.  Everything is int32 exactly as the definition is written: >> on numpy's signed integers is the
arithmetic (flooring) shift.  Parity with OpenCV is unpinned (OpenCV is not available to the tests); this file is the oracle.

Planes: `y` (h, w); NV12 / NV21: `uv` (h / 2, w) of U, V / V, U byte pairs; I420: `u`, `v` (h / 2, w / 2).  A frame travels as the
tuple of its planes.  The deliberately wrong variants exist so that the CPU test can show that the cases tell them from the right one."""
from __future__ import annotations

import numpy as np

NV12, NV21, I420 = 0, 1, 2
LAYOUT_NAMES = {NV12: "nv12", NV21: "nv21", I420: "i420"}
H = 1 << 19

# (Y, U, V) -> (B, G, R) and (B, G, R) -> (Y, U, V): the known answers of the definition
DECODE_KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((255, 128, 128), (255, 255, 255)), ((0, 0, 0), (0, 154, 0)),
                ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)), ((255, 255, 255), (255, 125, 255)),
                ((128, 0, 255), (0, 77, 255))]
ENCODE_KNOWN = [((0, 0, 0), (16, 128, 128)), ((255, 255, 255), (235, 128, 128)), ((0, 0, 255), (82, 90, 240)), ((0, 255, 0), (145, 54, 34)),
                ((255, 0, 0), (41, 240, 110)), ((1, 2, 3), (18, 127, 129))]

# the lane and wave widths of csrc/vj_yuv_units.hpp (the CPU test reads them from the header and compares)
LANE_W, BLOCK_W, BLOCK_H = 4, 256, 32
WIDTHS = [2, 4, 6, 8, 62, 64, 66, 254, 256, 258, 510, 514]
HEIGHTS = [2, 4, 6, 30, 32, 34, 62, 64, 66]
# eleven frames of differing even sizes
MIXED_SIZES = [(240, 180), (130, 98), (142, 110), (210, 62), (66, 170), (30, 28), (154, 134), (88, 88), (2, 2), (258, 6), (126, 102)]


def _sat(t):
    return np.clip(t, 0, 255)


# ------------------------------------------------------------------------------------------------------------------- pixels
def decode_px(Y, U, V, floor=True, clamp_y=True):
    """(Y, U, V) int arrays -> (B, G, R) int32 arrays.  floor=False: truncating division; clamp_y=False: no max(Y - 16, 0)."""
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    yy = (np.maximum(Y - 16, 0) if clamp_y else Y - 16) * np.int32(1220542)
    u, v = U - 128, V - 128
    tb, tg, tr = yy + H + 2116026 * u, yy + H - 852492 * v - 409993 * u, yy + H + 1673527 * v
    if floor:
        sh = lambda t: t >> 20
    else:
        sh = lambda t: (np.sign(t) * (np.abs(t) >> 20)).astype(np.int32)
    return _sat(sh(tb)), _sat(sh(tg)), _sat(sh(tr))


def encode_px(B, G, R):
    """(B, G, R) int arrays -> (Y, U, V) int32 arrays, unclamped."""
    B, G, R = (np.asarray(a).astype(np.int32) for a in (B, G, R))
    Y = (269484 * R + 528482 * G + 102760 * B + H + (16 << 20)) >> 20
    U = (-155188 * R - 305135 * G + 460324 * B + H + (128 << 20)) >> 20
    V = (460324 * R - 385875 * G - 74448 * B + H + (128 << 20)) >> 20
    return Y, U, V


# ------------------------------------------------------------------------------------------------------------------- frames
def split_chroma(planes, layout):
    """-> (y, u, v), u and v (h / 2, w / 2)"""
    if layout == I420:
        return planes
    y, uv = planes
    a, b = uv[:, 0::2], uv[:, 1::2]
    return (y, a, b) if layout == NV12 else (y, b, a)


def join_chroma(y, u, v, layout):
    if layout == I420:
        return y, u, v
    uv = np.empty((u.shape[0], u.shape[1] * 2), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = (u, v) if layout == NV12 else (v, u)
    return y, uv


def decode(planes, layout, channels=3, rgb=False, variant=None):
    """The BGR / BGRA (rgb: RGB / RGBA) image (h, w, channels) of a frame.  variant: None, "trunc" (truncating division),
    "swap_uv" (U and V exchanged), "no_clamp" (no max(Y - 16, 0))."""
    y, u, v = split_chroma(planes, layout)
    if variant == "swap_uv":
        u, v = v, u
    U, V = (np.repeat(np.repeat(c, 2, axis=0), 2, axis=1) for c in (u, v))     # chroma sample (x >> 1, y >> 1)
    b, g, r = decode_px(y, U, V, floor=variant != "trunc", clamp_y=variant != "no_clamp")
    out = np.full(y.shape + (channels,), 255, np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = (r, g, b) if rgb else (b, g, r)
    return out


def encode(img, layout, rgb=False, variant=None):
    """The planes of a BGR / BGRA image (h, w, 3 | 4), h and w even.  variant: None, "average" (chroma averaged over the 2 x 2 block),
    "bottom_right" (chroma from the block's bottom-right pixel), "swap_uv"."""
    c0, g, c2 = (img[..., k].astype(np.int32) for k in range(3))
    b, r = (c2, c0) if rgb else (c0, c2)
    Y, U, V = encode_px(b, g, r)
    if variant == "average":
        U, V = ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (U, V))
    elif variant == "bottom_right":
        U, V = U[1::2, 1::2], V[1::2, 1::2]
    else:
        U, V = U[0::2, 0::2], V[0::2, 0::2]
    if variant == "swap_uv":
        U, V = V, U
    assert Y.min() >= 0 and Y.max() <= 255 and min(U.min(), V.min()) >= 0 and max(U.max(), V.max()) <= 255
    return join_chroma(Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8), layout)


# ------------------------------------------------------------------------------------------------------------------- buffers
def align(v, a):
    return (v + a - 1) // a * a


def stacked(planes, layout):
    """The (h * 3 // 2, w) array OpenCV and the decoders hand out."""
    y = planes[0]
    h, w = y.shape
    out = np.empty((h * 3 // 2, w), np.uint8)
    out[:h] = y
    out[h:].reshape(-1)[:] = np.concatenate([p.reshape(-1) for p in planes[1:]])
    return out


def unstack(a, layout):
    h, w = a.shape[0] * 2 // 3, a.shape[1]
    y, rest = a[:h], a[h:].reshape(-1)
    if layout == I420:
        q = (w // 2) * (h // 2)
        return y, rest[:q].reshape(h // 2, w // 2), rest[q:].reshape(h // 2, w // 2)
    return y, rest.reshape(h // 2, w)


def decode_buffer(frames, layout, channels, rgb, total, sentinel):
    """The whole destination buffer of yuv_to_bgr(frames): images at multiples of 256, rows at align4(w * channels) with the pad
    bytes 0, everything else — the gaps between images and the margin up to `total` — the sentinel.  layout: one, or one per frame."""
    buf = np.full(total, sentinel, np.uint8)
    layouts = layout if isinstance(layout, (list, tuple)) else [layout] * len(frames)
    off, recs = 0, []
    for planes, lay in zip(frames, layouts):
        img = decode(planes, lay, channels, rgb)
        h, w = img.shape[:2]
        pitch = align(w * channels, 4)
        off = align(off, 256)
        rows = np.zeros((h, pitch), np.uint8)
        rows[:, :w * channels] = img.reshape(h, w * channels)
        buf[off:off + h * pitch] = rows.reshape(-1)
        recs.append((off, w, h, pitch))
        off += h * pitch
    return buf, recs, off


def encode_buffer(images, layout, rgb, total, sentinel):
    """The whole destination buffer of bgr_to_yuv(images): stacked frames at multiples of 256, the Y plane at align4(w), the pair
    plane at align4(w) or the U and V planes at align4(w / 2), pad bytes 0, everything else the sentinel."""
    buf = np.full(total, sentinel, np.uint8)
    off, recs = 0, []
    for img in images:
        planes = encode(img, layout, rgb)
        off = align(off, 256)
        at, offs = off, []
        for p in planes:
            pitch = align(p.shape[1], 4)
            rows = np.zeros((p.shape[0], pitch), np.uint8)
            rows[:, :p.shape[1]] = p
            buf[at:at + rows.size] = rows.reshape(-1)
            offs.append(at)
            at += rows.size
        recs.append(tuple(offs))
        off = at
    return buf, recs, off


# ------------------------------------------------------------------------------------------------------------------- cases
def random_frame(w, h, layout, seed):
    """Full-range random planes."""
    rng = np.random.default_rng(seed * 7919 + w * 131 + h)
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
    return join_chroma(y, u, v, layout)


def random_image(w, h, channels, seed):
    return np.random.default_rng(seed * 104729 + w * 131 + h + channels).integers(0, 256, (h, w, channels), dtype=np.uint8)


def exhaustive_frames(layout):
    """Every term of the decoder: all (Y, U) with V in {0, 127, 128, 129, 255} and all (Y, V) with U in the same set — 10 frames of
    256 x 256 = 655 360 pixels.  A frame's 128 x 128 chroma samples run through the swept chroma value c = 0 .. 255, 64 samples each,
    and the 2 x 2 block of sample k of a value holds the four DIFFERENT luma values 4 k .. 4 k + 3: over its 64 samples a chroma
    value meets all 256 Y."""
    frames = []
    idx = np.arange(128 * 128).reshape(128, 128)
    c = (idx // 64).astype(np.uint8)                       # 0 .. 255, 64 samples each
    k = idx % 64                                           # which quarter of the Y range a sample's block holds
    y = np.empty((256, 256), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[dy::2, dx::2] = (4 * k + 2 * dy + dx).astype(np.uint8)
    for fixed in (0, 127, 128, 129, 255):
        other = np.full((128, 128), fixed, np.uint8)
        frames.append(join_chroma(y.copy(), c.copy(), other.copy(), layout))       # all (Y, U), V fixed
        frames.append(join_chroma(y.copy(), other.copy(), c.copy(), layout))       # all (Y, V), U fixed
    return frames


def encode_images(channels):
    """What the encoder's tests sweep beyond random frames: the cube's corners, gray ramps, per-channel ramps with the others at 0 and
    at 255, and frames whose odd rows and odd columns differ wildly from the even ones."""
    out = []
    corners = np.array([[(i & 1) * 255, (i >> 1 & 1) * 255, (i >> 2 & 1) * 255] for i in range(8)], np.uint8)
    img = np.repeat(np.repeat(corners.reshape(2, 4, 3), 2, axis=0), 2, axis=1)      # 4 x 8, every corner a whole 2 x 2 block
    out.append(img)
    ramp = np.arange(256, dtype=np.uint8)
    gray = np.repeat(ramp[None, :, None], 3, axis=2).repeat(2, axis=0)              # 2 x 256
    out.append(gray)
    for ch in range(3):
        for base in (0, 255):
            im = np.full((2, 256, 3), base, np.uint8)
            im[:, :, ch] = ramp
            out.append(im)
    out.append(wild_image(66, 6, 5))
    if channels == 4:
        rng = np.random.default_rng(99)
        out = [np.concatenate([im, rng.integers(0, 256, im.shape[:2] + (1,), dtype=np.uint8)], axis=2) for im in out]
    return out


def wild_image(w, h, seed):
    """Even rows and columns random; odd rows and odd columns their complement, roughly: where the chroma-sampling variants differ."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[1::2] = 255 - img[0::2]
    img[:, 1::2] = img[:, 0::2][..., ::-1] // 2 + 64
    return img
