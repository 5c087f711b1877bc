"""Cases of vj_extract, shared by tests/test_extract_cpu.py — which checks the mapping and the layout through ctypes
and states the premises of the GPU tests on the CPU with the restatements alone — and tests/test_gpu_extract.py, which runs them on
the device.

The reference of every byte is a composition of the existing restatements, nothing new: the crop padded by clamping its indices to
the frame, then scale_image_oracle.resize_linear per channel — with oracle.bgr2gray of the padded crop first for gray=True (the
conversion is per pixel, so converting the frame and cropping is the same).  The mapping is restated with prep_cases.cv_round."""
from __future__ import annotations

import numpy as np

import prep_cases as pc
import scale_image_oracle as so


def map_region(rect, scale=(1.0, 1.0), margin=0.0):
    """(frame, x, y, w, h) -> the source region (frame, x, y, w, h), as OpenCV's facedetect sample maps its boxes, plus the margin."""
    f, x, y, w, h = (int(v) for v in rect)
    sx, sy = (float(s) or 1.0 for s in scale)
    x0, y0 = pc.cv_round(x * sx), pc.cv_round(y * sy)
    w0, h0 = max(pc.cv_round(w * sx), 1), max(pc.cv_round(h * sy), 1)
    mx, my = pc.cv_round(w0 * margin), pc.cv_round(h0 * margin)
    return f, x0 - mx, y0 - my, w0 + 2 * mx, h0 + 2 * my


def padded_crop(img: np.ndarray, x, y, w, h) -> np.ndarray:
    """crop[i][j] = img[clamp(y + i, 0, H - 1)][clamp(x + j, 0, W - 1)]: the region with the frame's border replicated."""
    ys = np.clip(np.arange(y, y + h), 0, img.shape[0] - 1)
    xs = np.clip(np.arange(x, x + w), 0, img.shape[1] - 1)
    return np.ascontiguousarray(img[np.ix_(ys, xs)])


def restate(oracle, frames, rects, size, scale=(1.0, 1.0), margin=0.0, gray=False, planar=False) -> np.ndarray:
    """What vj_extract must write: (n, h, w, C) uint8, or (n, C, h, w) with planar=True.  frames: a list of (H, W) or (H, W, 3 | 4)
    arrays; rects: rows of (frame, x, y, w, h)."""
    rows = as_rows(rects)
    ow, oh = int(size[0]), int(size[1])
    outs = []
    for r in rows:
        f, x, y, w, h = map_region(r, scale, margin)
        crop = padded_crop(np.asarray(frames[f]), x, y, w, h)
        if gray and crop.ndim == 3:
            crop = oracle.bgr2gray(np.ascontiguousarray(crop))
        if crop.ndim == 2:
            crop = crop[:, :, None]
        outs.append(np.stack([so.resize_linear(np.ascontiguousarray(crop[:, :, c]), ow, oh) for c in range(crop.shape[2])], axis=2))
    ch = outs[0].shape[2] if outs else 1
    out = np.stack(outs) if outs else np.zeros((0, oh, ow, ch), np.uint8)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if planar else out


def as_rows(rects) -> np.ndarray:
    """(n, 5) int32 rows of (frame, x, y, w, h) from rows or from a RECT_DTYPE array."""
    r = np.asarray(rects)
    if r.dtype.names is not None:
        return np.stack([r[k].astype(np.int32) for k in ("frame", "x", "y", "w", "h")], axis=1).reshape(-1, 5)
    return r.astype(np.int32).reshape(-1, 5)


# ---- the crop-edge case: a 20 x 17 crop in the middle of a 37 x 29 frame whose pixels right outside the crop differ strongly from
# the ones inside, taken up to 64 x 34 (factors 3.2 and 2): the first and last taps of both axes reach past the crop unless they
# clamp at it
EDGE_FRAME_W, EDGE_FRAME_H = 37, 29
EDGE_RECT = (0, 8, 6, 20, 17)
EDGE_SIZE = (64, 34)


def edge_frame(ch: int = 3) -> np.ndarray:
    """Values up to 60 inside EDGE_RECT, from 200 outside it."""
    rng = np.random.default_rng(41)
    shape = (EDGE_FRAME_H, EDGE_FRAME_W, ch) if ch > 1 else (EDGE_FRAME_H, EDGE_FRAME_W)
    f = rng.integers(200, 256, shape, dtype=np.uint8)
    _, x, y, w, h = EDGE_RECT
    f[y:y + h, x:x + w] = rng.integers(1, 61, f[y:y + h, x:x + w].shape, dtype=np.uint8)
    return f


# ---- many regions: every raw candidate of the OpenCV profile on the end-to-end frames of tests/prep_cases.py, prepared to 240 x 180,
# cut from the 432 x 324 colour sources (factor 1.8) to 24 x 24.  The sources are colour versions of those frames whose gray image is
# the frame itself, byte for byte: B = g + 5, G = g, R = g - 2 where 2 <= g <= 250 ((1868 * 5 - 4899 * 2 + 8192) >> 14 = 0), else
# B = G = R = g — preprocessing them gives what preprocessing the gray frames gives, so the CPU premise speaks of the same candidates.
MANY_SCALE = (pc.E2E_SRC_W / pc.E2E_SIZE[0], pc.E2E_SRC_H / pc.E2E_SIZE[1])
MANY_SIZE = (24, 24)
_BGR = None


def e2e_bgr() -> np.ndarray:
    """(3, 324, 432, 3); built once; do not modify."""
    global _BGR
    if _BGR is None:
        g = pc.e2e_frames().astype(np.int16)
        mid = (g >= 2) & (g <= 250)
        _BGR = np.stack([g + 5 * mid, g, g - 2 * mid], axis=-1).astype(np.uint8)
        _BGR.setflags(write=False)
    return _BGR
