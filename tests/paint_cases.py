"""The numpy restatement of vj_paint (include/vj.h) and the cases tests/test_paint_cpu.py — which checks the layout
through ctypes and states the premises of the GPU tests with the restatement alone — and tests/test_gpu_paint.py share.

All arithmetic is on integers.  The mapping is extract_cases.map_region (prep_cases.cv_round); everything else is restated here:
the size, the shape, the painted set, the value of every mode and the overlap rule.  The variants (`winner`, `sequential`,
`truncate`, `clamp`) are deliberately WRONG readings of the definition: the CPU premises show that the chosen cases tell them apart."""
from __future__ import annotations

import os
import re

import numpy as np

import extract_cases as ec
import prep_cases as pc

FILL, OUTLINE, PIXELATE, BLUR = 0, 1, 2, 3
MODES = {"fill": FILL, "outline": OUTLINE, "pixelate": PIXELATE, "blur": BLUR}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def units_header() -> dict:
    """The block, band and limit sizes csrc/vj_paint_units.hpp names."""
    text = open(os.path.join(ROOT, "clfacedetection_amd", "csrc", "vj_paint_units.hpp")).read()
    out = {}
    for name in ("PAINT_BLOCK_SLOTS", "PAINT_BLOCK_H", "PAINT_WAVES", "PAINT_BAND_H", "PAINT_BAND_COLS", "PAINT_MAX_SIDE", "PAINT_MAX_KK",
                 "PAINT_MAX_CELL"):
        out[name] = int(re.search(r"\b%s = (\d+)" % name, text).group(1))
    return out


def size_of(mode: int, wm: int, hm: int, size: int, rel: float) -> int:
    """t (OUTLINE), s (PIXELATE), kk (BLUR), 0 (FILL)."""
    if mode == FILL:
        return 0
    v = min(wm, hm) * float(rel)
    s = int(size) if size > 0 else (max(pc.cv_round(v), 1) if v <= 65536.0 else 65536)
    return max(s | 1, 3) if mode == BLUR else s


def clip(m, fw: int, fh: int):
    """K of the mapped rectangle (x, y, w, h) in a fw x fh frame -> (cx0, cy0, cx1, cy1), or None when it is empty."""
    x, y, w, h = m
    cx0, cy0, cx1, cy1 = max(x, 0), max(y, 0), min(x + w, fw), min(y + h, fh)
    return (cx0, cy0, cx1, cy1) if cx1 > cx0 and cy1 > cy0 else None


def in_shape(px, py, x0: int, y0: int, w: int, h: int, ellipse: bool):
    """px, py: int64 arrays that broadcast.  Sides up to 32767: the products stay below 2^60."""
    dx, dy = px - x0, py - y0
    inside = (dx >= 0) & (dy >= 0) & (dx < w) & (dy < h)
    if not ellipse:
        return inside & np.ones(np.broadcast(px, py).shape, bool)
    a, b = np.where(inside, 2 * dx + 1 - w, 0), np.where(inside, 2 * dy + 1 - h, 0)
    return inside & (a * a * (h * h) + b * b * (w * w) <= (w * w) * (h * h))


def painted(mode: int, m, k, s: int, ellipse: bool) -> np.ndarray:
    """The painted set of a region as a bool array over K's pixels."""
    x0, y0, w, h = m
    cx0, cy0, cx1, cy1 = k
    px, py = np.arange(cx0, cx1, dtype=np.int64)[None, :], np.arange(cy0, cy1, dtype=np.int64)[:, None]
    sh = in_shape(px, py, x0, y0, w, h, ellipse)
    if mode == OUTLINE and w - 2 * s > 0 and h - 2 * s > 0:
        sh &= ~in_shape(px, py, x0 + s, y0 + s, w - 2 * s, h - 2 * s, ellipse)
    return sh


def _box_sums(crop: np.ndarray, r: int) -> np.ndarray:
    """Sum over dy, dx in -r .. r of crop with its border replicated; crop (h, w, C) int64."""
    p = np.pad(crop, ((r, r), (r, r), (0, 0)), mode="edge")
    c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0), (0, 0))), axis=0), axis=1)
    kk = 2 * r + 1
    return c[kk:, kk:] - c[:-kk, kk:] - c[kk:, :-kk] + c[:-kk, :-kk]


def values(mode: int, F: np.ndarray, k, s: int, fill, truncate: bool = False, clamp: str = "K") -> np.ndarray:
    """The value of every pixel of K, (kh, kw, C) uint8, from the frame F (H, W, C)."""
    cx0, cy0, cx1, cy1 = k
    kh, kw, C = cy1 - cy0, cx1 - cx0, F.shape[2]
    if mode in (FILL, OUTLINE):
        return np.broadcast_to(np.array([fill[c] for c in range(C)], np.uint8), (kh, kw, C)).copy()
    crop = F[cy0:cy1, cx0:cx1].astype(np.int64)
    if mode == PIXELATE:
        ys, xs = np.arange(0, kh, s), np.arange(0, kw, s)                      # the cells' first rows and columns, anchored at K's corner
        sums = np.add.reduceat(np.add.reduceat(crop, ys, axis=0), xs, axis=1)
        n = (np.minimum(ys + s, kh) - ys)[:, None, None] * (np.minimum(xs + s, kw) - xs)[None, :, None]
        mean = (sums + (0 if truncate else n // 2)) // n
        return np.repeat(np.repeat(mean, s, axis=0), s, axis=1)[:kh, :kw].astype(np.uint8)
    r = s >> 1
    if clamp == "K":
        sums = _box_sums(crop, r)
    else:   # the wrong reading: the border replicated at the FRAME's edge, so a region reads its neighbours' pixels
        ys = np.clip(np.arange(cy0 - r, cy1 + r), 0, F.shape[0] - 1)
        xs = np.clip(np.arange(cx0 - r, cx1 + r), 0, F.shape[1] - 1)
        wide = F[np.ix_(ys, xs)].astype(np.int64)
        c = np.cumsum(np.cumsum(np.pad(wide, ((1, 0), (1, 0), (0, 0))), axis=0), axis=1)
        kk = 2 * r + 1
        sums = c[kk:, kk:] - c[:-kk, kk:] - c[kk:, :-kk] + c[:-kk, :-kk]
    return ((sums + (0 if truncate else (s * s) // 2)) // (s * s)).astype(np.uint8)


def _as3(f: np.ndarray) -> np.ndarray:
    return f[:, :, None] if f.ndim == 2 else f


def restate(frames, rects, mode, size=0, rel=0.25, scale=(1.0, 1.0), margin=0.0, ellipse=False, fill=(0, 0, 0, 0),
            winner="last", sequential=False, truncate=False, clamp="K") -> list:
    """What vj_paint must leave in the frames: new arrays of the frames' shapes.  frames: a list of (H, W) or (H, W, 3 | 4) uint8
    arrays; rects: rows of (frame, x, y, w, h); mode: a name or a number."""
    mode = MODES.get(mode, mode)
    fill = tuple(fill) + (0,) * (4 - len(tuple(fill)))
    orig = [_as3(np.asarray(f)).copy() for f in frames]
    out = [f.copy() for f in orig]
    rows = ec.as_rows(rects)
    for r in (rows if winner == "last" else rows[::-1]):
        f, x, y, w, h = ec.map_region(r, scale, margin)
        k = clip((x, y, w, h), orig[f].shape[1], orig[f].shape[0])
        if k is None:
            continue
        s = size_of(mode, w, h, size, rel)
        mask = painted(mode, (x, y, w, h), k, s, ellipse)
        val = values(mode, out[f] if sequential else orig[f], k, s, fill, truncate, clamp)
        view = out[f][k[1]:k[3], k[0]:k[2]]
        view[mask] = val[mask]
    return [o.reshape(np.asarray(f).shape) for o, f in zip(out, frames)]


_ONCE = {}


def once_restate(key, build):
    """A restatement several tests share: computed once; do not modify."""
    if key not in _ONCE:
        _ONCE[key] = build()
    return _ONCE[key]


def layout(frames, rects, mode, size=0, rel=0.25, scale=(1.0, 1.0), margin=0.0):
    """What vj_paint_layout must report: ((n, 5) rows of K, w = h = 0 when empty; (n,) sizes; scratch bytes)."""
    mode = MODES.get(mode, mode)
    rows = ec.as_rows(rects)
    ks, sizes, scratch = [], [], 0
    for r in rows:
        f, x, y, w, h = ec.map_region(r, scale, margin)
        fr = np.asarray(frames[f])
        C = 1 if fr.ndim == 2 else fr.shape[2]
        k = clip((x, y, w, h), fr.shape[1], fr.shape[0])
        s = size_of(mode, w, h, size, rel)
        sizes.append(s)
        if k is None:
            ks.append((f, 0, 0, 0, 0))
            continue
        kw, kh = k[2] - k[0], k[3] - k[1]
        ks.append((f, k[0], k[1], kw, kh))
        if mode == BLUR:
            scratch += (2 * kh * kw * C + 15) // 16 * 16
        elif mode == PIXELATE:
            scratch += (-(-kw // s) * -(-kh // s) * C + 15) // 16 * 16
    return np.array(ks, np.int32).reshape(-1, 5), np.array(sizes, np.int32), scratch


# ---- the shared cases
W, H = 37, 29


def sources(seed: int) -> list:
    """Random 37 x 29 frames: gray, BGR, BGRA."""
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, (H, W, ch) if ch > 1 else (H, W), dtype=np.uint8) for ch in (1, 3, 4)]


def wide_frame(seed: int = 5) -> np.ndarray:
    """One 300 x 40 BGR frame: rows of 900 bytes, more than one block of slots and of byte columns."""
    return np.random.default_rng(seed).integers(1, 256, (40, 300, 3), dtype=np.uint8)


# regions of the 37 x 29 frames: 1 x 1, 1 x n, n x 1, each side, each corner, partly and wholly outside, the whole frame
SMALL_RECTS = [(0, 3, 4, 1, 1), (0, 20, 2, 1, 9), (0, 9, 20, 11, 1),
               (0, -5, 8, 10, 10), (0, 30, 8, 10, 10), (0, 8, -5, 10, 10), (0, 8, 25, 10, 10),
               (0, -3, -3, 10, 10), (0, 30, -3, 10, 10), (0, -3, 22, 10, 10), (0, 30, 22, 10, 10),
               (0, 100, 100, 6, 6), (0, -40, 3, 6, 6), (0, 5, -30, 6, 6), (0, 12, 9, 14, 12)]
WHOLE = [(0, 0, 0, W, H)]
FILL_COLOR = (17, 201, 94, 250)

# the overlap case: three regions of differing sizes on one frame, the middle one covering part of both others
OVERLAP_RECTS = [(0, 2, 2, 20, 16), (0, 10, 8, 22, 18), (0, 6, 12, 12, 9)]
# the rounding case: values whose cell and window sums leave remainders of at least half the divisor somewhere
ROUNDING_RECT = [(0, 4, 3, 21, 15)]

# pixels of the ellipse inscribed in w x h, counted by hand from (2 dx + 1 - w)^2 h^2 + (2 dy + 1 - h)^2 w^2 <= w^2 h^2:
#   1 x n, n x 1: a = 0 (or b = 0) and the other term is at most its bound: every pixel.
#   2 x 2: (1 + 1) * 4 = 8 <= 16: all 4.          3 x 3: the corners (4 + 4) * 9 = 72 <= 81: all 9.
#   4 x 4: the corners (9 + 9) * 16 = 288 > 256 are out: 12.
#   5 x 5: the corners (16 + 16) * 25 = 800 > 625 are out, their neighbours (16 + 4) * 25 = 500 are in: 21.
#   6 x 4: rows 0, 3: b^2 = 9, 16 a^2 <= 576 - 324 -> a^2 <= 15, a in {-3, -1, 1, 3}: 4; rows 1, 2: b^2 = 1, a^2 <= 33: all 6 -> 20.
#   7 x 3: rows 0, 2: b^2 = 4, 9 a^2 <= 441 - 196 -> a^2 <= 27, a in {-4 .. 4} even: 5; row 1: all 7 -> 17.
ELLIPSE_COUNTS = {(1, 1): 1, (1, 7): 7, (7, 1): 7, (2, 2): 4, (3, 3): 9, (4, 4): 12, (5, 5): 21, (6, 4): 20, (7, 3): 17}
