"""The numpy restatement of vj_paint_yuv (include/vj.h) and the cases tests/test_paint_yuv_cpu.py and
tests/test_gpu_paint_yuv.py share.

A frame travels as the tuple of its planes, as in tests/yuv_cases.py.  The LUMA part is paint_cases.restate on the Y plane with
fill = Yc: that ties the definition to vj_paint's.  The CHROMA part is restated here: Kc, the any-of-four set, the halved sizes, the
values and the overlap rule.  The variants are deliberately WRONG readings; the CPU premises show that the cases tell them apart:
  "top_left"    the chroma set taken from the top-left luma pixel of each 2 x 2 block only
  "luma_sizes"  chroma painted with the luma sizes (s, kk not halved)
  "k_lists"     overlap decided on K instead of Kc: of two regions with disjoint K that share a chroma sample the EARLIER one keeps it
  "sequential"  every region reads what the regions before it wrote
  "frame_clamp" BLUR's border replicated at the plane's edge instead of Kc's
  "swap_uv"     Uc and Vc exchanged
  "truncate"    no + n / 2 before the divisions"""
from __future__ import annotations

import os
import re

import numpy as np

import extract_cases as ec
import paint_cases as pcs
import yuv_cases as yc

FILL, OUTLINE, PIXELATE, BLUR = pcs.FILL, pcs.OUTLINE, pcs.PIXELATE, pcs.BLUR
MODES = pcs.MODES
VARIANTS = ["top_left", "luma_sizes", "k_lists", "sequential", "frame_clamp", "swap_uv", "truncate"]
LAYOUTS = [yc.NV12, yc.NV21, yc.I420]


def units_header() -> dict:
    """The block and band sizes the kernels of vj_paint_yuv use: vj_paint's, and the prefix bound of its own header."""
    out = pcs.units_header()
    text = open(os.path.join(pcs.ROOT, "clfacedetection_amd", "csrc", "vj_paint_yuv_units.hpp")).read()
    out["PAINT_YUV_PREFIX_MAX"] = int(re.search(r"\bPAINT_YUV_PREFIX_MAX = (\d+)", text).group(1))
    return out


def color_of(fill):
    """(B, G, R) -> (Yc, Uc, Vc) by §4.21's encode formulas."""
    b, g, r = (tuple(fill) + (0, 0, 0))[:3]
    y, u, v = yc.encode_px(b, g, r)
    return int(y), int(u), int(v)


def chroma_size(mode: int, s: int) -> int:
    if mode == PIXELATE:
        return (s + 1) >> 1
    if mode == BLUR:
        return max((s >> 1) | 1, 3)
    return s


def chroma_rect(k):
    """Kc of K = (cx0, cy0, cx1, cy1)."""
    return k[0] >> 1, k[1] >> 1, (k[2] + 1) >> 1, (k[3] + 1) >> 1


def luma_mask(mode, m, k, s, ellipse, fw, fh) -> np.ndarray:
    """P_k as a bool array over the whole (fh, fw) frame."""
    full = np.zeros((fh, fw), bool)
    full[k[1]:k[3], k[0]:k[2]] = pcs.painted(mode, m, k, s, ellipse)
    return full


def chroma_mask(full: np.ndarray, top_left: bool = False) -> np.ndarray:
    """Pc_k over the whole (fh / 2, fw / 2) chroma image: any of the four luma pixels."""
    if top_left:
        return full[0::2, 0::2].copy()
    return full[0::2, 0::2] | full[0::2, 1::2] | full[1::2, 0::2] | full[1::2, 1::2]


def chroma_values(mode: int, F: np.ndarray, kc, cs: int, uv, truncate=False, frame_clamp=False) -> np.ndarray:
    """The value of every sample of Kc, (kh, kw, 2) uint8, from the chroma image F (h / 2, w / 2, 2)."""
    x0, y0, x1, y1 = kc
    kh, kw = y1 - y0, x1 - x0
    if mode in (FILL, OUTLINE):
        return np.broadcast_to(np.array(uv, np.uint8), (kh, kw, 2)).copy()
    crop = F[y0:y1, x0:x1].astype(np.int64)
    out = np.empty((kh, kw, 2), np.uint8)
    if mode == PIXELATE:
        for j in range(0, kh, cs):
            for i in range(0, kw, cs):
                cell = crop[j:j + cs, i:i + cs]
                n = cell.shape[0] * cell.shape[1]
                out[j:j + cs, i:i + cs] = (cell.sum(axis=(0, 1)) + (0 if truncate else n // 2)) // n
        return out
    r = cs >> 1
    if frame_clamp:
        ys, xs = np.clip(np.arange(y0 - r, y1 + r), 0, F.shape[0] - 1), np.clip(np.arange(x0 - r, x1 + r), 0, F.shape[1] - 1)
        wide = F[np.ix_(ys, xs)].astype(np.int64)
    else:
        ys, xs = np.clip(np.arange(-r, kh + r), 0, kh - 1), np.clip(np.arange(-r, kw + r), 0, kw - 1)
        wide = crop[np.ix_(ys, xs)]
    c = np.zeros((wide.shape[0] + 1, wide.shape[1] + 1, 2), np.int64)
    c[1:, 1:] = wide.cumsum(axis=0).cumsum(axis=1)
    sums = c[cs:, cs:] - c[:-cs, cs:] - c[cs:, :-cs] + c[:-cs, :-cs]
    return ((sums + (0 if truncate else (cs * cs) // 2)) // (cs * cs)).astype(np.uint8)


def restate(frames, layouts, rects, mode, size=0, rel=0.25, scale=(1.0, 1.0), margin=0.0, ellipse=False, fill=(0, 0, 0), variant=None) -> list:
    """What vj_paint_yuv must leave in the frames: new plane tuples.  frames: tuples of planes; layouts: one, or one per frame."""
    mode = MODES.get(mode, mode)
    lays = list(layouts) if isinstance(layouts, (list, tuple)) else [layouts] * len(frames)
    Yc, Uc, Vc = color_of(fill)
    if variant == "swap_uv":
        Uc, Vc = Vc, Uc
    ys = pcs.restate([f[0] for f in frames], rects, mode, size, rel, scale, margin, ellipse, (Yc,), sequential=variant == "sequential",
                     truncate=variant == "truncate", clamp="frame" if variant == "frame_clamp" else "K")
    split = [yc.split_chroma(f, l) for f, l in zip(frames, lays)]
    orig = [np.stack([u, v], axis=2) for _, u, v in split]
    out = [o.copy() for o in orig]
    owner = [np.full(o.shape[:2], -1, np.int64) for o in orig]       # "k_lists": who painted a sample
    rows = ec.as_rows(rects)
    ks = {}
    for idx, r in enumerate(rows):
        f, x, y, w, h = ec.map_region(r, scale, margin)
        fh, fw = frames[f][0].shape
        k = pcs.clip((x, y, w, h), fw, fh)
        if k is None:
            continue
        ks[idx] = (f, k)
        s = pcs.size_of(mode, w, h, size, rel)
        cs = s if variant == "luma_sizes" else chroma_size(mode, s)
        kc = chroma_rect(k)
        mask = chroma_mask(luma_mask(mode, (x, y, w, h), k, s, ellipse, fw, fh), variant == "top_left")[kc[1]:kc[3], kc[0]:kc[2]]
        val = chroma_values(mode, out[f] if variant == "sequential" else orig[f], kc, cs, (Uc, Vc), variant == "truncate", variant == "frame_clamp")
        own = owner[f][kc[1]:kc[3], kc[0]:kc[2]]
        if variant == "k_lists":
            for j, (fj, kj) in ks.items():
                if j != idx and fj == f and not (k[0] < kj[2] and kj[0] < k[2] and k[1] < kj[3] and kj[1] < k[3]):
                    mask = mask & (own != j)                           # region j does not know of this one: it keeps the sample
        view = out[f][kc[1]:kc[3], kc[0]:kc[2]]
        view[mask] = val[mask]
        own[mask] = idx
    return [yc.join_chroma(np.asarray(y), np.ascontiguousarray(o[..., 0]), np.ascontiguousarray(o[..., 1]), l) for y, o, l in zip(ys, out, lays)]


def painted_union(frames, rects, mode, size=0, rel=0.25, scale=(1.0, 1.0), margin=0.0, ellipse=False):
    """Per frame (luma mask, chroma mask) of the union of the painted sets."""
    mode = MODES.get(mode, mode)
    res = [(np.zeros(f[0].shape, bool), np.zeros((f[0].shape[0] // 2, f[0].shape[1] // 2), bool)) for f in frames]
    for r in ec.as_rows(rects):
        f, x, y, w, h = ec.map_region(r, scale, margin)
        fh, fw = frames[f][0].shape
        k = pcs.clip((x, y, w, h), fw, fh)
        if k is None:
            continue
        full = luma_mask(mode, (x, y, w, h), k, pcs.size_of(mode, w, h, size, rel), ellipse, fw, fh)
        res[f][0][:] |= full
        res[f][1][:] |= chroma_mask(full)
    return res


def layout(sizes, rects, mode, size=0, rel=0.25, scale=(1.0, 1.0), margin=0.0):
    """What vj_paint_yuv_layout must report: (K rows, Kc rows, luma sizes, chroma sizes, scratch bytes).  sizes: (w, h) per frame."""
    mode = MODES.get(mode, mode)
    a16 = lambda v: (v + 15) // 16 * 16
    ks, kcs, ss, css, scratch = [], [], [], [], 0
    for r in ec.as_rows(rects):
        f, x, y, w, h = ec.map_region(r, scale, margin)
        k = pcs.clip((x, y, w, h), sizes[f][0], sizes[f][1])
        s = pcs.size_of(mode, w, h, size, rel)
        cs = chroma_size(mode, s)
        ss.append(s)
        css.append(cs)
        if k is None:
            ks.append((f, 0, 0, 0, 0))
            kcs.append((f, 0, 0, 0, 0))
            continue
        kc = chroma_rect(k)
        kw, kh, cw, chh = k[2] - k[0], k[3] - k[1], kc[2] - kc[0], kc[3] - kc[1]
        ks.append((f, k[0], k[1], kw, kh))
        kcs.append((f, kc[0], kc[1], cw, chh))
        if mode == BLUR:
            scratch += a16(2 * kh * kw) + 2 * a16(2 * chh * cw)
        elif mode == PIXELATE:
            scratch += a16(-(-kw // s) * -(-kh // s)) + 2 * a16(-(-cw // cs) * -(-chh // cs))
    return (np.array(ks, np.int32).reshape(-1, 5), np.array(kcs, np.int32).reshape(-1, 5), np.array(ss, np.int32), np.array(css, np.int32), scratch)


# ---- buffers: planes placed at chosen addresses mod 4 with padded strides and sentinel bytes all around
SENTINEL = 0xA5


def place(planes, layout, mods=(0, 0, 0), pad=0, gap=32):
    """One uint8 buffer that holds the planes of a frame: plane i begins at an offset = mods[i] (mod 4) behind `gap` sentinel bytes,
    its rows `pad` sentinel bytes longer than the row (the chroma planes of I420 share one stride).  -> (buffer, [(offset, stride)])."""
    strides = [planes[0].shape[1] + pad] + [planes[1].shape[1] + pad] * (len(planes) - 1)
    at, offs = 0, []
    for p, st, m in zip(planes, strides, mods):
        at += gap
        at += (m - at) % 4
        offs.append((at, st))
        at += st * p.shape[0]
    buf = np.full(at + gap, SENTINEL, np.uint8)
    for p, (o, st) in zip(planes, offs):
        rows = buf[o:o + st * p.shape[0]].reshape(p.shape[0], st)
        rows[:, :p.shape[1]] = p
    return buf, offs


# ---- the shared cases
W, H = 38, 30
# regions of the 38 x 30 frames: 1 x 1 at even and odd positions, 2 x 2 at an odd corner (four chroma samples), 1 x n, n x 1, each side,
# each corner, partly and wholly outside, an inner box.  All four parities of cx0, cx1, cy0, cy1 occur.
SMALL_RECTS = [(0, 4, 6, 1, 1), (0, 7, 9, 1, 1), (0, 4, 9, 1, 1), (0, 11, 13, 2, 2), (0, 20, 2, 1, 9), (0, 21, 3, 1, 8), (0, 9, 20, 11, 1),
               (0, 8, 23, 12, 1), (0, -5, 8, 10, 10), (0, 31, 9, 10, 9), (0, 8, -5, 11, 10), (0, 9, 25, 10, 10),
               (0, -3, -3, 10, 10), (0, 31, -3, 10, 10), (0, -3, 23, 10, 10), (0, 31, 23, 10, 10),
               (0, 100, 100, 6, 6), (0, -40, 3, 6, 6), (0, 5, -30, 6, 6), (0, 13, 9, 14, 12), (0, 12, 10, 15, 11)]
# sixteen boxes on a 4 x 4 grid: every combination of the parities of cx0, cx1, cy0, cy1
PARITY_RECTS = [(0, 2 + 8 * (i % 4) + (i & 1), 2 + 6 * (i // 4) + (i >> 2 & 1), 6 + (i >> 1 & 1) - (i & 1), 4 + (i >> 3 & 1) - (i >> 2 & 1)) for i in range(16)]
SMALL_RECTS += PARITY_RECTS
WHOLE = [(0, 0, 0, W, H)]
TINY_RECTS = [(0, 0, 0, 1, 1), (0, 1, 1, 1, 1), (0, 0, 0, 2, 2), (0, 1, 0, 1, 2), (0, -1, -1, 2, 2)]      # of the 2 x 2 frame
FILL_BGR = (17, 201, 94)
# overlaps: three regions of differing sizes, the middle one covering part of both others; the same region twice
OVERLAP_RECTS = [(0, 3, 3, 20, 15), (0, 11, 7, 22, 18), (0, 6, 12, 13, 9)]
TWICE_RECTS = [(0, 5, 5, 13, 11), (0, 5, 5, 13, 11)]
# the shared-sample pair: x ranges [2, 7) and [7, 12) are disjoint and share chroma sample 3
SHARED_RECTS = [(0, 2, 4, 5, 7), (0, 7, 4, 5, 7)]
ROUNDING_RECT = [(0, 5, 3, 21, 15)]
WIDE_W, WIDE_H = 300, 40
BIG_W, BIG_H = 524, 68       # its I420 chroma rows (262 bytes) and chroma heights (34) straddle the block and band constants too


def wide_rects():
    """Regions of the 300 x 40 frame whose luma rows and pair-plane rows lie around the wave-row / band width (256 bytes) and the lane
    width (4 bytes), at even and odd corners, taller than a block of rows."""
    u = pcs.units_header()
    wr = u["PAINT_BLOCK_SLOTS"] * 4
    assert wr == u["PAINT_BAND_COLS"] == 256 and u["PAINT_BLOCK_H"] == u["PAINT_BAND_H"] == 32
    return [(0, 2, 1, wr - 2, 37), (0, 2, 2, wr, 35), (0, 1, 0, wr + 1, 40), (0, 3, 3, wr + 2, 32), (0, 40, 5, 3, 3), (0, 41, 6, 4, 4), (0, 50, 7, 5, 5),
            (0, -5, -5, 400, 20), (0, 299, 39, 5, 5)]


def big_rects():
    """Regions of the 524 x 68 frame: I420 chroma rows of 255 .. 258 bytes, chroma heights of 31 .. 34 rows."""
    return [(0, 2, 2, 510, 62), (0, 3, 2, 511, 64), (0, 0, 0, 514, 66), (0, 5, 0, 516, 68)]


def frame(w, h, layout, seed):
    return yc.random_frame(w, h, layout, seed)


def smooth_frame(w, h, layout, seed):
    """A frame whose rounding matters: values whose window and cell sums leave remainders of at least half the divisor somewhere."""
    rng = np.random.default_rng(seed)
    mk = lambda hh, ww: (rng.integers(0, 4, (hh, ww)) + 97 + (np.arange(ww)[None, :] % 5)).astype(np.uint8)
    return yc.join_chroma(mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2), layout)


def same(a, b) -> bool:
    """Two lists of plane tuples equal."""
    return len(a) == len(b) and all(len(p) == len(q) and all(np.array_equal(x, y) for x, y in zip(p, q)) for p, q in zip(a, b))
