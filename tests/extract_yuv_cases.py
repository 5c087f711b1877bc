"""The restatement of vj_extract_yuv / vj_extract_affine_yuv (include/vj.h) and the cases
tests/test_extract_yuv_cpu.py and tests/test_gpu_extract_yuv.py share.

The restatement IS the definition's sentence, a composition of restatements that exist: yuv_cases.decode of every frame, then
extract_cases.restate (or affine_cases.restate) on the decoded images.  Nothing new computes the right bytes.

model() is something else: the same function written tap by tap, the way a kernel has to compute it — the taps of §4.8 as numpy index
and weight arrays, the clamps, the chroma index, the decode of each tap, the blend.  The CPU test shows that it equals the restatement
(so the per-tap description in vj.h says the same as the sentence), and its deliberately WRONG variants are what that test tells from
the right one on the cases meant to catch them:
  "blend_first"    blend Y, U and V with the resize arithmetic, decode afterwards
  "chroma_before"  the chroma sample from the tap's coordinate BEFORE the crop-edge clamp.  (Before the FRAME clamp alone there is
                   nothing to tell: (x >> 1) clamped to the chroma plane is (x clamped to the frame) >> 1 when the sizes are even.)
                   It shows where a tap beyond the crop's edge belongs to another chroma sample: above a crop whose y0 is even,
                   left of one whose x0 is even, below or right of one whose far edge is even.
  "chroma_split"   the chroma index (x0 >> 1) + (j >> 1) instead of (x0 + j) >> 1: wrong at odd origins
  "swap_uv"        U and V exchanged (what reading NV21 as NV12 gives)
  "frame_clamp"    the taps clamped at the frame instead of at the crop"""
from __future__ import annotations

import numpy as np

import affine_cases as ac
import extract_cases as ec
import prep_cases as pc
import yuv_cases as yc

LAYOUTS = [yc.NV12, yc.NV21, yc.I420]
VARIANTS = ["blend_first", "chroma_before", "chroma_split", "swap_uv", "frame_clamp"]


def _layouts(frames, layout):
    return list(layout) if isinstance(layout, (list, tuple)) else [layout] * len(frames)


def decoded(frames, layout, alpha=False, rgb=False):
    """yuv_cases.decode per frame: what vj_yuv_to_bgr returns.  layout: one, or one per frame."""
    return [yc.decode(f, lay, 4 if alpha else 3, rgb) for f, lay in zip(frames, _layouts(frames, layout))]


def restate(oracle, frames, layout, rects, size, scale=(1.0, 1.0), margin=0.0, gray=False, planar=False, alpha=False, rgb=False):
    """What vj_extract_yuv must write: vj_extract's bytes on the decoded frames."""
    return ec.restate(oracle, decoded(frames, layout, alpha, rgb), rects, size, scale, margin, gray, planar)


def restate_affine(oracle, frames, layout, affines, size, gray=False, planar=False, alpha=False, rgb=False):
    """What vj_extract_affine_yuv must write: vj_extract_affine's bytes on the decoded frames."""
    return ac.restate(oracle, decoded(frames, layout, alpha, rgb), affines, size, gray, planar)


# ------------------------------------------------------------------------------------------------------------- the tap-level model
def _src_coord(d, scale):
    f = np.float32((d + 0.5) * scale - 0.5)
    i = int(np.floor(f))
    return i, np.float32(f - np.float32(i))


def _coef(v):
    return int(np.clip(pc.cv_round(float(np.float32(v) * np.float32(2048))), -32768, 32767))


def axis_taps(src, dst, rows, crop_clamp=True):
    """§4.8's taps of a src -> dst resize -> (i0, i1, u0, u1, w0, w1) int arrays of length dst.  i0, i1: the two source indices,
    clamped to [0, src) (crop_clamp=False: left as they fall); u0, u1: the same before that clamp; w0, w1: the 11-bit weights.  Rows
    keep their fraction and clamp the indices; columns take one tap with weight 2048 beyond either edge."""
    scale = 1.0 / (float(dst) / float(src))
    out = []
    for d in range(dst):
        s, f = _src_coord(d, scale)
        u0, u1 = s, s + 1
        if not crop_clamp:
            out.append((u0, u1, u0, u1, _coef(np.float32(1) - f), _coef(f)))
        elif rows:
            out.append((min(max(s, 0), src - 1), min(max(s + 1, 0), src - 1), u0, u1, _coef(np.float32(1) - f), _coef(f)))
        else:
            if s < 0:
                s, f = 0, np.float32(0)
            if s >= src - 1:
                out.append((src - 1, src - 1, u0, u1, 2048, 0))
            else:
                out.append((s, s + 1, u0, u1, _coef(np.float32(1) - f), _coef(f)))
    return [np.array(c, np.int64) for c in zip(*out)]


def _blend(t00, t01, t10, t11, a0, a1, b0, b1):
    h0, h1 = t00 * a0 + t01 * a1, t10 * a0 + t11 * a1
    return (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2


def model(planes, layout, region, size, variant=None, alpha=False, rgb=False):
    """One mapped region (x, y, w, h), in luma pixels, of one frame to size = (w, h), tap by tap -> (h, w, C) uint8."""
    y, u, v = (p.astype(np.int64) for p in yc.split_chroma(planes, layout))
    if variant == "swap_uv":
        u, v = v, u
    H, W = y.shape
    x0, y0, cw, ch = (int(t) for t in region)
    ow, oh = int(size[0]), int(size[1])
    clamp = variant != "frame_clamp"
    if cw == 2 * ow and ch == 2 * oh:                  # the 2 x 2 mean: taps 2 d, 2 d + 1, the sum rounded
        ix0, iy0 = 2 * np.arange(ow), 2 * np.arange(oh)
        ix1, iy1, ux0, ux1, uy0, uy1 = ix0 + 1, iy0 + 1, ix0, ix0 + 1, iy0, iy0 + 1
        wts = None
    else:
        ix0, ix1, ux0, ux1, a0, a1 = axis_taps(cw, ow, False, clamp)
        iy0, iy1, uy0, uy1, b0, b1 = axis_taps(ch, oh, True, clamp)
        wts = (a0[None, :], a1[None, :], b0[:, None], b1[:, None])
    taps = []
    for iy, uy in ((iy0, uy0), (iy1, uy1)):
        for ix, ux in ((ix0, ux0), (ix1, ux1)):
            ly, lx = np.clip(y0 + iy, 0, H - 1), np.clip(x0 + ix, 0, W - 1)
            if variant == "chroma_before":
                cy, cx = np.clip((y0 + uy) >> 1, 0, H // 2 - 1), np.clip((x0 + ux) >> 1, 0, W // 2 - 1)
            elif variant == "chroma_split":
                cy, cx = np.clip((y0 >> 1) + (iy >> 1), 0, H // 2 - 1), np.clip((x0 >> 1) + (ix >> 1), 0, W // 2 - 1)
            else:
                cy, cx = ly >> 1, lx >> 1
            Y, U, V = y[np.ix_(ly, lx)], u[np.ix_(cy, cx)], v[np.ix_(cy, cx)]
            if variant == "blend_first":
                taps.append(np.stack([Y, U, V], axis=2))
            else:
                b, g, r = yc.decode_px(Y, U, V)
                chans = [r, g, b] if rgb else [b, g, r]
                taps.append(np.stack([c.astype(np.int64) for c in chans] + ([np.full(Y.shape, 255, np.int64)] if alpha else []), axis=2))
    if wts is None:
        out = (taps[0] + taps[1] + taps[2] + taps[3] + 2) >> 2
    else:
        out = _blend(*taps, *(w[:, :, None] for w in wts))
    if variant == "blend_first":
        b, g, r = yc.decode_px(out[..., 0], out[..., 1], out[..., 2])
        out = np.stack(([r, g, b] if rgb else [b, g, r]) + ([np.full(b.shape, 255)] if alpha else []), axis=2)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------- the cases
SIZES = [(38, 30), (66, 34)]                            # the frames of the GPU tests: random, full range
OUT_WIDTHS = list(range(1, 10)) + [21, 63, 64, 65, 255, 256, 257]
OUT_HEIGHTS = [1, 2, 5, 15, 16, 17]


def frames(layout, seed=71):
    return [yc.random_frame(w, h, layout, seed + i) for i, (w, h) in enumerate(SIZES)]


def crops(frame=0, fw=38, fh=30):
    """Crops of 1 x 1, 2 x 3, 5 x 5 and 20 x 17 at even and odd x and y, over every side and corner of a fw x fh frame, wholly
    outside it, and the whole frame — rows of (frame, x, y, w, h)."""
    out = []
    for w, h in [(1, 1), (2, 3), (5, 5), (20, 17)]:
        for x, y in [(8, 6), (9, 6), (8, 7), (9, 7)]:
            out.append((frame, x, y, w, h))
        for x, y in [(-w // 2 - 1, 8), (fw - w // 2 - 1, 9), (7, -h // 2 - 1), (8, fh - h // 2 - 1),
                     (-1, -1), (fw - w + 1, -1), (-1, fh - h + 1), (fw - w + 1, fh - h + 1)]:
            out.append((frame, x, y, w, h))
        out.append((frame, fw + 20, fh + 11, w, h))
        out.append((frame, -50, 3, w, h))
    out.append((frame, 0, 0, fw, fh))
    return out


def resize_cases(frame=0):
    """(rects, size): the copy, the 2 x 2 mean and the bilinear path of the same 10 x 10 and 20 x 17 boxes, inside at the four
    parities of the origin and over every side and corner."""
    boxes = [(8, 6), (9, 6), (8, 7), (9, 7), (-5, 8), (33, 9), (8, -5), (9, 25), (-3, -3), (31, -3), (-3, 23), (31, 23), (100, 100), (-40, 3)]
    r10 = [(frame, x, y, 10, 10) for x, y in boxes]
    r20 = [(frame, x, y, 20, 16) for x, y in boxes]
    return [(r10, (10, 10)), (r10, (5, 5)), (r10, (7, 3)), (r20, (20, 16)), (r20, (10, 8)), (r20, (64, 34)), (r10 + r20, (21, 17))]


FLAG_CASES = [dict(alpha=a, rgb=r, gray=g, planar=p) for a in (False, True) for r in (False, True) for g in (False, True) for p in (False, True)]


def edge_planes(layout):
    """extract_cases.edge_frame as a 4:2:0 frame, 38 x 30: Y up to 60 inside EDGE_RECT and from 200 outside it, and chroma that differs
    as strongly — U, V up to 60 at the samples of the crop, from 200 around them."""
    rng = np.random.default_rng(43)
    w, h = 38, 30
    y = rng.integers(200, 256, (h, w), dtype=np.uint8)
    u = rng.integers(200, 256, (h // 2, w // 2), dtype=np.uint8)
    v = rng.integers(200, 256, (h // 2, w // 2), dtype=np.uint8)
    _, rx, ry, rw, rh = ec.EDGE_RECT
    y[ry:ry + rh, rx:rx + rw] = rng.integers(1, 61, (rh, rw), dtype=np.uint8)
    cy0, cy1, cx0, cx1 = ry >> 1, (ry + rh + 1) >> 1, rx >> 1, (rx + rw + 1) >> 1
    u[cy0:cy1, cx0:cx1] = rng.integers(1, 61, (cy1 - cy0, cx1 - cx0), dtype=np.uint8)
    v[cy0:cy1, cx0:cx1] = rng.integers(1, 61, (cy1 - cy0, cx1 - cx0), dtype=np.uint8)
    return yc.join_chroma(y, u, v, layout)


def affine_matrices():
    """(name, matrices, size) on a 38 x 30 frame: affine_cases' families (they were made for 37 x 29)."""
    return [("identity", [ac.identity()], (38, 30)),
            ("translation", [ac.translation(3, 2), ac.translation(-4, 5), ac.translation(7, -3)], (20, 17)),
            ("rot", [ac.ROT, ac.mirrored(ac.ROT, ac.ROT_SIZE[0])], ac.ROT_SIZE),
            ("shear", [ac.SHEAR, ac.DOWN5, ac.UP4], (21, 17)),
            ("ties", ac.tie_family(), ac.TIE_SIZE),
            ("edges", ac.edge_matrices(), (12, 10))]


REPRESENTATIVE = ac.rotation(20.0, 0.8, (17.5, 13.0), (21, 17))     # the flag and placement variations of the affine call


# ---- the end-to-end case: the 432 x 324 colour sources of tests/test_gpu_paint.py (extract_cases.e2e_bgr) encoded to NV12
_E2E = None


def e2e_nv12():
    """[(y, uv)] of the three frames; built once; do not modify."""
    global _E2E
    if _E2E is None:
        _E2E = [yc.encode(f, yc.NV12) for f in ec.e2e_bgr()]
    return _E2E
