"""Cases of vj_extract_affine, shared by tests/test_affine_cpu.py — which checks the layout, the limits, the matrix
helpers and the pairing rule through ctypes and states the premises of the GPU tests on the CPU with the restatement alone — and
tests/test_gpu_affine.py, which runs them on the device.

warp() restates §4.19's definition in numpy, with prep_cases.cv_round as rne and oracle.bgr2gray for the gray flag (the conversion
is per pixel, so converting the frame and then taking the taps is taking the taps through it).  Nothing else computes these bytes;
the independent cross-checks (identity, integer translation against extract_cases.padded_crop, the quarter turn against an index
permutation) tie it to things that do not share its arithmetic.  from_rect(), from_eyes() and align() restate the two matrix
helpers and the pairing rule of align_transforms."""
from __future__ import annotations

import math

import numpy as np

import prep_cases as pc

W, H = 37, 29


def half_up(v: float) -> int:
    """NOT the definition: round half up, the variant the tie family tells from cv_round."""
    return int(math.floor(np.float64(v) + 0.5))


def positions(m, size, rnd=pc.cv_round, offset=16):
    """-> (X, Y): (out_h, out_w) int64 arrays of the 1/32-pixel positions (source index << 5 | fraction)."""
    ow, oh = int(size[0]), int(size[1])
    m = [float(v) for v in m]
    ax = np.array([rnd((m[0] * float(x)) * 1024.0) for x in range(ow)], np.int64)
    bx = np.array([rnd((m[3] * float(x)) * 1024.0) for x in range(ow)], np.int64)
    x0 = np.array([rnd((m[1] * float(y) + m[2]) * 1024.0) + offset for y in range(oh)], np.int64)
    y0 = np.array([rnd((m[4] * float(y) + m[5]) * 1024.0) + offset for y in range(oh)], np.int64)
    s = x0[:, None] + ax[None, :]
    t = y0[:, None] + bx[None, :]
    assert np.abs(s).max() < 2**31 and np.abs(t).max() < 2**31           # int32 in the library
    return s >> 5, t >> 5


def warp(oracle, frame: np.ndarray, m, size, gray=False, rnd=pc.cv_round, offset=16) -> np.ndarray:
    """One region: (out_h, out_w, C) uint8."""
    f = np.asarray(frame)
    if gray and f.ndim == 3:
        f = oracle.bgr2gray(np.ascontiguousarray(f))
    if f.ndim == 2:
        f = f[:, :, None]
    fh, fw = f.shape[:2]
    X, Y = positions(m, size, rnd, offset)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    w = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    assert np.all(w[0] + w[1] + w[2] + w[3] == 32768)
    acc = np.full(X.shape + (f.shape[2],), 16384, np.int64)
    for wk, (i, j) in zip(w, ((0, 0), (0, 1), (1, 0), (1, 1))):
        p = f[np.clip(sy + i, 0, fh - 1), np.clip(sx + j, 0, fw - 1)].astype(np.int64)
        acc += p * wk[:, :, None]
    assert int(acc.max()) < 2**31
    return (acc >> 15).astype(np.uint8)


def as_rows(affines) -> np.ndarray:
    """(n, 7) float64 rows of (frame, m0 .. m5) from rows or from an AFFINE_DTYPE array."""
    a = np.asarray(affines)
    if a.dtype.names is not None:
        return np.concatenate([a["frame"].astype(np.float64).reshape(-1, 1), a["m"].reshape(-1, 6)], axis=1)
    return a.astype(np.float64).reshape(-1, 7)


def restate(oracle, frames, affines, size, gray=False, planar=False, **kw) -> np.ndarray:
    """What vj_extract_affine must write: (n, h, w, C) uint8, or (n, C, h, w) with planar=True."""
    outs = [warp(oracle, frames[int(r[0])], r[1:], size, gray, **kw) for r in as_rows(affines)]
    ch = outs[0].shape[2] if outs else 1
    out = np.stack(outs) if outs else np.zeros((0, int(size[1]), int(size[0]), ch), np.uint8)
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)) if planar else out


def touches(m, size, fw, fh):
    """-> (samples with a fractional position, samples with a clamped tap) of one region."""
    X, Y = positions(m, size)
    sx, sy = X >> 5, Y >> 5
    frac = ((X & 31) != 0) | ((Y & 31) != 0)
    clamped = (sx < 0) | (sx + 1 > fw - 1) | (sy < 0) | (sy + 1 > fh - 1)
    return int(frac.sum()), int(clamped.sum())


# ------------------------------------------------------------------------------------------------------------------ the matrices
def identity():
    return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def translation(tx, ty):
    return [1.0, 0.0, float(tx), 0.0, 1.0, float(ty)]


def quarter_turn(x0, y0, out_w):
    """out[y][x] = frame[y0 + out_w - 1 - x][x0 + y]"""
    return [0.0, 1.0, float(x0), -1.0, 0.0, float(y0 + out_w - 1)]


def rotation(deg, scale, centre, size):
    """The output's centre pixel lands on `centre` of the source; output steps are `scale` source pixels long, turned by `deg`."""
    a, b = scale * math.cos(math.radians(deg)), scale * math.sin(math.radians(deg))
    ox, oy = (size[0] - 1) / 2, (size[1] - 1) / 2
    return [a, -b, centre[0] - a * ox + b * oy, b, a, centre[1] - b * ox - a * oy]


def mirrored(m, out_w):
    """The same region with its columns reversed."""
    return [-m[0], m[1], m[2] + m[0] * (out_w - 1), -m[3], m[4], m[5] + m[3] * (out_w - 1)]


ROT_SIZE = (33, 21)
ROT = rotation(30.0, 1.3, (18.0, 14.0), ROT_SIZE)
SHEAR = [1.0, 0.375, 2.25, 0.125, 1.0, -1.5]
DOWN5 = [5.0, 0.0, 1.3, 0.0, 5.0, 0.7]                # 5 x down-scale: 8 x 6 outputs span the frame
UP4 = [0.25, 0.0, 10.1, 0.0, 0.25, 8.3]               # 4 x up-scale
TIE_SIZE = (36, 28)


def tie_family():
    """Positions that are ties of rne at many pixels: (1 + 1/2048) x * 1024 = 1024 x + x / 2 is a half for every odd x."""
    return [[1.0 + 1.0 / 2048, 0.0, j / 1024, 0.0, 1.0 + 1.0 / 2048, (31 - j) / 1024] for j in range(32)]


def edge_matrices():
    """Regions over each side and corner of the 37 x 29 frame and wholly outside it, turned a little so fractions occur."""
    out = []
    for cx, cy in [(-3, 14), (39, 14), (18, -3), (18, 31), (-2, -2), (38, -2), (-2, 30), (38, 30), (100, 100), (-60, 5), (5, -50)]:
        out.append(rotation(10.0, 0.9, (float(cx), float(cy)), (12, 10)))
    return out


def sources(seed):
    """Random 37 x 29 frames: gray, BGR, BGRA."""
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, (H, W), dtype=np.uint8), rng.integers(1, 256, (H, W, 3), dtype=np.uint8),
            rng.integers(1, 256, (H, W, 4), dtype=np.uint8)]


def rows_for(frame, matrices):
    return np.array([[float(frame)] + [float(v) for v in m] for m in matrices], np.float64).reshape(-1, 7)


# ------------------------------------------------------------------------------------------------- the helpers and the pairing rule
def from_rect(x, y, w, h, size):
    x, y, w, h = float(x), float(y), float(w), float(h)
    ow, oh = int(size[0]), int(size[1])
    return [w / ow, 0.0, x + 0.5 * w / ow - 0.5, 0.0, h / oh, y + 0.5 * h / oh - 0.5]


def from_eyes(lx, ly, rx, ry, size, eye_pos=(0.3, 0.7, 0.35)):
    lx, ly, rx, ry = float(lx), float(ly), float(rx), float(ry)
    ow, oh = int(size[0]), int(size[1])
    ex_l, ex_r, ey = (float(v) for v in eye_pos)
    d = (ex_r - ex_l) * ow
    a, b = (rx - lx) / d, (ry - ly) / d
    cxl, cy = ex_l * ow, ey * oh
    return [a, -b, lx - a * cxl + b * cy, b, a, ly - b * cxl - a * cy]


def align(face_rects, eye_rects, size, eye_pos=(0.3, 0.7, 0.35), scale=(1.0, 1.0)):
    """The pairing rule of align_transforms restated -> ((n, 7) rows, paired as a list of bool)."""
    sx, sy = float(scale[0]), float(scale[1])
    rows, paired = [], []
    for k, f in enumerate(face_rects):
        x, y, w, h = float(f["x"]), float(f["y"]), float(f["w"]), float(f["h"])
        left = right = None
        for e in eye_rects:
            if int(e["frame"]) != k:
                continue
            cx, cy = float(e["x"]) + float(e["w"]) / 2, float(e["y"]) + float(e["h"]) / 2
            if cy >= h / 2:
                continue
            if cx < w / 2:
                if left is None or float(e["weight"]) > left[0]:
                    left = (float(e["weight"]), cx, cy)
            elif right is None or float(e["weight"]) > right[0]:
                right = (float(e["weight"]), cx, cy)
        if left is not None and right is not None:
            m = from_eyes((x + left[1]) * sx, (y + left[2]) * sy, (x + right[1]) * sx, (y + right[2]) * sy, size, eye_pos)
        else:
            m = from_rect(x * sx, y * sy, w * sx, h * sy, size)
        rows.append([float(int(f["frame"]))] + m)
        paired.append(left is not None and right is not None)
    return np.array(rows, np.float64).reshape(-1, 7), paired


def rects(rows):
    """A RECT_DTYPE-like array from rows of (frame, x, y, w, h, weight)."""
    dt = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("weight", "<f4"), ("frame", "<i4"), ("scale_idx", "<i4")])
    out = np.zeros(len(rows), dt)
    for i, (f, x, y, w, h, wt) in enumerate(rows):
        out[i] = (x, y, w, h, wt, f, 0)
    return out


# ---- the end-to-end case: frontalface_alt then eye (raw candidates) on the prepared 240 x 180 frames of tests/prep_cases.py, faces
# grouped with min_neighbors = 3; every face cut from the 432 x 324 colour sources (extract_cases.e2e_bgr, factor 1.8) to 32 x 32.
# The counts are the oracle's (tests/test_affine_cpu.py asserts them; tests/test_gpu_affine.py expects the same of the device).
# The eye cascade finds nothing inside these drawn faces, so no face is paired and every crop is the box's (affine_from_rect): the
# hand-made case below runs the other branch.
E2E_SIZE = (32, 32)
E2E_FACES = 9
E2E_PAIRED = 0

# a hand-made paired case on the same sources: one face with an eye on each side, so affine_from_eyes' branch runs on the device too
HAND_FACES = [(0, 60, 40, 80, 80, 0.0), (1, 100, 50, 64, 64, 0.0), (2, 20, 30, 90, 90, 0.0)]
HAND_EYES = [(0, 12, 18, 20, 16, 2.0), (0, 46, 22, 20, 16, 3.0), (0, 30, 60, 20, 16, 9.0),      # face 0: both eyes, and a mouth
             (1, 8, 10, 16, 16, 1.0),                                                             # face 1: one eye
             (2, 10, 12, 22, 20, 1.0), (2, 50, 20, 22, 20, 1.0), (2, 52, 8, 20, 20, 1.0)]         # face 2: a weight tie on the right
