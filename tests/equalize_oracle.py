"""cv::equalizeHist for 8-bit single-channel images (OpenCV imgproc/histogram.cpp, 2.4.4 .. 4.x) restated in numpy, line by line as
DESIGN.md §4.15 defines it — the reference of vj_equalize_hist and VJ_FLAG_EQUALIZE_HIST (tests/test_equalize_cpu.py,
tests/test_gpu_equalize.py).  All float arithmetic is binary32 through np.float32: one division, one int -> float conversion and
one multiplication per table entry, each correctly rounded; np.rint rounds halves to even, as cvRound does."""
from __future__ import annotations

import numpy as np


def lut(gray: np.ndarray):
    """The 256-entry table of one image, or None for an image of one value (which equalizeHist returns unchanged).  Entries below
    the lowest value present are never read by a pixel; they are 0 here."""
    assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.size > 0
    hist = np.bincount(gray.reshape(-1), minlength=256).astype(np.int64)        # 1. hist[v] = pixels of value v
    total = int(gray.size)
    i = int(np.flatnonzero(hist)[0])                                            # 2. the lowest value present
    if hist[i] == total:
        return None
    scale = np.float32(255.0) / np.float32(total - int(hist[i]))                # 3. one binary32 division ((float)int is exact or RNE)
    assert scale.dtype == np.float32
    table = np.zeros(256, np.uint8)                                             # 4. lut[i] = 0, sum = 0
    s = 0
    for k in range(i + 1, 256):                                                 # 5. sum += hist[k]; lut[k] = saturate_cast<uchar>(sum * scale)
        s += int(hist[k])
        assert s < 2**31
        prod = np.float32(s) * scale                                            #    np.float32(int) rounds to nearest even, as (float)int does
        assert prod.dtype == np.float32
        table[k] = min(max(int(np.rint(prod)), 0), 255)
    return table


def equalize(gray: np.ndarray) -> np.ndarray:
    """6. dst = lut[src]"""
    t = lut(gray)
    return gray.copy() if t is None else t[gray]


_CACHE = {}


def equalized(frames) -> list:
    """equalize() of every frame of a list that is built once and never modified (mixed_cases.frames(), a test's own batch):
    computed once per list and frame."""
    out = []
    for f in frames:
        key = (f.shape, hash(f.tobytes()))
        if key not in _CACHE:
            e = equalize(np.ascontiguousarray(f))
            e.setflags(write=False)
            _CACHE[key] = e
        out.append(_CACHE[key])
    return out
