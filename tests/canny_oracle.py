"""ctypes view of tests/canny_oracle.c — the test restatement of CV_HAAR_DO_CANNY_PRUNING (Canny edge map + pruned walk).
Compiled with gcc and oracle/Makefile's flags on first use, into a temporary directory (nothing is written to the tree)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle.oracle import _RECT_DT, CascadeArrays, Oracle, _OcCascade, _OcStats

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Wno-unused-parameter"]
_LIB = None


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="canny_oracle_"), "libcannyoracle.so")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, os.path.join(HERE, "canny_oracle.c"), "-lm"],
                       check=True, capture_output=True)
        L = C.CDLL(out)
        L.cn_canny.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.cn_canny.restype = None
        L.cn_detect_opencvlike.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_double, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_OcStats)]
        L.cn_detect_opencvlike.restype = C.c_int
        _LIB = L
    return _LIB


def canny(gray: np.ndarray) -> np.ndarray:
    """cvCanny(gray, edges, 0, 50, 3) as restated in DESIGN.md §4.7: (h, w) uint8, 255 on edges."""
    assert gray.dtype == np.uint8 and gray.ndim == 2
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    e = np.empty((h, w), np.uint8)
    _lib().cn_canny(g.ctypes.data, w, h, g.strides[0], e.ctypes.data, e.strides[0])
    return e


def detect_opencvlike(c: CascadeArrays, gray: np.ndarray, min_size=(0, 0), scale_factor: float = 1.1, prune: bool = True,
                      cap: int = 1 << 20, sq_clause: bool = True):
    """Oracle.detect_opencvlike's walk with (prune=True) or without the canny pruning test.  sq_clause=False drops the test's
    sq < 20 half (not OpenCV: it lets tests show that a frame exercises that half).  Returns (rects, stats)."""
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    s, keep = Oracle._cstruct(c)
    out = np.zeros(cap, _RECT_DT)
    n_total = C.c_int(0)
    st = _OcStats()
    n = _lib().cn_detect_opencvlike(C.byref(s), g.ctypes.data, w, h, g.strides[0], min_size[0], min_size[1], float(scale_factor),
                                    (1 if sq_clause else 2) if prune else 0, out.ctypes.data, cap, C.byref(n_total), C.byref(st))
    if n < 0:
        raise ValueError("a pruning rectangle reaches past the frame's integral allocation")
    return out[:n], {"windows": int(st.windows), "stump_evals": int(st.stump_evals),
                     "stage_entered": [int(v) for v in st.stage_entered[:c.n_stages]]}


def patches_frame(seed: int, h: int, w: int) -> np.ndarray:
    """Content where pruning bites: a flat background with a few textured patches and crude faces (the synth generators
    have edges almost everywhere)."""
    from clfacedetection_amd import synth
    rng = np.random.default_rng(seed)
    f = np.full((h, w), 96, np.uint8)
    for _ in range(3):
        ph, pw = int(rng.integers(h // 8, h // 3)), int(rng.integers(w // 8, w // 3))
        y, x = int(rng.integers(0, h - ph)), int(rng.integers(0, w - pw))
        f[y:y + ph, x:x + pw] = rng.integers(0, 256, (ph, pw), dtype=np.uint8)
    for _ in range(2):
        s = int(rng.integers(max(24, min(h, w) // 8), max(25, min(h, w) // 3)))
        y, x = int(rng.integers(0, h - s)), int(rng.integers(0, w - s))
        f[y:y + s, x:x + s] = synth.crude_face(s)
    return f


def soft_face_frame(h: int = 240, w: int = 320) -> np.ndarray:
    """A blurred low-contrast crude face on a flat background: the cascade finds it, Canny finds no edge (every window pruned)."""
    from clfacedetection_amd import synth
    g = np.full((h, w), 96.0)
    s = min(100, h // 2, w // 2)
    y, x = (h - s) // 2, (w - s) // 2
    g[y:y + s, x:x + s] = 96 + (synth.crude_face(s).astype(np.float64) - 96) / 5
    for _ in range(3):   # 5 x 5 box blur, three times
        p = np.pad(g, 2, mode="edge")
        g = sum(p[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) / 25.0
    return g.round().astype(np.uint8)


def black_edge_frame(h: int = 240, w: int = 320) -> np.ndarray:
    """Black on the left, bright rectangles on the right: the edge column of each rectangle is the last BLACK column, so windows
    whose pruning rectangle ends there have s >= 100 but sq = 0 < 20."""
    g = np.zeros((h, w), np.uint8)
    g[h // 8:h - h // 8, w // 2:w - w // 8] = 220
    g[h // 3:h // 2, w // 4:w // 3] = 180
    return g
