"""ctypes view of tests/scale_image_oracle.c — the test restatement of CV_HAAR_SCALE_IMAGE (8-bit bilinear resize + the level
loop with the cascade at base size on every grid position).  Compiled with gcc and oracle/Makefile's flags on first use, into a
temporary directory (nothing is written to the tree)."""
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
        out = os.path.join(tempfile.mkdtemp(prefix="scale_image_oracle_"), "libscaleimageoracle.so")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, os.path.join(HERE, "scale_image_oracle.c"), "-lm"],
                       check=True, capture_output=True)
        L = C.CDLL(out)
        L.si_resize_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.si_resize_linear.restype = None
        L.si_level_verdicts.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.POINTER(_OcStats)]
        L.si_level_verdicts.restype = C.c_long
        L.si_detect_scale_image.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                            C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_OcStats), C.POINTER(C.c_int), C.c_void_p]
        L.si_detect_scale_image.restype = C.c_int
        _LIB = L
    return _LIB


def resize_linear(gray: np.ndarray, dst_w: int, dst_h: int) -> np.ndarray:
    """cvResize(gray, dst, CV_INTER_LINEAR) as restated in DESIGN.md §4.8: (dst_h, dst_w) uint8."""
    assert gray.dtype == np.uint8 and gray.ndim == 2
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    d = np.empty((dst_h, dst_w), np.uint8)
    _lib().si_resize_linear(g.ctypes.data, w, h, g.strides[0], d.ctypes.data, dst_w, dst_h, d.strides[0])
    return d


def _stats(st, c):
    return {"windows": int(st.windows), "stump_evals": int(st.stump_evals), "stage_entered": [int(v) for v in st.stage_entered[:c.n_stages]]}


def level_verdicts(c: CascadeArrays, gray: np.ndarray, ystep: int = 2):
    """cvRunHaarClassifierCascadeSum's result (> 0 pass, 0 / -i reject) at every position y, x = 0, ystep, ... < size - window of
    `gray` with the cascade at scale 1: an (ny, nx) int array, and the stats of evaluating all of them."""
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    ny, nx = len(range(0, h - c.win_h, ystep)), len(range(0, w - c.win_w, ystep))
    v = np.zeros((max(ny, 0), max(nx, 0)), np.int32)
    s, keep = Oracle._cstruct(c)
    st = _OcStats()
    n = _lib().si_level_verdicts(C.byref(s), g.ctypes.data, w, h, g.strides[0], ystep, v.ctypes.data, C.byref(st))
    assert n == v.size
    return v, _stats(st, c)


def detect_scale_image(c: CascadeArrays, gray: np.ndarray, min_size=(0, 0), scale_factor: float = 1.1, cap: int = 1 << 20):
    """cvHaarDetectObjects(flags = CV_HAAR_SCALE_IMAGE, min_neighbors = 0) restated.  Returns (rects, stats); stats["levels"] is the
    list of the evaluated levels' (w, h)."""
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    s, keep = Oracle._cstruct(c)
    out = np.zeros(cap, _RECT_DT)
    n_total, n_levels = C.c_int(0), C.c_int(0)
    sizes = np.zeros((64, 2), np.int32)
    st = _OcStats()
    n = _lib().si_detect_scale_image(C.byref(s), g.ctypes.data, w, h, g.strides[0], int(min_size[0]), int(min_size[1]), float(scale_factor),
                                     out.ctypes.data, cap, C.byref(n_total), C.byref(st), C.byref(n_levels), sizes.ctypes.data)
    assert n == n_total.value, "oracle rectangle buffer too small"
    d = _stats(st, c)
    d["levels"] = [tuple(int(v) for v in sizes[k]) for k in range(min(n_levels.value, 64))]
    d["n_levels"] = n_levels.value
    return out[:n], d


def faces_frame(seed: int, h: int, w: int, n_faces: int = 4) -> np.ndarray:
    """Synthetic content with crude faces of several sizes on a textured background: hits on several levels of the pyramid."""
    from clfacedetection_amd import synth
    rng = np.random.default_rng(seed)
    f = synth.frame("smooth", seed, h, w).copy()
    for _ in range(n_faces):
        s = int(rng.integers(max(24, min(h, w) // 8), max(25, min(h, w) // 2)))
        y, x = int(rng.integers(0, h - s + 1)), int(rng.integers(0, w - s + 1))
        f[y:y + s, x:x + s] = synth.crude_face(s)
    return f


def face_grid_frame(seed: int, h: int = 240, w: int = 320) -> np.ndarray:
    """Three crude faces of about 90 pixels and twelve of about 44, side by side: hits on the levels of factor 2 and 4, enough of them
    for scale_factor = 2.0 (whose few levels leave a random layout with a handful of rectangles)."""
    from clfacedetection_amd import synth
    rng = np.random.default_rng(seed)
    f = synth.frame("smooth", seed, h, w).copy()
    for k in range(3):
        s = int(rng.integers(78, 100))
        f[4:4 + s, 2 + 104 * k:2 + 104 * k + s] = synth.crude_face(s)
    for y0 in (110, 170):
        for k in range(6):
            s = int(rng.integers(38, 50))
            f[y0:y0 + s, 2 + 52 * k:2 + 52 * k + s] = synth.crude_face(s)
    return f


# What tests/test_gpu_scale_image.py runs, chosen on the CPU (tests/test_scale_image_cpu.py checks the premises: at least 10 raw
# rectangles and three levels per frame, and a result that differs from the scale-cascade path's): cascade -> seeds of faces_frame
FRAME_H, FRAME_W = 180, 240
CASES = {
    "frontalface_alt": [1, 2, 3, 4, 5, 6, 7, 8, 9],      # stumps; the batch of 9 distinct frames
    "frontalface_default": [1, 2, 7],
    "frontalface_alt2": [1, 2, 3],                       # two-node trees
    "frontalface_alt_tree": [2, 9, 10],                  # stage tree
    "mcs_mouth": [2, 3, 4],                              # tilted features
}
# (frontalface_alt, seed, keyword arguments): other scale factors, a min_size that skips leading levels
PARAM_CASES = [(1, {"scale_factor": 1.25}), (7, {"min_size": (40, 40)}), (7, {"min_size": (30, 30), "scale_factor": 1.25})]
GRID_SEED = 3                                            # face_grid_frame for scale_factor = 2.0 (the area branch, ystep = 1)


def case_frames(casc: str) -> np.ndarray:
    return np.stack([faces_frame(s, FRAME_H, FRAME_W) for s in CASES[casc]])
