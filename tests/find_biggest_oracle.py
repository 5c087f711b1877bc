"""ctypes view of tests/find_biggest_oracle.c — the test restatement of CV_HAAR_FIND_BIGGEST_OBJECT (the descending scale loop, the
grouping after each scale, the scanROI and the final grouping).  Compiled with gcc and oracle/Makefile's flags on first use, into a
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


class _FbInfo(C.Structure):
    _fields_ = [("found", C.c_int32), ("result", C.c_int32 * 4), ("neighbors", C.c_int32), ("n_factors", C.c_int32),
                ("scales_evaluated", C.c_int32), ("first_hit_scale", C.c_int32), ("roi_scales", C.c_int32), ("roi_candidates", C.c_int32),
                ("roi", C.c_int32 * 4), ("roi_clamped", C.c_int32), ("min_size", C.c_int32 * 2)]


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="find_biggest_oracle_"), "libfindbiggestoracle.so")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, os.path.join(HERE, "find_biggest_oracle.c"), "-lm"],
                       check=True, capture_output=True)
        L = C.CDLL(out)
        L.fb_detect_biggest.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_OcStats), C.POINTER(_FbInfo)]
        L.fb_detect_biggest.restype = C.c_int
        _LIB = L
    return _LIB


def detect_biggest(c: CascadeArrays, gray: np.ndarray, min_size=(0, 0), scale_factor: float = 1.1, min_neighbors: int = 3,
                   rough: bool = False, cap: int = 1 << 18):
    """cvHaarDetectObjects(flags = CV_HAAR_FIND_BIGGEST_OBJECT [| CV_HAAR_DO_ROUGH_SEARCH]) restated.  Returns (result, stats):
    result is None or (x, y, w, h, neighbors); stats holds windows / stage_entered / stump_evals and, for inspection, n_factors,
    scales_evaluated, first_hit_scale (-1: never), roi_scales, roi_candidates, roi, roi_clamped, min_size and `candidates`: the raw
    list in allCandidates' order (scale_idx -2 marks the pushed maxRect)."""
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    s, keep = Oracle._cstruct(c)
    out = np.zeros(cap, _RECT_DT)
    n_total = C.c_int(0)
    st, info = _OcStats(), _FbInfo()
    n = _lib().fb_detect_biggest(C.byref(s), g.ctypes.data, w, h, g.strides[0], int(min_size[0]), int(min_size[1]), float(scale_factor),
                                 int(min_neighbors), int(bool(rough)), out.ctypes.data, cap, C.byref(n_total), C.byref(st), C.byref(info))
    assert n == n_total.value, "oracle candidate buffer too small"
    d = {"windows": int(st.windows), "stump_evals": int(st.stump_evals), "stage_entered": [int(v) for v in st.stage_entered[:c.n_stages]],
         "n_factors": info.n_factors, "scales_evaluated": info.scales_evaluated, "first_hit_scale": info.first_hit_scale,
         "roi_scales": info.roi_scales, "roi_candidates": info.roi_candidates, "roi": tuple(info.roi), "roi_clamped": bool(info.roi_clamped),
         "min_size": tuple(info.min_size), "candidates": out[:n].copy()}
    res = (info.result[0], info.result[1], info.result[2], info.result[3], info.neighbors) if info.found else None
    return res, d


# ---- what tests/test_gpu_find_biggest.py runs; tests/test_find_biggest_cpu.py checks the premises on the oracle alone
FRAME_H, FRAME_W = 180, 240
FACELESS = ("smooth", 41), ("smooth", 42)        # synth.frame(kind, seed, FRAME_H, FRAME_W): no candidate at all


def frames_for(casc: str) -> np.ndarray:
    """The frames of a cascade's case: scale_image_oracle's faces_frame seeds; frontalface_alt: nine distinct frames, two of them
    faceless (positions 2 and 6)."""
    import scale_image_oracle as so
    from clfacedetection_amd import synth
    fr = [so.faces_frame(s, FRAME_H, FRAME_W) for s in CASES[casc]]
    if casc == "frontalface_alt":
        fr.insert(2, synth.frame(FACELESS[0][0], FACELESS[0][1], FRAME_H, FRAME_W))
        fr.insert(6, synth.frame(FACELESS[1][0], FACELESS[1][1], FRAME_H, FRAME_W))
    return np.stack(fr)


CASES = {
    "frontalface_alt": [1, 2, 3, 4, 5, 6, 7],            # stumps; with the two faceless frames the batch of nine
    "frontalface_default": [1, 2, 7],
    "frontalface_alt2": [1, 2, 3],                       # two-node trees
    "frontalface_alt_tree": [2, 9, 10],                  # stage tree
    "mcs_mouth": [2, 3, 4],                              # tilted features
}
HIGH_NEIGHBORS = 20                                      # some frame of the frontalface_alt batch never groups at this value
MIN_SIZE_BREAK = (150, 150)                              # breaks before any hit
MIN_SIZE_CASE = (85, 85)                                # the faceless frames break after a few scales; the others find their face first


def big_face_frame(seed: int = 5, h: int = 480, w: int = 640, size: int = 300) -> np.ndarray:
    """One 480 x 640 frame with a crude face of about 300 pixels: the scanROI's scales fall where the plain path runs LDS tiles."""
    from clfacedetection_amd import synth
    f = synth.frame("smooth", seed, h, w).copy()
    f[100:100 + size, 200:200 + size] = synth.crude_face(size)
    return f


def last_scale_frame(h: int = 120, w: int = 160, size: int = 20, y: int = 40, x: int = 50) -> np.ndarray:
    """A crude face of the cascade's base size on a smooth frame: with LAST_SCALE_CASES the first group forms only after the LAST
    scale of the walk (scale_idx 0), so the grouping step that follows it pushes maxRect right before the final grouping."""
    from clfacedetection_amd import synth
    f = synth.frame("smooth", 3, h, w).copy()
    f[y:y + size, x:x + size] = synth.crude_face(size)
    return f


LAST_SCALE_CASES = [(1.1, 9), (1.25, 5)]                 # (scale_factor, min_neighbors)
