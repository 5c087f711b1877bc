"""Cases of the mixed-size entry points (vj_detect_mixed, vj_detect_opencv_mixed), shared by tests/test_mixed_cases_cpu.py — which
states their premises on the CPU with the oracle alone — and tests/test_gpu_mixed.py, which runs them on the device.

Eleven frames: five widths that are no multiple of 4, two frames of one size, two frames too small for any scale of any shipped
cascade.  The checker is the existing oracle frame by frame: the contract of a mixed call is "the concatenation over i of what the
batched call returns for frames[i] alone"."""
from __future__ import annotations

import numpy as np

import cv_rois_cases as cc
from clfacedetection_amd import synth

SIZES = [(240, 180), (131, 97), (141, 111), (211, 61), (67, 171), (29, 29), (155, 133), (88, 88), (240, 180), (31, 22), (127, 103)]   # (w, h)
TINY = [5, 9]            # too small for any scale

# cascade -> rectangles per frame, as the oracle finds them on the CPU (tests/test_mixed_cases_cpu.py): (OpenCV profile, clod profile;
# None: the clod profile's oracle does not run the cascade — mcs_mouth has tilted features)
EXPECTED = {
    "frontalface_alt": ([47, 52, 49, 11, 22, 0, 46, 25, 67, 0, 34],) * 2,
    "frontalface_alt2": ([38, 41, 29, 7, 21, 0, 38, 13, 69, 0, 39],) * 2,
    "mcs_mouth": ([62, 16, 8, 19, 0, 0, 13, 5, 47, 0, 1], None),
    "frontalface_alt_tree": ([5, 5, 4, 5, 2, 0, 11, 2, 13, 0, 5], [8, 9, 5, 5, 3, 0, 13, 3, 24, 0, 8]),
}

_FRAMES = None


def frames() -> list:
    """Frame i: drawn faces on a textured background where a face fits, else the texture alone.  Built once; do not modify."""
    global _FRAMES
    if _FRAMES is None:
        _FRAMES = [cc.faces_frame(1 + i, h, w, n_faces=3) if min(h, w) >= 40 else synth.frame("smooth", 1 + i, h, w).copy()
                   for i, (w, h) in enumerate(SIZES)]
        for f in _FRAMES:
            f.setflags(write=False)
    return _FRAMES


_ORACLE = {}


def oracle_cv(oracle, name: str, a, **kw) -> list:
    """Per frame: (rectangles, stats) of Oracle.detect_opencvlike; computed once per (cascade, arguments)."""
    key = ("cv", name, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.detect_opencvlike(a, f, **kw) for f in frames()]
    return _ORACLE[key]


def oracle_clod(oracle, name: str, a, **kw) -> list:
    key = ("clod", name, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.detect(a, f, **kw) for f in frames()]
    return _ORACLE[key]


rows = cc.rows
