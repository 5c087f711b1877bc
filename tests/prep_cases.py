"""Cases of vj_preprocess, shared by tests/test_prep_cpu.py — which checks the layout through ctypes and states the
premise of the end-to-end tests on the CPU with the oracles alone — and tests/test_gpu_prep.py, which runs them on the device.

The reference is the composition of the existing restatements, nothing new: oracle.bgr2gray, scale_image_oracle.resize_linear (the
identity when the size does not change) and equalize_oracle.equalize — of the RESIZED image."""
from __future__ import annotations

import numpy as np

import cv_rois_cases as cc
import equalize_oracle as eo
import mixed_cases as mc
import scale_image_oracle as so


def cv_round(v: float) -> int:
    return int(np.rint(np.float64(v)))          # half to even, as lrint


def dst_size(w: int, h: int, size=None, fx=None, fy=None):
    if size is not None:
        return int(size[0]), int(size[1])
    if fx is not None:
        return max(cv_round(w * fx), 1), max(cv_round(h * fy), 1)
    return w, h


def restate(oracle, img: np.ndarray, size=None, fx=None, fy=None, equalize=False) -> np.ndarray:
    """What vj_preprocess must write for one frame: vj_grayscale, vj_resize_linear, vj_equalize_hist as the tests restate them."""
    g = np.ascontiguousarray(img if img.ndim == 2 else oracle.bgr2gray(np.ascontiguousarray(img)))
    w, h = dst_size(g.shape[1], g.shape[0], size, fx, fy)
    if (w, h) != (g.shape[1], g.shape[0]):
        g = so.resize_linear(g, w, h)
    return eo.equalize(g) if equalize else g


# ---- the end-to-end cases: three 432 x 324 frames to 240 x 180 (factor 1.8: the bilinear path), equalized.  240 x 180 is the size
# the window-list restatements (tests/run_window_oracle.py, tests/clod_window_oracle.py) build their grids for.
E2E_SRC_W, E2E_SRC_H = 432, 324
E2E_SIZE = (240, 180)
E2E_SEEDS = (1, 2, 3)
CASC = "frontalface_alt"
_E2E = None
_E2E_PREP = {}


def e2e_frames() -> np.ndarray:
    """Built once; do not modify."""
    global _E2E
    if _E2E is None:
        _E2E = np.stack([cc.faces_frame(s, E2E_SRC_H, E2E_SRC_W, n_faces=5) for s in E2E_SEEDS])
        _E2E.setflags(write=False)
    return _E2E


def e2e_prepared(oracle, equalize=True) -> np.ndarray:
    """restate() of the end-to-end frames; computed once."""
    if equalize not in _E2E_PREP:
        p = np.stack([restate(oracle, f, size=E2E_SIZE, equalize=equalize) for f in e2e_frames()])
        p.setflags(write=False)
        _E2E_PREP[equalize] = p
    return _E2E_PREP[equalize]


_MIXED_PREP = {}


def mixed_prepared(oracle, equalize: bool) -> list:
    """restate() of the eleven frames of tests/mixed_cases.py at fx = fy = 0.5; computed once."""
    if equalize not in _MIXED_PREP:
        _MIXED_PREP[equalize] = [restate(oracle, f, fx=0.5, fy=0.5, equalize=equalize) for f in mc.frames()]
        for p in _MIXED_PREP[equalize]:
            p.setflags(write=False)
    return _MIXED_PREP[equalize]


_RES = {}


def once(key, fn):
    if key not in _RES:
        _RES[key] = fn()
    return _RES[key]
