"""Cases of the OpenCV profile's region pass (vj_detect_opencv_rois / vj_detect_opencv_chain), shared by tests/test_cv_rois_cpu.py —
which states their premises on the CPU: the oracle alone finds rectangles on three scales, at least 10 per case, and a region whose
result is not the frame's own detections restricted to it — and tests/test_gpu_cv_rois.py, which runs them on the device.

The checker is the existing oracle on numpy crops: the contract of vj_detect_opencv_rois is "what vj_detect_opencv returns for the
region as a sub-image", and Oracle.detect_opencvlike on frame[y:y + h, x:x + w] is that."""
from __future__ import annotations

import numpy as np

from clfacedetection_amd import synth

FRAME_H, FRAME_W = 180, 240


def faces_frame(seed: int, h: int = FRAME_H, w: int = FRAME_W, n_faces: int = 5) -> np.ndarray:
    """Crude faces of several sizes on a textured background (the content of tests/scale_image_oracle.py's cases)."""
    rng = np.random.default_rng(seed)
    f = synth.frame("smooth", seed, h, w).copy()
    for _ in range(n_faces):
        s = int(rng.integers(max(24, min(h, w) // 8), max(25, min(h, w) // 2)))
        y, x = int(rng.integers(0, h - s + 1)), int(rng.integers(0, w - s + 1))
        f[y:y + s, x:x + s] = synth.crude_face(s)
    return f


# Regions of a FRAME_W x FRAME_H frame as (x, y, w, h), the same geometry for every case: odd origins, every frame edge touched,
# overlaps, the whole frame, regions too small for any scale of any shipped cascade (a window of 20 needs more than 30 pixels), and a
# dozen different sizes in one call.
REGIONS = [
    (0, 0, FRAME_W, FRAME_H),            # the whole frame
    (0, 0, 131, 97),                     # touches the top and left edges
    (FRAME_W - 141, 0, 141, 111),        # top and right
    (0, FRAME_H - 103, 127, 103),        # bottom and left
    (FRAME_W - 150, FRAME_H - 120, 150, 120),   # bottom and right
    (37, 21, 155, 133),                  # odd origin, overlaps all of the above
    (51, 33, 101, 99),                   # inside the last one
    (13, 7, 211, 61),                    # wide and flat
    (101, 5, 67, 171),                   # tall and narrow
    (5, 3, 29, 29),                      # too small for any scale
    (199, 150, 31, 22),                  # too small, at an odd origin
    (63, 41, 88, 88),
    (17, 59, 120, 110),
]

# name -> (cascade, seeds of faces_frame, keyword arguments of the detection).  The seeds were chosen on the CPU so that the premises
# above hold for every case (tests/test_cv_rois_cpu.py).
CASES = {
    "stumps": ("frontalface_alt", [1, 2, 3], {}),
    "two_node_trees": ("frontalface_alt2", [1, 2, 3], {}),
    "stage_tree": ("frontalface_alt_tree", [2, 9, 10], {}),
    "tilted": ("mcs_mouth", [2, 3, 4], {}),
    "eye": ("eye", [1, 2, 3], {}),
    "stumps_sf125_min": ("frontalface_alt", [4, 5], {"scale_factor": 1.25, "min_size": (30, 30)}),
}


def case_frames(name: str) -> np.ndarray:
    return np.stack([faces_frame(s) for s in CASES[name][1]])


def case_rois(name: str) -> np.ndarray:
    """Rows of (frame, x, y, w, h): every region of REGIONS in every frame of the case, frames interleaved (the list is NOT sorted by
    frame: the call must not depend on that)."""
    n = len(CASES[name][1])
    return np.array([(f, *r) for r in REGIONS for f in range(n)], np.int32)


def crop(frames, roi) -> np.ndarray:
    f, x, y, w, h = (int(v) for v in roi)
    return frames[f][y:y + h, x:x + w]


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


def oracle_rois(oracle, a, frames, rois, **kw):
    """Per region: (rectangles, stats) of the oracle on the crop."""
    return [oracle.detect_opencvlike(a, np.ascontiguousarray(crop(frames, r)), **kw) for r in rois]


# The chain: frontalface_alt2 then a second cascade on drawn-faces frames (the frames of g_alt2_eye_3 in tests/cases.py: synth kind
# "faces", 360 x 640).  haarcascade_eye finds only a handful of rectangles inside drawn faces in this arithmetic (seeds 2 and 5: three
# behind the grouped faces; seed 1: six behind the raw candidates), so it stays as the BASELINE config 5 pair and mcs_lefteye, which
# finds ten and more per frame, carries the weight.  (first, second, seeds, min_neighbors of the first)
CHAIN_H, CHAIN_W = 360, 640
CHAIN_CASES = {
    "alt2_eye_grouped": ("frontalface_alt2", "eye", [2, 5], 3),
    "alt2_eye_raw": ("frontalface_alt2", "eye", [1], 0),
    "alt2_lefteye_grouped": ("frontalface_alt2", "mcs_lefteye", [1, 2, 3], 3),
    "alt2_lefteye_raw": ("frontalface_alt2", "mcs_lefteye", [2], 0),
    "alt2_tilted_grouped": ("frontalface_alt2", "mcs_mouth", [1, 2], 3),   # a second cascade with tilted nodes behind one without
}


def chain_frames(name: str) -> np.ndarray:
    return np.stack([synth.frame("faces", s, CHAIN_H, CHAIN_W) for s in CHAIN_CASES[name][2]])


def oracle_chain(oracle, a1, a2, frames, min_neighbors):
    """-> (regions as rows of (frame, x, y, w, h), per-region (rects, stats) of the second cascade): the first cascade's raw
    candidates in the library's order (frame, scale_idx, y, x), grouped per frame when min_neighbors != 0."""
    regions = []
    for f in range(len(frames)):
        r, _ = oracle.detect_opencvlike(a1, frames[f])
        r = r[np.lexsort((r["x"], r["y"], r["scale_idx"]))]
        xywh = np.array([[v["x"], v["y"], v["w"], v["h"]] for v in r], np.int32).reshape(-1, 4)
        if min_neighbors:
            xywh, _ = oracle.group_rectangles(xywh, max(min_neighbors, 1))
        regions += [(f, *map(int, q)) for q in xywh]
    regions = np.array(regions, np.int32).reshape(-1, 5)
    return regions, oracle_rois(oracle, a2, frames, regions)
