"""ctypes view of tests/roc_oracle.c — the test restatement of cvHaarDetectObjectsForROC with outputRejectLevels (the per-window
run returning (result, stage_sum), the ROC invoker, the level loop with maxSize, groupRectangles' level overload).  Compiled
with gcc on first use, into a temporary directory, like tests/scale_image_oracle.py (nothing is written to the tree)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle.oracle import _RECT_DT, CascadeArrays, Oracle, _OcCascade
from scale_image_oracle import CFLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# Frames of the GPU cases (tests/test_gpu_roc.py), chosen on the CPU: seeds of scale_image_oracle.faces_frame at 180 x 240.
# tests/test_roc_cpu.py asserts the premises on PREMISE_SEEDS: per linear cascade every one of its three near-miss levels
# occurs over those seeds, and every one of those frames has at least 5 near-miss rejects.  frontalface_default: seeds 1 and 2
# show levels 23 and 24 only; 3 is the first seed of a search upwards from 3 that shows level 22 as well.
FRAME_H, FRAME_W = 180, 240
CASES = {
    "frontalface_alt": [1, 2, 3, 4, 5, 6, 7, 8, 9],     # 22 stump stages; the batch of 9 distinct frames
    "frontalface_default": [1, 2, 3],                   # 25 stump stages
    "frontalface_alt2": [1, 2, 3],                      # 20 stages of two-node trees
    "mcs_mouth": [2, 3, 4],                             # 17 stages, tilted features
    "frontalface_alt_tree": [2, 9, 10],                 # 47 stages, a stage tree: accepted windows only
}
PREMISE_SEEDS = {"frontalface_alt": [1, 2, 3], "frontalface_default": [1, 2, 3], "frontalface_alt2": [1, 2, 3], "mcs_mouth": [2, 3, 4]}
# a wide, low frame of heavy_cases' dots content under a survivor cascade of 3 all-pass stages and a selective one: every grid
# position reaches the last stage and is reported (level 3 or 4); a row of level 0 has 690 stage-0 survivors, so the wave's queue
# (CV_QCAP = 320 entries, flushed above CV_QCAP - 64) is flushed in the middle of the row
WIDE_SPEC = ("dots", 7000, 64, 1400, 22)
WIDE_FORMS = ("stumps", "trees")
CV_QCAP = 320


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="roc_oracle_"), "librocoracle.so")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, os.path.join(HERE, "roc_oracle.c"), "-lm"],
                       check=True, capture_output=True)
        L = C.CDLL(out)
        L.roc_detect.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.roc_detect.restype = C.c_int
        L.roc_group.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]
        L.roc_group.restype = C.c_int
        _LIB = L
    return _LIB


def detect_roc(c: CascadeArrays, gray: np.ndarray, min_size=(0, 0), max_size=(0, 0), scale_factor: float = 1.1, cap: int = 1 << 20):
    """cvHaarDetectObjectsForROC(flags = CV_HAAR_SCALE_IMAGE, min_neighbors = 0, outputRejectLevels = true) restated.  Returns
    (rects, levels, weights, n_levels) in the reference's order, which is sorted by (scale_idx, y, x)."""
    g = np.ascontiguousarray(gray)
    h, w = g.shape
    s, keep = Oracle._cstruct(c)
    out = np.zeros(cap, _RECT_DT)
    levels = np.zeros(cap, np.int32)
    weights = np.zeros(cap, np.float64)
    n_total, n_levels = C.c_int(0), C.c_int(0)
    n = _lib().roc_detect(C.byref(s), g.ctypes.data, w, h, g.strides[0], int(min_size[0]), int(min_size[1]), int(max_size[0]),
                          int(max_size[1]), float(scale_factor), out.ctypes.data, levels.ctypes.data, weights.ctypes.data, cap,
                          C.byref(n_total), C.byref(n_levels))
    assert n == n_total.value, "oracle buffers too small"
    return out[:n].copy(), levels[:n].copy(), weights[:n].copy(), n_levels.value


def group_levels(xywh: np.ndarray, levels, weights, group_threshold: int, eps: float = 0.2):
    """groupRectangles(rectList, rejectLevels, levelWeights, groupThreshold, eps) restated: (n, 4) ints in detection order with
    their levels and weights -> (grouped (m, 4), levels (m,), weights (m,))."""
    r = np.ascontiguousarray(xywh, np.int32).reshape(-1, 4).copy()
    lv = np.ascontiguousarray(levels, np.int32).copy()
    lw = np.ascontiguousarray(weights, np.float64).copy()
    assert len(r) == len(lv) == len(lw)
    m = _lib().roc_group(r.ctypes.data, lv.ctypes.data, lw.ctypes.data, len(r), int(group_threshold), float(eps))
    return r[:m], lv[:m], lw[:m]


def case_frames(casc: str) -> np.ndarray:
    from scale_image_oracle import faces_frame
    return np.stack([faces_frame(s, FRAME_H, FRAME_W) for s in CASES[casc]])


def first_stages(c: CascadeArrays, k: int) -> CascadeArrays:
    """The first k stages of a linear cascade as a cascade of its own."""
    assert 1 <= k <= c.n_stages and (c.stage_next == -1).all()
    t = CascadeArrays()
    t.win_w, t.win_h, t.name = c.win_w, c.win_h, f"{c.name}_first{k}"
    nt = int(c.stage_first_tree[k - 1] + c.stage_n_trees[k - 1])
    nn = int(c.tree_first_node[nt - 1] + c.tree_n_nodes[nt - 1])
    na = int(c.tree_first_alpha[nt]) if nt < c.n_trees else c.n_alpha
    t.stage_first_tree, t.stage_n_trees, t.stage_threshold = c.stage_first_tree[:k].copy(), c.stage_n_trees[:k].copy(), c.stage_threshold[:k].copy()
    t.stage_parent, t.stage_next = c.stage_parent[:k].copy(), c.stage_next[:k].copy()
    t.stage_child = c.stage_child[:k].copy()
    t.stage_child[k - 1] = -1
    t.tree_first_node, t.tree_n_nodes, t.tree_first_alpha = c.tree_first_node[:nt].copy(), c.tree_n_nodes[:nt].copy(), c.tree_first_alpha[:nt].copy()
    t.node_rect, t.node_weight = c.node_rect[:nn * 12].copy(), c.node_weight[:nn * 3].copy()
    t.node_threshold, t.node_left, t.node_right = c.node_threshold[:nn].copy(), c.node_left[:nn].copy(), c.node_right[:nn].copy()
    t.node_tilted = c.node_tilted[:nn].copy() if len(c.node_tilted) == c.n_nodes else c.node_tilted.copy()
    t.alpha = c.alpha[:na].copy()
    return t


def wide_cascade(form: str) -> CascadeArrays:
    from cases import survivor_cascade
    return survivor_cascade(form, 3)
