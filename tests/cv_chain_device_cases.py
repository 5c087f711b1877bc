"""Cases of vj_detect_opencv_chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE) beyond tests/cv_rois_cases.py's CHAIN_CASES, shared by
tests/test_cv_chain_device_cpu.py — which states their premises on the oracle alone — and tests/test_gpu_cv_chain_device.py.  All
frames are 360 x 640 (cc.CHAIN_H x cc.CHAIN_W)."""
from __future__ import annotations

import numpy as np

import cv_rois_cases as cc
from clfacedetection_amd import synth

# A stage tree as the second cascade, behind the grouped faces of frontalface_alt2: 15 rectangles in 9 regions, and windows that
# enter the tree's last stage.
TREE_CASE = ("frontalface_alt2", "frontalface_alt_tree", [3, 4], 3)

# Frames that give nothing, between frames that do: a constant frame (no raw candidate) and a smooth one (one raw candidate, so
# no group at min_neighbors 3).  With max_subbatch 1 a sub-batch without any region occurs.
NOTHING_CASE = ("frontalface_alt2", "mcs_lefteye")

# Raw candidates of frontalface_alt2 per frame, by seed: what "group_max" 100 lets the device group (seed 2 only) and 96 does not
RAW_COUNTS = {2: 97, 1: 120, 3: 185}
GROUP_MAX_SEEDS = [2, 1, 3]


def faces(seed: int) -> np.ndarray:
    return synth.frame("faces", seed, cc.CHAIN_H, cc.CHAIN_W)


def tree_frames() -> np.ndarray:
    return np.stack([faces(s) for s in TREE_CASE[2]])


def constant_frame() -> np.ndarray:
    return np.full((cc.CHAIN_H, cc.CHAIN_W), 128, np.uint8)


def smooth_frame() -> np.ndarray:
    return synth.frame("smooth", 1, cc.CHAIN_H, cc.CHAIN_W)


def nothing_frames() -> np.ndarray:
    return np.stack([faces(2), constant_frame(), smooth_frame(), faces(5)])


def group_max_frames() -> np.ndarray:
    return np.stack([faces(s) for s in GROUP_MAX_SEEDS])
