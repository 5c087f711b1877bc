"""Premises of tests/test_gpu_cv_rois_scale_image.py, stated on the CPU with the scale-image oracle alone
(scale_image_oracle.detect_scale_image on the crops of tests/cv_rois_cases.py): every case finds rectangles on at least six factor
numbers, so a test that passes on it cannot pass on empty results; the 2 x 2 mean path and the step-1 levels occur; and a region's
result is not the frame's result restricted to the region — a resized crop is not a crop of the resized frame, which is why the
regions need level images of their own.  The counts below were measured with this oracle; they are asserted as lower bounds."""
import functools
import os

import numpy as np
import pytest

import cv_rois_cases as cc
import scale_image_oracle as so
from clfacedetection_amd.api import DATA_DIR
from oracle.oracle import load_vjc

# case -> (rectangles, level images) over all regions
MEASURED = {"stumps": (275, 600), "two_node_trees": (238, 600), "stage_tree": (108, 600), "tilted": (95, 585), "eye": (14, 600),
            "stumps_sf125_min": (69, 130)}


@functools.lru_cache(maxsize=None)
def _arrays(name):
    return load_vjc(os.path.join(DATA_DIR, f"haarcascade_{name}.vjc"))


def oracle_crops(a, frames, rois, **kw):
    """Per region: (rectangles, stats) of the scale-image oracle on the crop."""
    return [so.detect_scale_image(a, np.ascontiguousarray(cc.crop(frames, r)), **kw) for r in rois]


def test_every_case_is_measured():
    assert set(MEASURED) == set(cc.CASES)


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cases_are_non_trivial(name):
    casc, seeds, kw = cc.CASES[name]
    a = _arrays(casc)
    frames, rois = cc.case_frames(name), cc.case_rois(name)
    res = oracle_crops(a, frames, rois, **kw)
    n = sum(len(r) for r, _ in res)
    levels = sum(st["n_levels"] for _, st in res)
    factors = {int(s) for r, _ in res for s in r["scale_idx"]}
    print(name, "rectangles", n, "level images", levels, "factor numbers", sorted(factors))
    assert n >= (1 if name == "eye" else 10)
    assert n >= MEASURED[name][0] and levels >= MEASURED[name][1]
    assert len(factors) >= 6, factors
    assert sum(st["windows"] for _, st in res) > 0
    # levels with ystep 1 (factor > 2) are evaluated, and some are hit
    assert any(w * 2 < int(roi[3]) for (_, st), roi in zip(res, rois) for w, h in st["levels"])
    # regions smaller than the window contribute nothing (the scale-image loop, unlike the scale-cascade one, takes a 29 x 29 region)
    r, st = so.detect_scale_image(a, np.ascontiguousarray(frames[0][3:3 + a.win_h - 1, 5:5 + 40]), **kw)
    assert len(r) == 0 and st["windows"] == 0 and st["n_levels"] == 0


def test_scale_factor_two_takes_the_2x2_mean_path():
    a = _arrays("frontalface_alt")
    frames, rois = cc.case_frames("stumps"), cc.case_rois("stumps")
    res = oracle_crops(a, frames, rois, scale_factor=2.0)
    n = sum(len(r) for r, _ in res)
    halves = sum(1 for (_, st), roi in zip(res, rois) for w, h in st["levels"] if 2 * w == int(roi[3]) and 2 * h == int(roi[4]))
    print("rectangles", n, "levels at exactly half their crop", halves)
    assert n >= 18 and n >= 10 and halves >= 12


def test_a_regions_result_is_not_the_frames_restricted_to_it():
    a = _arrays("frontalface_alt")
    frames = cc.case_frames("stumps")
    x, y, w, h = 37, 21, 155, 133
    mine, _ = so.detect_scale_image(a, np.ascontiguousarray(frames[0][y:y + h, x:x + w]))
    whole, _ = so.detect_scale_image(a, frames[0])
    inside = sorted((int(v["x"]) - x, int(v["y"]) - y, int(v["w"]), int(v["h"])) for v in whole
                    if v["x"] >= x and v["y"] >= y and v["x"] + v["w"] <= x + w and v["y"] + v["h"] <= y + h)
    assert len(mine) >= 1 and sorted((int(v["x"]), int(v["y"]), int(v["w"]), int(v["h"])) for v in mine) != inside
