"""Premises of the mixed-size cases (tests/mixed_cases.py), stated on the CPU with the oracle alone: for each of the four cascades at
least 8 of the 11 frames give rectangles, there are at least 40 in total, the two tiny frames give none — and the counts per frame
are the ones the module records, in both arithmetic profiles."""
import os

import pytest

import mixed_cases as mc
from clfacedetection_amd.api import DATA_DIR
from oracle.oracle import load_vjc


def _arrays(name):
    return load_vjc(os.path.join(DATA_DIR, f"haarcascade_{name}.vjc"))


def _check(counts, want):
    assert counts == want
    assert sum(1 for n in counts if n > 0) >= 8 and sum(counts) >= 40
    assert all(counts[i] == 0 for i in mc.TINY)


def test_the_frames_are_the_sizes_the_cases_name():
    fr = mc.frames()
    assert [(f.shape[1], f.shape[0]) for f in fr] == mc.SIZES and len(fr) == 11
    assert sum(1 for w, _ in mc.SIZES if w % 4) >= 5
    assert mc.SIZES[0] == mc.SIZES[8] and len(set(mc.SIZES)) == 10


@pytest.mark.parametrize("name", list(mc.EXPECTED))
def test_opencv_profile_premises(oracle, name):
    res = mc.oracle_cv(oracle, name, _arrays(name))
    _check([len(r) for r, _ in res], mc.EXPECTED[name][0])


@pytest.mark.parametrize("name", [n for n in mc.EXPECTED if mc.EXPECTED[n][1] is not None])
def test_clod_profile_premises(oracle, name):
    res = mc.oracle_clod(oracle, name, _arrays(name))
    _check([len(r) for r, _ in res], mc.EXPECTED[name][1])
