"""cv::equalizeHist as restated in tests/equalize_oracle.py: the known answers of DESIGN.md §4.15, the properties of the table, and
the premise of the detect tests of tests/test_gpu_equalize.py — equalizing the frames of tests/mixed_cases.py changes what the
oracle finds in them, in both arithmetic profiles."""
import os

import numpy as np
import pytest

import equalize_oracle as eo
import mixed_cases as mc
from clfacedetection_amd import synth
from clfacedetection_amd.api import DATA_DIR
from oracle.oracle import load_vjc


def test_known_answers():
    ramp = np.arange(7, dtype=np.uint8)[None]                  # scale = 255 / 6 = 42.5: 42.5, 127.5 and 212.5 go to the even integer
    assert eo.equalize(ramp).tolist() == [[0, 42, 85, 128, 170, 212, 255]]
    assert eo.equalize(np.array([[10, 20, 30, 40]], np.uint8)).tolist() == [[0, 85, 170, 255]]
    assert eo.equalize(np.array([[10, 20], [30, 40]], np.uint8)).tolist() == [[0, 85], [170, 255]]
    for v in (0, 7, 255):                                      # a constant image is unchanged
        c = np.full((3, 5), v, np.uint8)
        assert eo.lut(c) is None and np.array_equal(eo.equalize(c), c)
    assert eo.equalize(np.array([[3]], np.uint8)).tolist() == [[3]]
    two = np.array([[5, 5, 5, 200]], np.uint8)                 # two values: the lower one to 0, the upper one to 255
    assert eo.equalize(two).tolist() == [[0, 0, 0, 255]]


def test_int_to_float_rounds_to_nearest_even_above_2_pow_24():
    """(float)sum is inexact above 2^24: the conversion the restatement relies on rounds to nearest, ties to even, in one step."""
    assert np.float32(2**24 + 1) == np.float32(2**24) and np.float32(2**24 + 3) == np.float32(2**24 + 4)
    assert np.float32(2**25 + 2) == np.float32(2**25) and np.float32(2**25 + 6) == np.float32(2**25 + 8)


@pytest.mark.parametrize("kind", ["noise", "smooth", "blocks", "faces"])
def test_the_table_is_monotone_and_ends_at_255(kind):
    for seed, (h, w) in enumerate([(1, 2), (5, 9), (61, 131), (180, 240)]):
        g = synth.frame(kind, 3 + seed, h, w)
        t = eo.lut(g)
        if t is None:
            assert len(np.unique(g)) == 1
            continue
        present = np.unique(g)
        assert np.all(np.diff(t.astype(int)) >= 0) and t[present[0]] == 0 and t[present[-1]] == 255 and t[255] == 255
        e = eo.equalize(g)
        assert e.min() == 0 and e.max() == 255 and e.shape == g.shape
        assert np.all(np.diff(e.reshape(-1)[np.argsort(g.reshape(-1), kind="stable")].astype(int)) >= 0)   # the order of the pixels is kept


def _counts(res):
    return [len(r) for r, _ in res]


def test_equalization_changes_what_the_detector_finds(oracle):
    """The premise of the flag's detect tests: on the eleven frames of tests/mixed_cases.py with frontalface_alt the rectangle lists
    with and without equalization differ in at least 8 frames, in both profiles, and the equalized lists hold at least 40."""
    a = load_vjc(os.path.join(DATA_DIR, "haarcascade_frontalface_alt.vjc"))
    eq = eo.equalized(mc.frames())
    for plain, mine in ((mc.oracle_cv(oracle, "frontalface_alt", a), [oracle.detect_opencvlike(a, f) for f in eq]),
                        (mc.oracle_clod(oracle, "frontalface_alt", a), [oracle.detect(a, f) for f in eq])):
        differ = sum(1 for (r0, _), (r1, _) in zip(plain, mine) if mc.rows(r0) != mc.rows(r1))
        print("rectangles per frame as is", _counts(plain), "equalized", _counts(mine), "frames that differ", differ)
        assert differ >= 8 and sum(_counts(mine)) >= 40
        assert all(_counts(mine)[i] == 0 for i in mc.TINY)
