"""Cases of the stream-ordering tests ("Sharing a process with PyTorch"), shared by tests/test_stream_order_cpu.py —
which states their premises on the CPU with the oracles and restatements alone — and tests/test_gpu_stream_order.py, which runs
them on the device with torch work pending on the memory the calls are given.

A is what the memory holds before that work, B what it holds after it: frames 0 and 1 of prep_cases.e2e_prepared (240 x 180, the
smallest setup in the project where the detector finds enough) for everything that takes a prepared frame, frames 0 and 1 of
prep_cases.e2e_frames / extract_cases.e2e_bgr (432 x 324) for preprocess and extract.  A call that read its input too early returns
A's result; every case therefore needs A's and B's results to differ, which is what the CPU file asserts."""
from __future__ import annotations

import numpy as np

import canny_oracle as co
import clod_window_oracle as cw
import equalize_oracle as eo
import extract_cases as ec
import prep_cases as pc
import run_window_oracle as rw
import scale_image_oracle as so

A, B = 0, 1
N_WINDOWS = 1500                                     # of each case list, as tests/test_gpu_prep.py::test_window_lists takes them
RESIZE_TO = (101, 77)                                # resize_linear's destination: both sides odd, neither a divisor of 240 x 180
EXTRACT_SIZE = ec.MANY_SIZE
EXTRACT_SCALE = ec.MANY_SCALE                        # regions in the prepared frame's coordinates, cut from the 432 x 324 source
# (frame, x, y, w, h): inside, across the left and the bottom edge, the whole frame
EXTRACT_RECTS = [(0, 20, 30, 60, 60), (0, 100, 50, 80, 70), (0, -5, 120, 50, 50), (0, 150, 140, 70, 60), (0, 0, 0, 240, 180)]
PREP_KW = dict(size=pc.E2E_SIZE, equalize=True)


def prepared(oracle, which: int) -> np.ndarray:
    return pc.e2e_prepared(oracle)[which]


def detect_lists(oracle, a, profile: str) -> list:
    """[(rectangles, stats)] of the three prepared frames; the keys and values tests/test_gpu_prep.py caches."""
    want = pc.e2e_prepared(oracle)
    if profile == "clod":
        return pc.once("clod", lambda: [oracle.detect(a, f) for f in want])
    return pc.once("cv", lambda: [oracle.detect_opencvlike(a, f) for f in want])


def cv_windows(a) -> np.ndarray:
    return rw.full_list(a, frame=0)[:N_WINDOWS]


def clod_windows(a) -> np.ndarray:
    return cw.full_list(a, frame=0)[:N_WINDOWS]


def cv_verdicts(oracle, a, which: int):
    return pc.once(("so_cv_windows", which), lambda: rw.run_windows(a, [prepared(oracle, which)], cv_windows(a), rw.case_scales()))


def clod_verdicts(oracle, a, which: int):
    return pc.once(("so_clod_windows", which), lambda: cw.run_windows(a, [prepared(oracle, which)], clod_windows(a), cw.case_scales()))


def canny(oracle, which: int) -> np.ndarray:
    return pc.once(("so_canny", which), lambda: co.canny(np.ascontiguousarray(prepared(oracle, which))))


def equalized(oracle, which: int) -> np.ndarray:
    return pc.once(("so_equalize", which), lambda: eo.equalize(np.ascontiguousarray(prepared(oracle, which))))


def resized(oracle, which: int) -> np.ndarray:
    return pc.once(("so_resize", which), lambda: so.resize_linear(np.ascontiguousarray(prepared(oracle, which)), *RESIZE_TO))


def extracted(oracle, which: int) -> np.ndarray:
    """extract_cases.restate of EXTRACT_RECTS on the colour source `which`."""
    return pc.once(("so_extract", which), lambda: ec.restate(oracle, [ec.e2e_bgr()[which]], EXTRACT_RECTS, EXTRACT_SIZE, scale=EXTRACT_SCALE))
