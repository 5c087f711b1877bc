"""ctypes view of tests/run_window_oracle.c — the test restatement of cvSetImagesForHaarClassifierCascade +
cvRunHaarClassifierCascadeSum for one window at an arbitrary double scale — and the window lists of the GPU cases
(tests/test_gpu_run_windows.py), whose premises tests/test_run_windows_cpu.py asserts.  Compiled with gcc on first use, into a
temporary directory, like tests/roc_oracle.py (nothing is written to the tree)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle.oracle import CascadeArrays, Oracle, _OcCascade
from scale_image_oracle import CFLAGS, faces_frame

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31

FRAME_H, FRAME_W = 180, 240
# the six cascades of the GPU cases -> seed of scale_image_oracle.faces_frame at 180 x 240.  The linear ones: the first seed from 1
# upwards whose union of window lists shows the premises (tests/test_run_windows_cpu.py searches the same way); the stage tree: the
# first with at least 10 results of each kind.  eye_tree_eyeglasses: the drawn faces have no eyes it accepts — no seed of 1 .. 399
# gives more than one pass a frame (eleven of them give a reject in one of its last three stages) —, so its seed is the first that
# shows the premise without the passes (eye_premises), and its passes and late stages are reached with start_stage instead
# (EYE_START_STAGES: 4, 460 and 19388 passes of the full list, rejects at every stage from the start on).
SEEDS = {
    "frontalface_alt": 1,
    "frontalface_default": 1,
    "frontalface_alt2": 1,
    "eye_tree_eyeglasses": 17,
    "mcs_mouth": 1,
    "frontalface_alt_tree": 14,
}
LINEAR = ("frontalface_alt", "frontalface_default", "frontalface_alt2", "eye_tree_eyeglasses", "mcs_mouth")
CHAIN_STEPS = (0, 3, 6, 9)          # members of the factor chain 1.1^k (the doubles of the enumeration: repeated multiplication)
OFF_CHAIN = (2.5, 1.37)             # 2.5: cvRound ties (20 * 2.5 = 50 exactly, 5 * 2.5 = 12.5, ...)
SHUFFLE_SEED, N_DUPLICATES = 5, 64
EYE_START_STAGES = (20, 25, 29)
BATCH_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9)   # nine distinct frames


def _lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        out = os.path.join(tempfile.mkdtemp(prefix="run_window_oracle_"), "librunwindoworacle.so")
        subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", out, os.path.join(HERE, "run_window_oracle.c"), "-lm"],
                       check=True, capture_output=True)
        L = C.CDLL(out)
        L.rw_create.argtypes = [C.POINTER(_OcCascade), C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.rw_create.restype = C.c_void_p
        L.rw_free.argtypes = [C.c_void_p]
        L.rw_free.restype = None
        L.rw_set_scale.argtypes = [C.c_void_p, C.c_double]
        L.rw_set_scale.restype = None
        L.rw_two_rects.argtypes = [C.c_void_p, C.c_int]
        L.rw_two_rects.restype = C.c_int
        L.rw_run_list.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.rw_run_list.restype = None
        _LIB = L
    return _LIB


class WindowOracle:
    """The cascade on one gray frame: run(xy, scale, start_stage) -> (results int32[n], stage sums float64[n])."""

    def __init__(self, c: CascadeArrays, gray: np.ndarray):
        self._g = np.ascontiguousarray(gray)
        self._s, self._keep = Oracle._cstruct(c)
        h, w = self._g.shape
        self.n_stages = c.n_stages
        self._h = _lib().rw_create(C.byref(self._s), self._g.ctypes.data, w, h, self._g.strides[0])

    def run(self, xy, scale: float, start_stage: int = 0):
        p = np.ascontiguousarray(np.asarray(xy, np.int64).reshape(-1, 2).astype(np.int32))
        res = np.zeros(len(p), np.int32)
        sums = np.zeros(len(p), np.float64)
        _lib().rw_set_scale(self._h, float(scale))
        _lib().rw_run_list(self._h, p.ctypes.data, len(p), int(start_stage), res.ctypes.data, sums.ctypes.data)
        assert not (res == INT32_MIN).any(), "the reference asserts here (start_stage)"
        return res, sums

    def two_rects(self, stage: int) -> bool:
        """The stage takes the f64-product branch (tempcv.cpp:872-888)."""
        return bool(_lib().rw_two_rects(self._h, int(stage)))

    def __del__(self):
        try:
            _lib().rw_free(self._h)
        except Exception:
            pass


def run_windows(c: CascadeArrays, frames, windows, scales, start_stage: int = 0):
    """What vj_run_windows_opencv must return for rows of (frame, x, y, scale index): (results, stage sums)."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    res = np.zeros(len(w), np.int32)
    sums = np.zeros(len(w), np.float64)
    for f in np.unique(w[:, 0]):
        o = WindowOracle(c, frames[int(f)])
        for k in np.unique(w[w[:, 0] == f, 3]):
            sel = np.flatnonzero((w[:, 0] == f) & (w[:, 3] == k))
            res[sel], sums[sel] = o.run(w[sel, 1:3], scales[int(k)], start_stage)
    return res, sums


def cv_round(v: float) -> int:
    return int(np.rint(v))          # half to even, as lrint


def chain_factor(k: int, scale_factor: float = 1.1) -> float:
    f = 1.0
    for _ in range(k):
        f *= scale_factor
    return f


def case_scales():
    return [chain_factor(k) for k in CHAIN_STEPS] + list(OFF_CHAIN)


def grid_of(c: CascadeArrays, factor: float, W: int = FRAME_W, H: int = FRAME_H) -> np.ndarray:
    """Every grid position cvHaarDetectObjects' scale-cascade loop gives a factor (tempcv.cpp:1359-1377, :1132-1140): (n, 2) of x, y."""
    ystep = max(2.0, factor)
    win_w, win_h = cv_round(c.win_w * factor), cv_round(c.win_h * factor)
    end_x, end_y = cv_round((W - win_w) / ystep), cv_round((H - win_h) / ystep)
    xs = [cv_round(ix * ystep) for ix in range(max(end_x, 0))]
    ys = [cv_round(iy * ystep) for iy in range(max(end_y, 0))]
    return np.array([(x, y) for y in ys for x in xs], np.int64).reshape(-1, 2)


def full_list(c: CascadeArrays, frame: int = 0) -> np.ndarray:
    """The full grid of the four chain factors and the two factors outside any chain, shuffled with a fixed seed, its first
    N_DUPLICATES windows once more at the end: rows of (frame, x, y, scale index into case_scales())."""
    rows = []
    for k, f in enumerate(case_scales()):
        g = grid_of(c, f)
        rows.append(np.column_stack([np.full(len(g), frame), g, np.full(len(g), k)]))
    w = np.concatenate(rows)
    w = w[np.random.default_rng(SHUFFLE_SEED).permutation(len(w))]
    return np.concatenate([w, w[:N_DUPLICATES]])


def edge_list(c: CascadeArrays, frame: int = 0) -> np.ndarray:
    """Both sides of every edge of the border rule at every scale of case_scales(): x + real_w in {W - 1, W, W + 1, W + 2} (W is
    evaluated, W + 1 is -1), the same for y; x = -1, 0; y = -1, 0."""
    rows = []
    for k, f in enumerate(case_scales()):
        rw, rh = cv_round(c.win_w * f), cv_round(c.win_h * f)
        xs = [-1, 0] + [FRAME_W + d - rw for d in (-1, 0, 1, 2)]
        ys = [-1, 0] + [FRAME_H + d - rh for d in (-1, 0, 1, 2)]
        rows += [(frame, x, y, k) for y in ys for x in xs]
    return np.array(rows, np.int64)


def extreme_list(frame: int = 0) -> np.ndarray:
    """-1, INT32_MAX and INT32_MIN in x, in y and in both, at the first and the last scale of case_scales()."""
    ext = (-1, INT32_MAX, INT32_MIN, INT32_MAX - 19, INT32_MIN + 20)
    rows = []
    for k in (0, len(case_scales()) - 1):
        rows += [(frame, e, 10, k) for e in ext] + [(frame, 10, e, k) for e in ext] + [(frame, e, e2, k) for e in ext for e2 in ext]
    return np.array(rows, np.int64)


def border_mask(c: CascadeArrays, windows, scales) -> np.ndarray:
    """The border rule (tempcv.cpp:817-820) on rows of (frame, x, y, scale index), in Python's unbounded ints."""
    out = []
    for _, x, y, k in np.asarray(windows, np.int64).reshape(-1, 4).tolist():
        rw, rh = cv_round(c.win_w * scales[k]), cv_round(c.win_h * scales[k])
        out.append(x < 0 or y < 0 or x + rw >= FRAME_W + 1 or y + rh >= FRAME_H + 1)
    return np.array(out, bool)


def union_list(c: CascadeArrays) -> np.ndarray:
    return np.concatenate([full_list(c), edge_list(c), extreme_list()])


def union_results(c: CascadeArrays, seed: int):
    """(windows, results, sums) of full_list + edge_list + extreme_list on the cascade's frame."""
    w = union_list(c)
    res, sums = run_windows(c, [faces_frame(seed, FRAME_H, FRAME_W)], w, case_scales())
    return w, res, sums


def linear_premises(c: CascadeArrays, w: np.ndarray, res: np.ndarray) -> bool:
    """At least 6 distinct reject stages, stage 0 and one of the last three among them; at least 10 passes; at least 10 windows
    at -1 by the border rule (off the border -1 is a reject at stage 1)."""
    n = c.n_stages
    border = border_mask(c, w, case_scales())
    assert (res[border] == -1).all()
    stages = {int(-r) for r in res[~border] if r <= 0}
    return (len(stages) >= 6 and 0 in stages and bool(stages & {n - 3, n - 2, n - 1}) and int((res == 1).sum()) >= 10 and
            int(border.sum()) >= 10)


def eye_premises(c: CascadeArrays, w: np.ndarray, res: np.ndarray) -> bool:
    """linear_premises without the passes: what drawn faces can show of eye_tree_eyeglasses."""
    n = c.n_stages
    border = border_mask(c, w, case_scales())
    assert (res[border] == -1).all()
    stages = {int(-r) for r in res[~border] if r <= 0}
    return len(stages) >= 6 and 0 in stages and bool(stages & {n - 3, n - 2, n - 1}) and int(border.sum()) >= 10
