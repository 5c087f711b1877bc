"""vj_run_windows_opencv without a GPU: the restatement of cvSetImagesForHaarClassifierCascade + cvRunHaarClassifierCascadeSum
(tests/run_window_oracle.c) tied to the restatements the project already trusts, the premises of the GPU cases
(tests/test_gpu_run_windows.py), and the argument checks, which run before the environment is needed."""
import os

import numpy as np
import pytest

import roc_oracle as ro
import run_window_oracle as rw
import scale_image_oracle as so
from clfacedetection_amd import Cascade, VjError, cvRunHaarClassifierCascade, run_windows_opencv
from clfacedetection_amd.api import DATA_DIR
from oracle.oracle import Oracle, load_vjc

_ARR = {}


def arrays(casc):
    if casc not in _ARR:
        _ARR[casc] = load_vjc(os.path.join(DATA_DIR, f"haarcascade_{casc}.vjc"))
    return _ARR[casc]


@pytest.mark.parametrize("casc", list(ro.CASES))
def test_raw_rectangles_of_the_detector_pass(casc):
    """(a) every raw rectangle of detect_opencvlike (min_neighbors 0), as the window (x, y) at its factor, gives result 1."""
    a = arrays(casc)
    oracle = Oracle()
    total = 0
    for seed in ro.CASES[casc][:3]:
        f = so.faces_frame(seed, ro.FRAME_H, ro.FRAME_W)
        rects = oracle.detect_opencvlike(a, f)[0]                        # raw: the oracle never groups (min_neighbors 0)
        o = rw.WindowOracle(a, f)
        for k in np.unique(rects["scale_idx"]):
            sel = rects[rects["scale_idx"] == k]
            res, sums = o.run(np.column_stack([sel["x"], sel["y"]]), rw.chain_factor(int(k)))
            assert (res == 1).all(), (casc, seed, int(k))
            assert (sel["w"] == rw.cv_round(a.win_w * rw.chain_factor(int(k)))).all()
        total += len(rects)
    assert total >= 10


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_alt2", "mcs_mouth", "frontalface_alt_tree"])
def test_scale_one_against_level_verdicts_and_roc(casc):
    """(b) at scale 1.0 on every grid position the results are scale_image_oracle.level_verdicts'; where roc_oracle.detect_roc reports
    a window of level 0, level and weight agree bit for bit."""
    full = arrays(casc)
    f = so.faces_frame(ro.CASES[casc][0], ro.FRAME_H, ro.FRAME_W)
    ys, xs = range(0, ro.FRAME_H - full.win_h, 2), range(0, ro.FRAME_W - full.win_w, 2)
    xy = np.array([(x, y) for y in ys for x in xs])
    at = {(int(x), int(y)): i for i, (x, y) in enumerate(xy.tolist())}
    # the cascade itself, and (linear ones) its first four stages: of those detect_roc reports every stage-0 survivor, so that
    # level 0 — the frame at scale 1 — holds reports whatever the content
    for a in (full,) if casc == "frontalface_alt_tree" else (full, ro.first_stages(full, 4)):
        v, _ = so.level_verdicts(a, f, 2)
        res, sums = rw.WindowOracle(a, f).run(xy, 1.0)
        assert np.array_equal(res.reshape(v.shape), v) and (res != -1).any()
        r, lv, lw, _ = ro.detect_roc(a, f)
        n, seen = a.n_stages, 0
        for x, l, wgt in zip(r, lv, lw):
            if x["scale_idx"] != 0:
                continue
            i = at[(int(x["x"]), int(x["y"]))]
            assert (n if res[i] == 1 else -int(res[i])) == int(l)
            assert np.float64(sums[i]).view(np.uint64) == np.float64(wgt).view(np.uint64)
            seen += 1
        assert seen > 100 or a is full


EYE = "eye_tree_eyeglasses"   # see run_window_oracle.SEEDS: drawn faces give it no passes


@pytest.mark.parametrize("casc", rw.LINEAR)
def test_premises_linear(casc):
    """(c) the union of the GPU window lists: at least 6 distinct reject stages with stage 0 and one of the last three, at least 10
    passes (eye_tree_eyeglasses: none, see below), at least 10 border windows; the listed seed is the first from 1 upwards that
    shows them."""
    a = arrays(casc)
    holds = rw.eye_premises if casc == EYE else rw.linear_premises
    for seed in range(1, 40):
        w, res, _ = rw.union_results(a, seed)
        if holds(a, w, res):
            break
    assert seed == rw.SEEDS[casc]


def test_premise_three_node_trees_pass_and_fail_late_with_start_stage():
    """The passes drawn faces do not give eye_tree_eyeglasses from stage 0 come with start_stage: over EYE_START_STAGES the full list
    shows at least 10 passes and rejects at each of the last three stages, and every verdict is of a stage from the start on."""
    a = arrays(EYE)
    n = a.n_stages
    f = so.faces_frame(rw.SEEDS[EYE], rw.FRAME_H, rw.FRAME_W)
    w = rw.full_list(a)
    passes, stages = 0, set()
    for start in rw.EYE_START_STAGES:
        res, sums = rw.run_windows(a, [f], w, rw.case_scales(), start)
        assert ((res == 1) | (res <= -start)).all() and (sums != 0.0).all()
        passes += int((res == 1).sum())
        stages |= {int(-r) for r in res if r <= 0}
    assert passes >= 10 and {n - 3, n - 2, n - 1} <= stages and n == 30


def test_premise_both_stump_modes_decide_rejects():
    a = arrays("frontalface_alt")
    w, res, _ = rw.union_results(a, rw.SEEDS["frontalface_alt"])
    o = rw.WindowOracle(a, so.faces_frame(rw.SEEDS["frontalface_alt"], rw.FRAME_H, rw.FRAME_W))
    border = rw.border_mask(a, w, rw.case_scales())
    modes = {o.two_rects(int(-r)) for r in res[~border] if r <= 0}
    assert modes == {True, False}


def test_premise_stage_tree():
    a = arrays("frontalface_alt_tree")
    for seed in range(1, 40):
        w, res, _ = rw.union_results(a, seed)
        if (res == 0).sum() >= 10 and (res == 1).sum() >= 10:
            break
    assert seed == rw.SEEDS["frontalface_alt_tree"]
    border = rw.border_mask(a, w, rw.case_scales())
    assert set(res[~border].tolist()) == {0, 1}


def test_start_stage_of_the_restatement():
    a = arrays("frontalface_alt")
    o = rw.WindowOracle(a, so.faces_frame(1, rw.FRAME_H, rw.FRAME_W))
    xy = rw.grid_of(a, 1.0)
    base, bsum = o.run(xy, 1.0)
    for start in (1, 11, 21):
        res, sums = o.run(xy, 1.0, start)
        assert ((res == 1) | (res <= -start)).all()
        late = base <= -start
        assert np.array_equal(res[late], base[late]) and np.array_equal(sums[late].view(np.uint64), bsum[late].view(np.uint64))
    res, sums = o.run(xy, 1.0, 22)
    assert (res == 1).all() and (sums == 0.0).all()


def test_measurement_script_builds_the_chain_grid():
    """tests/measure_run_windows.py is run by hand on a GPU; what it does without one is kept alive here: it imports (no device is
    touched before main()), and its list is the detector's enumeration — the factors of the chain up to the frame, every position of
    grid_of per factor, rows of (0, x, y, slot) as int32."""
    import measure_run_windows as m
    a = arrays("frontalface_alt")
    scales, w = m.chain_grid(rw.FRAME_W, rw.FRAME_H, a.win_w, a.win_h)
    want = [rw.chain_factor(k) for k in range(len(scales))]
    assert scales == want and want[-1] * a.win_h < rw.FRAME_H - 10 <= want[-1] * 1.1 * a.win_h
    assert w.dtype == np.int32 and w.flags.c_contiguous and (w[:, 0] == 0).all() and (np.diff(w[:, 3]) >= 0).all()
    for k, s in enumerate(scales):
        assert np.array_equal(w[w[:, 3] == k][:, 1:3], rw.grid_of(a, s)), k
    assert not rw.border_mask(a, w, scales).any()                          # every one of them is evaluated
    big_scales, big = m.chain_grid(m.W, m.H, m.WIN, m.WIN)
    assert len(big_scales) == 42 and len(big) < 2**27                      # 20 * 1.1^41 < 1070 <= 20 * 1.1^42; within a call's cap


def test_wrappers_refuse_bad_arguments_without_a_device():
    """(d) the host checks run before the environment is looked at: with no environment at all, a bad list is refused for what is
    wrong with it, and a good one for the missing environment."""
    c = Cascade.load("frontalface_alt")
    tree = Cascade.load("frontalface_alt_tree")
    f = so.faces_frame(1, rw.FRAME_H, rw.FRAME_W)

    def refused(cascade, windows, scales, start=0, frames=None):
        with pytest.raises(VjError) as ei:
            run_windows_opencv([f] if frames is None else frames, cascade, None, windows, scales, start)
        assert ei.value.code == 1                                           # VJ_ERR_ARG
        return str(ei.value)

    assert "frame 1 of 1" in refused(c, [(1, 0, 0, 0)], [1.0])
    assert "frame -1" in refused(c, [(0, 0, 0, 0), (-1, 0, 0, 0)], [1.0])
    assert "scale 2 of 2" in refused(c, [(0, 0, 0, 2)], [1.0, 1.1])
    assert "scale -1" in refused(c, [(0, 0, 0, -1)], [1.0])
    assert "negative" in refused(c, [(0, 0, 0, 0)], [1.0], -1)
    assert "stage tree" in refused(tree, [(0, 0, 0, 0)], [1.0], 1)
    assert "finite" in refused(c, [(0, 0, 0, 0)], [0.0])
    assert "finite" in refused(c, [(0, 0, 0, 0)], [float("nan")])
    assert "one size" in refused(c, [(0, 0, 0, 0)], [1.0], frames=[f, f[:90]])
    assert "no environment" in refused(c, [(0, 0, 0, 0)], [1.0])
    res, sums = run_windows_opencv([f], c, None, np.zeros((0, 4), np.int64), [1.0])   # n_windows == 0 is VJ_OK, environment or not
    assert len(res) == 0 and len(sums) == 0
    with pytest.raises(ValueError):
        run_windows_opencv([f], c, None, [(0, 0, 0)], [1.0])                # not rows of four
    with pytest.raises(ValueError):
        run_windows_opencv([f], c, None, [(0, 2**31, 0, 0)], [1.0])         # not an int32
    with pytest.raises(ValueError):
        run_windows_opencv([f], c, None, [(0.5, 0, 0, 0)], [1.0])
    with pytest.raises(VjError):
        cvRunHaarClassifierCascade(f, c, None, (0, 0), 1.0, -1)
