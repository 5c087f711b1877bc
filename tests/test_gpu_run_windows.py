"""vj_run_windows_opencv on the device against the test restatement (tests/run_window_oracle.c): `result` exactly, `stage_sum` as
u64 bit patterns.  Frames of 180 x 240; the window lists and their premises (reject stages, passes, border windows, both stump
modes) are built in tests/run_window_oracle.py and asserted on the CPU in tests/test_run_windows_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import heavy_cases as hc
import roc_oracle as ro
import run_window_oracle as rw
import scale_image_oracle as so
from cases import cascade_to_product, tunables
from clfacedetection_amd import DeviceFrames, VjError, cvRunHaarClassifierCascade, run_windows_opencv
from clfacedetection_amd.api import WINDOW_DTYPE, WINDOW_RESULT_DTYPE

pytestmark = pytest.mark.gpu
VJ_ERR_ARG = 1
H, W = rw.FRAME_H, rw.FRAME_W
_FRAMES = {}


def frame(seed):
    if seed not in _FRAMES:
        _FRAMES[seed] = so.faces_frame(seed, H, W)
    return _FRAMES[seed]


def check(env, c, a, frames, windows, scales, start_stage=0, color=False, gray=None):
    """One call against the restatement; returns (results, sums)."""
    res, sums = run_windows_opencv(frames, c, env, windows, scales, start_stage, color=color)
    assert res.dtype == np.int32 and sums.dtype == np.float64 and len(res) == len(sums) == len(windows)
    want_res, want_sums = rw.run_windows(a, frames if gray is None else gray, windows, scales, start_stage)
    bad = np.flatnonzero((res != want_res) | (sums.view(np.uint64) != want_sums.view(np.uint64)))
    assert len(bad) == 0, (len(bad), [(np.asarray(windows)[i].tolist(), int(res[i]), int(want_res[i]), float(sums[i]), float(want_sums[i]))
                                     for i in bad[:5]])
    return res, sums


@pytest.mark.parametrize("casc", list(rw.SEEDS))
def test_full_shuffled_list(env, cascades, casc):
    """The full grid of four chain factors, 2.5 (cvRound ties) and 1.37, shuffled, with duplicates: stumps in both stage modes,
    two- and three-node trees, tilted features, the stage tree."""
    c, a = cascades(casc)
    w = rw.full_list(a)
    res, sums = check(env, c, a, [frame(rw.SEEDS[casc])], w, rw.case_scales())
    n = rw.N_DUPLICATES
    assert np.array_equal(res[-n:], res[:n]) and np.array_equal(sums[-n:].view(np.uint64), sums[:n].view(np.uint64))
    assert (res <= 0).any() and ((res == 1).any() or casc == "eye_tree_eyeglasses")   # (its passes: test_start_stage_three_node_trees)
    if casc == "eye_tree_eyeglasses":
        assert (res <= -(a.n_stages - 3)).any()                            # a reject in one of the last three stages


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_list_lengths_of_one_scale(env, cascades, n):
    c, a = cascades("frontalface_alt")
    g = rw.grid_of(a, rw.case_scales()[1])[100:100 + n]
    w = np.column_stack([np.zeros(n, np.int64), g, np.zeros(n, np.int64)])
    check(env, c, a, [frame(1)], w, [rw.case_scales()[1]])


def test_two_scales_alternating(env, cascades):
    c, a = cascades("frontalface_alt")
    s = [rw.case_scales()[0], rw.OFF_CHAIN[0]]
    g0, g1 = rw.grid_of(a, s[0]), rw.grid_of(a, s[1])
    n = min(len(g0), len(g1), 500)
    w = np.zeros((2 * n, 4), np.int64)
    w[0::2, 1:3], w[1::2, 1:3], w[1::2, 3] = g0[:n], g1[:n], 1
    check(env, c, a, [frame(1)], w, s)


@pytest.mark.parametrize("casc", ["frontalface_alt", "mcs_mouth", "frontalface_alt_tree"])
def test_border_rule_edges(env, cascades, casc):
    """x + real_w == W is evaluated, x + real_w == W + 1 is -1; the same for y; x = -1 and y = -1 are -1."""
    c, a = cascades(casc)
    scales = rw.case_scales()
    w = rw.edge_list(a)
    res, sums = check(env, c, a, [frame(rw.SEEDS[casc])], w, scales)
    border = rw.border_mask(a, w, scales)
    assert (res[border] == -1).all() and (sums[border] == 0.0).all() and border.sum() >= 10
    for i, (_, x, y, k) in enumerate(w.tolist()):
        rw_, rh_ = rw.cv_round(a.win_w * scales[k]), rw.cv_round(a.win_h * scales[k])
        if x >= 0 and y >= 0 and x + rw_ <= W and y + rh_ <= H:
            assert not border[i]                                           # W itself is evaluated
        if x + rw_ == W + 1 or y + rh_ == H + 1 or x == -1 or y == -1:
            assert res[i] == -1
    linear = casc != "frontalface_alt_tree"
    assert (sums[~border & ((res != -1) if linear else True)] != 0.0).all()   # an evaluated window leaves a stage sum


def test_extreme_coordinates(env, cascades):
    """-1, INT32_MAX, INT32_MIN: -1 and no wild address."""
    c, a = cascades("frontalface_alt")
    w = rw.extreme_list()
    res, sums = check(env, c, a, [frame(1)], w, rw.case_scales())
    assert (res == -1).all() and (sums == 0.0).all()
    assert {rw.INT32_MAX, rw.INT32_MIN, -1} <= set(w[:, 1].tolist()) and {rw.INT32_MAX, rw.INT32_MIN, -1} <= set(w[:, 2].tolist())


def test_scale_whose_window_exceeds_the_frame(env, cascades):
    c, a = cascades("frontalface_alt")
    scales = [1.0, 9.5, 1e300, 12.0]                                       # 20 * 9.5 = 190 > 180: too high; 12.0: too wide as well
    g = rw.grid_of(a, 1.0)[::7]
    w = np.concatenate([np.column_stack([np.zeros(len(g), np.int64), g, np.full(len(g), k)]) for k in range(4)])
    res, _ = check(env, c, a, [frame(1)], w, scales)
    assert (res[w[:, 3] != 0] == -1).all() and (res[w[:, 3] == 0] != -1).any()


@pytest.mark.parametrize("start", [1, 11, 21, 22])
def test_start_stage(env, cascades, start):
    c, a = cascades("frontalface_alt")
    assert a.n_stages == 22
    scales = rw.case_scales()
    w = np.concatenate([rw.full_list(a)[:6000], rw.edge_list(a)])
    res, sums = check(env, c, a, [frame(1)], w, scales, start_stage=start)
    border = rw.border_mask(a, w, scales)
    assert (res[~border] <= -start).any() or start >= 21 or (res[~border] == 1).all()
    assert ((res[~border] == 1) | (res[~border] <= -start)).all()          # no verdict of a stage before start_stage
    if start == 22:
        assert (res[~border] == 1).all() and (sums == 0.0).all()
    base, _ = run_windows_opencv([frame(1)], c, env, w, scales)
    if start < 22:
        assert (res[base == 1] == 1).all()                                 # a window that passes every stage passes the later ones


@pytest.mark.parametrize("start", rw.EYE_START_STAGES)
def test_start_stage_three_node_trees(env, cascades, start):
    """eye_tree_eyeglasses from a late stage on: the passes and the late rejects of the multi-node-tree path, which drawn faces do
    not give it from stage 0 (the premise is asserted in tests/test_run_windows_cpu.py)."""
    c, a = cascades("eye_tree_eyeglasses")
    res, _ = check(env, c, a, [frame(rw.SEEDS["eye_tree_eyeglasses"])], rw.full_list(a), rw.case_scales(), start_stage=start)
    assert (res == 1).any() and (res <= -start).any() and ((res == 1) | (res <= -start)).all()


def test_start_stage_refusals(env, cascades):
    c, _ = cascades("frontalface_alt")
    t, _ = cascades("frontalface_alt_tree")
    w = [(0, 10, 10, 0)]
    for casc, start in ((c, -1), (c, -2**31), (t, 1), (t, 46)):
        with pytest.raises(VjError) as ei:
            run_windows_opencv([frame(1)], casc, env, w, [1.0], start)
        assert ei.value.code == VJ_ERR_ARG
    run_windows_opencv([frame(1)], t, env, w, [1.0], 0)


@pytest.mark.parametrize("form", ro.WIDE_FORMS)
def test_heavy_survivors(env, form):
    """The all-pass-prefix survivor cascade on heavy_cases' dots: every lane of a unit reaches the last stage (the premise is
    asserted here on the restatement's verdicts: no reject before stage 3)."""
    a = ro.wide_cascade(form)
    c = cascade_to_product(a)
    f = hc.frame_of(("dots", 7000, H, W, (H * W) // 4000))
    scales = [1.0, rw.case_scales()[1]]
    w = np.concatenate([np.column_stack([np.zeros(len(g), np.int64), g, np.full(len(g), k)])
                        for k, g in enumerate(rw.grid_of(a, s) for s in scales)])
    res, _ = check(env, c, a, [f], w, scales)
    assert a.n_stages == 4 and set(res.tolist()) <= {1, -3} and (res == 1).any() and (res == -3).any()


def _batch_case(a):
    frames = [frame(s) for s in rw.BATCH_SEEDS]
    scales = rw.case_scales()
    rng = np.random.default_rng(11)
    rows = []
    for k, s in enumerate(scales):
        g = rw.grid_of(a, s)
        g = g[rng.permutation(len(g))[:400]]
        rows.append(np.column_stack([rng.integers(0, len(frames), len(g)), g, np.full(len(g), k)]))
    w = np.concatenate(rows)
    w = w[rng.permutation(len(w))]                                         # out of frame order
    assert set(w[:, 0].tolist()) == set(range(9)) and (np.diff(w[:, 0]) < 0).any()
    return frames, scales, w


@pytest.mark.parametrize("casc", ["frontalface_alt", "mcs_mouth"])
def test_batch_of_nine_frames_and_subbatch_split(env, cascades, casc):
    c, a = cascades(casc)
    frames, scales, w = _batch_case(a)
    base = check(env, c, a, frames, w, scales)
    with tunables(env, ("max_subbatch", "2")):                             # five sub-batches
        split = check(env, c, a, frames, w, scales)
    assert np.array_equal(split[0], base[0]) and np.array_equal(split[1].view(np.uint64), base[1].view(np.uint64))
    assert env.query("max_subbatch") == "0"
    # windows of three of the nine frames only: the sub-batches no window looks at are skipped
    some = w[np.isin(w[:, 0], (1, 4, 8))]
    with tunables(env, ("max_subbatch", "2")):
        check(env, c, a, frames, some, scales)


def test_bgr_and_device_frames(env, oracle, cascades):
    c, a = cascades("frontalface_alt")
    frames, scales, w = _batch_case(a)
    frames = frames[:3]
    w = w[w[:, 0] < 3]
    bgr = np.repeat(np.stack(frames)[..., None], 3, axis=3)
    bgr[..., 1] = np.stack(frames)[:, ::-1]
    gray = [oracle.bgr2gray(b) for b in bgr]
    base = check(env, c, a, list(bgr), w, scales, color=True, gray=gray)
    bgra = np.concatenate([bgr, np.full(bgr.shape[:3] + (1,), 255, np.uint8)], axis=3)
    check(env, c, a, list(bgra), w, scales, color=True, gray=gray)
    import torch
    t = torch.from_numpy(bgr.copy()).cuda()
    dev = check(env, c, a, DeviceFrames.from_torch(t), w, scales, gray=gray)
    assert np.array_equal(dev[0], base[0]) and np.array_equal(dev[1].view(np.uint64), base[1].view(np.uint64))
    tg = torch.from_numpy(np.stack(frames)).cuda()
    check(env, c, a, DeviceFrames.from_torch(tg), w, scales, gray=frames)


def test_errors_leave_out_untouched(env, lib, cascades):
    c, a = cascades("frontalface_alt")
    imgs, n, keep = env._images([frame(1), frame(2)], False)
    scales = np.array([1.0, 1.5])
    good = np.array([(0, 4, 4, 0), (1, 8, 8, 1), (0, 2, 2, 1)], WINDOW_DTYPE)

    def call(wins, n_w=None, start=0):
        out = np.zeros(len(wins), WINDOW_RESULT_DTYPE)
        out["result"], out["reserved"], out["stage_sum"] = 77, 78, 79.0     # sentinel fill
        rc = lib.vj_run_windows_opencv(env._h, c._h, imgs, n, scales.ctypes.data, len(scales), wins.ctypes.data,
                                       len(wins) if n_w is None else n_w, start, out.ctypes.data)
        return rc, out

    def untouched(out):
        return (out["result"] == 77).all() and (out["reserved"] == 78).all() and (out["stage_sum"] == 79.0).all()

    rc, out = call(good)
    assert rc == 0 and (out["result"] != 77).all() and (out["reserved"] == 0).all()
    rc, out = call(good, n_w=0)
    assert rc == 0 and untouched(out)                                       # n_windows == 0
    assert lib.vj_run_windows_opencv(env._h, c._h, None, 0, None, 0, None, 0, 0, None) == 0
    for field, value in (("frame", 2), ("frame", -1), ("scale", 2), ("scale", -1), ("frame", 2**31 - 1)):
        for at in (0, 2):
            bad = good.copy()
            bad[field][at] = value
            rc, out = call(bad)
            assert rc == VJ_ERR_ARG and untouched(out), (field, value, at)
    res, sums = run_windows_opencv([frame(1)], c, env, np.zeros((0, 4), np.int64), [1.0])
    assert len(res) == 0 and len(sums) == 0
    for bad_scale in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(VjError) as ei:
            run_windows_opencv([frame(1)], c, env, [(0, 1, 1, 0)], [bad_scale])
        assert ei.value.code == VJ_ERR_ARG
    with pytest.raises(VjError):
        run_windows_opencv([frame(1), frame(1)[:100]], c, env, [(0, 1, 1, 0)], [1.0])   # frames of two sizes


def test_timing_of_the_last_call(env, lib, cascades):
    """vj_run_windows_timing: the device times of the last call, both positive after a call that ran the kernel, summed over the
    sub-batches of a split one, and refused for no environment."""
    c, a = cascades("frontalface_alt")
    frames, scales, w = _batch_case(a)
    run_windows_opencv(frames, c, env, w, scales)
    integral_ms, pass_ms = env.run_windows_timing()
    assert 0.0 < integral_ms < 1e3 and 0.0 < pass_ms < 1e3                  # (a kernel takes microseconds at the least; 1 s: no garbage)
    assert env.run_windows_timing() == (integral_ms, pass_ms)              # reading changes nothing
    run_windows_opencv(frames[:1], c, env, [(0, -1, 0, 0)], scales)         # a new call replaces them
    again = env.run_windows_timing()
    assert again[0] > 0.0 and again[1] > 0.0
    i_ms, p_ms = C.c_float(-1.0), C.c_float(-1.0)
    assert lib.vj_run_windows_timing(env._h, None, C.byref(p_ms)) == 0 and p_ms.value == again[1]
    assert lib.vj_run_windows_timing(None, C.byref(i_ms), C.byref(p_ms)) == VJ_ERR_ARG and i_ms.value == -1.0


@pytest.mark.parametrize("casc", ["frontalface_alt", "frontalface_alt2", "mcs_mouth", "frontalface_alt_tree"])
def test_raw_detections_pass_here(env, cascades, casc):
    """Every raw rectangle of vj_detect_opencv, as a window at its factor, gets result 1."""
    c, a = cascades(casc)
    frames = [frame(s) for s in ro.CASES[casc][:3]]
    r = env.detect_opencv(c, frames, min_neighbors=0)
    assert len(r.rects) >= 10
    n_scales = int(r.rects["scale_idx"].max()) + 1
    scales = [rw.chain_factor(k) for k in range(n_scales)]
    w = np.column_stack([r.rects["frame"], r.rects["x"], r.rects["y"], r.rects["scale_idx"]]).astype(np.int64)
    res, _ = check(env, c, a, frames, w, scales)
    assert (res == 1).all()


def test_one_window_wrapper_equals_the_batch_entry(env, cascades):
    c, a = cascades("frontalface_alt")
    scale = rw.OFF_CHAIN[1]
    g = rw.grid_of(a, scale)
    w = np.column_stack([np.zeros(len(g), np.int64), g, np.zeros(len(g), np.int64)])
    res, _ = check(env, c, a, [frame(1)], w, [scale])
    picks = [int(np.flatnonzero(res == v)[0]) for v in sorted(set(res.tolist()))][:8] + [0, len(g) - 1]
    for i in picks:
        assert cvRunHaarClassifierCascade(frame(1), c, env, (int(g[i, 0]), int(g[i, 1])), scale) == int(res[i])
    assert cvRunHaarClassifierCascade(frame(1), c, env, (-1, 0)) == -1
    assert cvRunHaarClassifierCascade(frame(1), c, env, (W - 20, H - 20)) != -1 or a.n_stages < 2   # x + 20 == W: evaluated
    s5, _ = run_windows_opencv([frame(1)], c, env, w, [scale], 5)
    i = int(np.flatnonzero(s5 <= 0)[0])
    assert cvRunHaarClassifierCascade(frame(1), c, env, (int(g[i, 0]), int(g[i, 1])), scale, 5) == int(s5[i])


def test_more_scales_than_the_plan_cache_holds(env, cascades):
    """64 scales in one call, more than plan_cache_max = 48: every table stays alive while the call runs."""
    c, a = cascades("frontalface_alt")
    scales = [1.0 + 0.03 * k for k in range(64)]
    rng = np.random.default_rng(3)
    rows = []
    for k, s in enumerate(scales):
        g = rw.grid_of(a, s)
        rows.append(np.column_stack([np.zeros(40, np.int64), g[rng.permutation(len(g))[:40]], np.full(40, k)]))
    w = np.concatenate(rows)
    w = w[rng.permutation(len(w))]
    check(env, c, a, [frame(1)], w, scales)
    check(env, c, a, [frame(1)], w[::-1], scales)
