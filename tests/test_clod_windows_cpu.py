"""CPU side of vj_run_windows: the numpy restatement of the per-window path (tests/clod_window_oracle.py) tied to
the committed oracle — the C one's detections and per-stage counts, the numpy twin's variances and leaf values — on one frame per
cascade kind over the full grid of every accepted scale; the premises of the lists the GPU file runs; and the binding."""
import os
import re

import numpy as np
import pytest

import clod_window_oracle as cw
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("frontalface_alt", "frontalface_alt2", "frontalface_alt_tree")   # stumps, two-node trees, a stage tree
_CASE = {}


def bits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def grid_case(oracle, cascades, casc):
    """The restatement on every grid window of every accepted scale of the cascade's frame: per scale (OcScale, xy, res, sums, var)."""
    if casc not in _CASE:
        _, a = cascades(casc)
        f = cw.faces_frame(cw.SEEDS[casc], cw.FRAME_H, cw.FRAME_W)
        o = cw.ClodWindowOracle(a, f)
        per_scale = []
        for sc in oracle.plan_scales(a, cw.FRAME_W, cw.FRAME_H):
            if not sc.accepted or sc.nx <= 0 or sc.ny <= 0:
                continue
            xy = cw.grid_of(a, sc.scale)
            assert len(xy) == sc.nx * sc.ny
            per_scale.append((sc, xy) + o.run(xy, sc.scale))
        _CASE[casc] = (a, f, per_scale)
    return _CASE[casc]


@pytest.mark.parametrize("casc", KINDS)
def test_geometry_is_setup_scale(oracle, cascades, casc):
    a, _, per_scale = grid_case(oracle, cascades, casc)
    assert len(per_scale) >= 10
    for sc, *_ in per_scale:
        g = cw.geometry(a, sc.scale)
        assert (g["sw"], g["sh"], g["ex"], g["ew"], g["eh"], g["area"]) == (sc.win_w, sc.win_h, sc.equ_x, sc.equ_w, sc.equ_h, sc.area)
    g = cw.geometry(a, 2.5)                                                # ties round away from zero: 2.5 -> 3, 45, 50
    assert (g["ex"], g["ew"], g["sw"]) == (3, 45, 50)
    assert cw.geometry(a, 1e30)["sw"] == cw.WIN_MAX


@pytest.mark.parametrize("casc", KINDS)
def test_passes_and_stage_counts_are_the_oracles(oracle, cascades, casc):
    a, f, per_scale = grid_case(oracle, cascades, casc)
    rects, stats = oracle.detect(a, f)
    mine = sorted((sc.scale_idx, int(x), int(y), sc.win_w, sc.win_h) for sc, xy, res, _, _ in per_scale for x, y in xy[res == 1])
    want = sorted((int(r["scale_idx"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in rects)
    assert mine == want and len(want) >= 1
    res = np.concatenate([r for _, _, r, _, _ in per_scale])
    assert not (res == cw.OUTSIDE).any()                                   # every grid window lies inside
    assert stats["stage_entered"][0] == len(res) == stats["windows"]
    if casc != "frontalface_alt_tree":
        for s in range(1, a.n_stages):
            assert int(((res == 1) | (res <= -s)).sum()) == stats["stage_entered"][s], s
    else:
        assert set(res.tolist()) == {0, 1}


@pytest.mark.parametrize("casc", KINDS)
def test_variance_and_stage_sums_are_the_twins(oracle, cascades, casc):
    a, f, per_scale = grid_case(oracle, cascades, casc)
    linear = casc != "frontalface_alt_tree"
    by_idx = {sc.scale_idx: (xy, res, sums, var) for sc, xy, res, sums, var in per_scale}
    compared = {}
    for stage in (0, 1, a.n_stages - 1) if linear else (0,):
        compared[stage] = 0
        for rec in np_oracle.stage_inputs(a, f, stage):
            xy, res, sums, var = by_idx[rec["scale"]["scale_idx"]]
            row = {(int(x), int(y)): i for i, (x, y) in enumerate(xy)}
            at = np.array([row[(int(x), int(y))] for x, y in zip(rec["x"], rec["y"])], np.int64)
            if stage == 0:
                assert len(at) == len(xy) and np.array_equal(at, np.arange(len(xy)))
                assert np.array_equal(bits(var), bits(rec["var"]))
            assert np.array_equal(bits(var[at]), bits(rec["var"]))
            want = np_oracle.in_order_sum(rec["leaves"])
            if linear:
                here = (res[at] == -stage) | ((res[at] == 1) & (stage == a.n_stages - 1))
            else:   # a reject at the root of the tree ends the walk (on_fail == -2): its sum is the stage's
                assert cw.stage_links(a)[1][0] == -2
                here = want < a.stage_threshold[0]
                assert (res[at][here] == 0).all()
            assert np.array_equal(bits(sums[at][here]), bits(want[here]))
            compared[stage] += int(here.sum())
    assert all(n > 0 for n in compared.values()), compared


@pytest.mark.parametrize("casc", list(cw.SEEDS))
def test_premises_of_the_gpu_lists(cascades, casc):
    """Rejects at six or more distinct stages and at least one pass in every full list; windows on both sides of every edge.
    eye_tree_eyeglasses: drawn faces hold no eye it accepts (no seed of 1 .. 29 gives a pass), so its frame is the first with
    a reject in one of its last three stages, and its passes come with start_stage (EYE_START_STAGES)."""
    _, a = cascades(casc)
    f = cw.faces_frame(cw.SEEDS[casc], cw.FRAME_H, cw.FRAME_W)
    scales = cw.case_scales()
    res, sums, var = cw.run_windows(a, [f], cw.full_list(a), scales)
    if casc == "eye_tree_eyeglasses":
        stages = {int(-r) for r in res if r <= 0}
        assert len(stages) >= 6 and 0 in stages and stages & {a.n_stages - 3, a.n_stages - 2, a.n_stages - 1}
        for start in cw.EYE_START_STAGES:
            r2, _, _ = cw.run_windows(a, [f], cw.full_list(a), scales, start_stage=start)
            assert (r2 == 1).any() and (r2 <= -start).any() and ((r2 == 1) | (r2 <= -start)).all()
    else:
        assert cw.list_premises(a, res)
    assert not (res == cw.OUTSIDE).any() and (var > 0).any()
    w = cw.edge_list(a)
    res, sums, var = cw.run_windows(a, [f], w, scales)
    out = cw.outside_mask(a, w, scales)
    assert (res[out] == cw.OUTSIDE).all() and (sums[out] == 0).all() and (var[out] == 0).all() and (res[~out] != cw.OUTSIDE).all()
    for k in range(len(scales)):
        g = cw.geometry(a, scales[k])
        for x, y, inside in ((cw.FRAME_W - g["sw"], 0, True), (cw.FRAME_W - g["sw"] + 1, 0, False), (0, cw.FRAME_H - g["sh"], True),
                             (0, cw.FRAME_H - g["sh"] + 1, False), (-1, 0, False), (0, -1, False), (0, 0, True)):
            i = np.flatnonzero((w[:, 1] == x) & (w[:, 2] == y) & (w[:, 3] == k))
            assert len(i) >= 1 and bool(out[i[0]]) == (not inside), (k, x, y)
    res, _, _ = cw.run_windows(a, [f], cw.extreme_list(), scales)
    assert (res == cw.OUTSIDE).all()


def test_header_and_binding_declare_the_call():
    from clfacedetection_amd.api import _SIGNATURES, CLOD_WINDOW_RESULT_DTYPE, VJ_WINDOW_OUTSIDE
    assert "vj_run_windows" in _SIGNATURES and len(_SIGNATURES["vj_run_windows"][1]) == 11
    header = open(os.path.join(ROOT, "include", "vj.h")).read()
    assert re.search(r"\bint\s+vj_run_windows\s*\(", header) and re.search(r"#define\s+VJ_WINDOW_OUTSIDE\s+INT32_MIN", header)
    assert re.search(r"typedef struct vj_clod_window_result \{ int32_t result; float variance; float stage_sum; int32_t reserved; \}", header)
    assert CLOD_WINDOW_RESULT_DTYPE.itemsize == 16 and CLOD_WINDOW_RESULT_DTYPE.names == ("result", "variance", "stage_sum", "reserved")
    assert VJ_WINDOW_OUTSIDE == -2**31 == cw.OUTSIDE
    import clfacedetection_amd as pkg
    assert callable(pkg.run_windows) and callable(pkg.runCascade) and callable(pkg.Environment.run_windows)
