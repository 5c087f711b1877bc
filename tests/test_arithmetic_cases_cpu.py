"""The premises of tests/test_gpu_arithmetic_edges.py, on the CPU: the cascades and frames of tests/cases.py that put stage
sums, variances and window sums where float rounding decides really do so, cell by cell of the tables both files walk.  The
C oracle and its numpy twin agree on them; then, from the twin's per-window leaf values (np_oracle.stage_inputs, and
cv_stage_inputs in the OpenCV profile's f64 arithmetic), every order in which a kernel may add a stage's leaves — reversed,
butterfly in balanced blocks of up to 64, K even ranges — changes the verdict of at least MIN_DECISIVE windows against the
reference's running sum.  The counts are conditions on the inputs (change a seed or a size if one fails, not the bound): a
kernel that trusted such a sum, replayed the wrong bits, or compared with > for >= would differ from the oracle on them."""
import numpy as np
import pytest

from cases import (ARITH_FRAMES, BRIGHT_CASCADES, BRIGHT_MIN, NEAR_FLAT_CELLS, NEAR_FLAT_LEVELS, ORDER_CELLS, ORDER_PREFIX, TIE_CELLS, alternative_orders,
                   arith_frames, bright_frame, cascade_to_product, geometry_cascade, near_flat_frames, order_cascade, sp_delta, tie_cascade)
from oracle import np_oracle

MIN_DECISIVE = 50
F = np.float32


def rows(r):
    return [tuple(int(q[k]) for k in ("scale_idx", "x", "y", "w", "h")) for q in r]


def twin_agrees(oracle, a, img, **kw):
    ro, st = oracle.detect(a, img, **kw)
    dets, entered = np_oracle.detect(a, img, **kw)
    assert rows(ro) == dets and st["stage_entered"] == entered, a.name
    return ro, st


def decisive(oracle, a, frames, stage, cv):
    """(leaves of every window entering `stage`, in-order sums, the threshold the profile compares with, dtype).  The
    windows the twin sees enter every stage up to `stage` are the oracle's, frame by frame."""
    lvs = []
    for f in frames:
        recs = np_oracle.cv_stage_inputs(a, f, stage) if cv else np_oracle.stage_inputs(a, f, stage)
        want = (oracle.detect_opencvlike if cv else oracle.detect)(a, f)[1]["stage_entered"]
        if cv:
            mine = [sum(r["entered"][s] for r in recs) for s in range(stage + 1)]
            assert mine == want[:stage + 1], f"{a.name}: the OpenCV-profile twin enters {mine}, the oracle {want[:stage + 1]}"
        assert sum(len(r["leaves"]) for r in recs) == want[stage], a.name
        lvs += [r["leaves"] for r in recs]
    lv = np.concatenate(lvs)
    dt = np.float64 if cv else F
    thr = np.float64(F(a.stage_threshold[stage]) - F(0.0001)) if cv else F(a.stage_threshold[stage])
    return lv, np_oracle.in_order_sum(lv, dt), thr, dt


@pytest.mark.parametrize("cell", ORDER_CELLS, ids=[c[0] for c in ORDER_CELLS])
def test_order_cells_are_decisive(oracle, cell):
    cid, form, n, cseed, size, fseed = cell
    a = order_cascade(form, n, cseed)
    assert cascade_to_product(a).info.n_stages == a.n_stages          # passes the loader's validation
    frames = arith_frames(size, fseed)
    cv = form == "huge"
    for f in frames:
        twin_agrees(oracle, a, f)
    stages = [ORDER_PREFIX] + ([ORDER_PREFIX + 1] if form == "two_stage" else [])
    for stage in stages:
        lv, base, thr, dt = decisive(oracle, a, frames, stage, cv)
        passed = base >= thr
        assert passed.sum() >= MIN_DECISIVE and (~passed).sum() >= MIN_DECISIVE, (cid, int(passed.sum()), len(lv))
        band = np.float64(sp_delta(a, stage)) * (2.0 ** -28 if cv else 1.0)
        assert np.isfinite(sp_delta(a, stage))
        assert np.all(np.abs(base.astype(np.float64) - np.float64(thr)) <= band), f"{cid}: windows outside the band: the fast path decides them"
        assert len(np.unique(lv.view(np.uint32), axis=0)) > len(lv) // 2 or n < 16, f"{cid}: the verdict bits hardly vary"
        for name, order in alternative_orders(lv.shape[1]).items():
            flips = int(((order(lv, dt) >= thr) != passed).sum())
            assert flips >= MIN_DECISIVE, f"{cid} stage {stage}: order {name} changes {flips} verdicts of {len(lv)}"


def test_tie_cells_are_decisive(oracle):
    (_, _, cseed, size, fseed), _ = TIE_CELLS
    ge, gt = tie_cascade(False, cseed), tie_cascade(True, cseed)
    assert gt.stage_threshold[ORDER_PREFIX] == np.nextafter(ge.stage_threshold[ORDER_PREFIX], F(np.inf))
    frames = arith_frames(size, fseed)
    for a in (ge, gt):
        cascade_to_product(a)
        for f in frames:
            twin_agrees(oracle, a, f)
    for cv in (False, True):
        lv, base, thr, dt = decisive(oracle, ge, frames, ORDER_PREFIX, cv)
        lv2, base2, thr2, _ = decisive(oracle, gt, frames, ORDER_PREFIX, cv)
        assert np.array_equal(lv, lv2)
        for order in alternative_orders(lv.shape[1]).values():      # every order gives the same exact sum
            assert np.array_equal(order(lv, dt), base)
        if cv:     # the profile's bias of 0.0001 is below the lattice (2^-6): the same windows pass both variants
            assert np.array_equal(base >= thr, base2 >= thr2)
            continue
        ties = base == ge.stage_threshold[ORDER_PREFIX]
        assert ties.sum() >= MIN_DECISIVE, int(ties.sum())
        assert np.array_equal((base >= thr) & ~(base2 >= thr2), ties) and not np.any(~(base >= thr) & (base2 >= thr2))
        assert (base >= thr).sum() - ties.sum() >= MIN_DECISIVE and (~(base >= thr)).sum() >= MIN_DECISIVE
        for a, b, t in ((ge, base, thr), (gt, base2, thr2)):
            outside = np.abs(b.astype(np.float64) - np.float64(t)) > np.float64(sp_delta(a, ORDER_PREFIX))
            assert outside.mean() >= 0.9, outside.mean()


def near_flat_cascade(name, cascades):
    if isinstance(name, tuple):
        a = geometry_cascade(name[1][0], name[1][1], name[2])
        return cascade_to_product(a), a
    return cascades(name)


@pytest.mark.parametrize("cell", NEAR_FLAT_CELLS, ids=[c[0] for c in NEAR_FLAT_CELLS])
def test_near_flat_frames_cancel_every_way(oracle, cascades, cell):
    """Over a cell's frames at least 20 evaluated windows have each of: the f32 value of Q / area - mean * mean negative
    (norm factor 1), exactly zero, and in (0, 1).  Levels 255 and 128 each give all three.  Level 1 cannot give a negative
    one — one pixel off leaves a true variance of about 1 / area >= 6e-5, far above the rounding of values near 1 — so there
    zero and positive are asserted.  Where stage 0 is made of stumps, some node comparison of it (rect_sum == thr * var) is an
    exact tie on one of the cell's frames at least; frontalface_alt2 has two-node trees only, in every stage, and the twin
    reports node sums for stumps, so that premise is not stated for its cell."""
    cid, name, size, n_off = cell
    _, a = near_flat_cascade(name, cascades)
    stumps0 = bool(np.all(a.tree_n_nodes[:a.stage_n_trees[0]] == 1))
    ties = 0
    for level, img in zip(NEAR_FLAT_LEVELS, near_flat_frames(size, n_off)):
        twin_agrees(oracle, a, img)
        recs = np_oracle.stage_inputs(a, img, 0, nodes=stumps0)
        raw = np.concatenate([r["var_raw"] for r in recs])
        counts = {"negative": int((raw < 0).sum()), "zero": int((raw == 0).sum()), "small": int(((raw > 0) & (raw < 1)).sum())}
        assert all(v >= 20 for k, v in counts.items() if not (level == 1 and k == "negative")), f"{cid} level {level}: {counts}"
        if stumps0:
            ties += sum(int((r["rect_sum"] == r["thr"]).sum()) for r in recs)
    assert ties >= 1 or not stumps0, f"{cid}: no node comparison is an exact tie"


@pytest.mark.parametrize("name", BRIGHT_CASCADES)
def test_bright_frame_reaches_the_sign_bit(oracle, cascades, name):
    _, a = cascades(name)
    img = bright_frame(1)
    kw = {"min_size": (BRIGHT_MIN, BRIGHT_MIN)}
    plain = twin_agrees(oracle, a, img, **kw)
    signed = twin_agrees(oracle, a, img, signed_mean=True, **kw)
    assert rows(plain[0]) != rows(signed[0]) or plain[1]["stage_entered"] != signed[1]["stage_entered"], \
        "VJ_FLAG_SIGNED_MEAN changes nothing on the bright frame"
    recs = np_oracle.stage_inputs(a, img, 0, **kw)
    assert sum(int((r["pixel_sum"] >= 2 ** 31).sum()) for r in recs) >= 1
    exact = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.uint64)
    exact[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.uint64), 0), 1)
    assert int(exact[-1, -1]) >= 2 ** 32
    straddle = 0
    for r in recs:
        sc = r["scale"]
        y0, x0 = r["y"] + sc["equ_y"], r["x"] + sc["equ_x"]
        wraps = np.stack([exact[y, x] >> np.uint64(32) for y in (y0, y0 + sc["equ_h"]) for x in (x0, x0 + sc["equ_w"])])
        straddle += int((wraps.min(0) != wraps.max(0)).sum())
    assert straddle >= 1, "no window has corners on both sides of a u32 wrap"
