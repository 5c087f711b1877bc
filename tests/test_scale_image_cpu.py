"""CV_HAAR_SCALE_IMAGE on the CPU: the test restatement (tests/scale_image_oracle.c) against hand-computed values and against the
oracle's own OpenCV-profile walk, and the premises of the GPU tests (tests/test_gpu_scale_image.py)."""
import numpy as np
import pytest

import scale_image_oracle as so
from clfacedetection_amd import synth


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (37, 53), (120, 161)])
def test_resize_identity_at_equal_size(h, w):
    g = synth.frame("noise", h + w, h, w)
    assert np.array_equal(so.resize_linear(g, w, h), g)


def test_resize_two_to_one_is_the_area_formula():
    g = synth.frame("noise", 2, 40, 60).astype(np.int32)
    want = (g[0::2, 0::2] + g[0::2, 1::2] + g[1::2, 0::2] + g[1::2, 1::2] + 2) >> 2
    assert np.array_equal(so.resize_linear(g.astype(np.uint8), 30, 20), want.astype(np.uint8))
    # 2:1 in one direction only is NOT the area path: bilinear taps at 0.5 / 0.5 horizontally, rows as they are
    got = so.resize_linear(g.astype(np.uint8), 30, 40)
    h = g[:, 0::2] * 1024 + g[:, 1::2] * 1024
    assert np.array_equal(got, ((((2048 * (h >> 4)) >> 16) + 2) >> 2).astype(np.uint8))


def test_resize_three_by_three_to_two_by_two_by_hand():
    """scale = 1.5: fx(0) = 0.25 -> taps (0, 1) weights (1536, 512); fx(1) = 1.75 -> taps (1, 2) weights (512, 1536); rows alike.
    dst(0, 0): h0 = 10 * 1536 + 20 * 512 = 25600, h1 = 40 * 1536 + 50 * 512 = 87040;
    ((1536 * 1600) >> 16) + ((512 * 5440) >> 16) + 2 = 37 + 42 + 2 = 81; 81 >> 2 = 20."""
    s = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    got = so.resize_linear(s, 2, 2)
    taps = [(0, 1, 1536, 512), (1, 2, 512, 1536)]
    want = np.zeros((2, 2), np.uint8)
    for y, (y0, y1, b0, b1) in enumerate(taps):
        for x, (x0, x1, a0, a1) in enumerate(taps):
            h0 = int(s[y0, x0]) * a0 + int(s[y0, x1]) * a1
            h1 = int(s[y1, x0]) * a0 + int(s[y1, x1]) * a1
            want[y, x] = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
    assert got[0, 0] == 20
    assert np.array_equal(got, want)
    assert want.tolist() == [[20, 35], [65, 80]]      # = the exact bilinear values 20, 35, 65, 80


def test_resize_clamps_last_row_and_column():
    """4 x 4 -> 7 x 7: column 6 has fx = 3.214 -> sx = 3 = sw - 1: the last source column alone; row 6 reads rows 3 and 4 -> 3 with
    its fraction kept (1609 / 439), row 0 reads rows -1 -> 0 and 0 (439 / 1609)."""
    s = synth.frame("noise", 9, 4, 4).copy()
    s[3, 3], s[0, 3] = 200, 100
    got = so.resize_linear(s, 7, 7)
    assert got[6, 6] == (((1609 * 25600) >> 16) + ((439 * 25600) >> 16) + 2) >> 2 == 200
    assert got[0, 6] == (((439 * 12800) >> 16) + ((1609 * 12800) >> 16) + 2) >> 2 == 100
    t = s.copy()
    t[:, :3] = 255 - t[:, :3]       # the last output column depends on the last source column only
    assert np.array_equal(so.resize_linear(t, 7, 7)[:, 6], got[:, 6])
    assert not np.array_equal(so.resize_linear(t, 7, 7)[:, 5], got[:, 5])


@pytest.mark.parametrize("casc,h,w", [("frontalface_alt", 32, 32), ("frontalface_alt", 120, 32), ("frontalface_default", 60, 35),
                                      ("frontalface_alt2", 120, 32), ("frontalface_alt_tree", 120, 32), ("mcs_mouth", 80, 37)])
def test_level_verdicts_match_the_oracle_walk(oracle, cascades, casc, h, w):
    """A frame with ONE factor (factor * win_w < W - 10 only for factor = 1) and ystep 2: the scale-cascade walk visits a subset of
    the exhaustive grid at the same scale.  Replaying its skip rule over the new oracle's verdicts must give its rectangles, its
    window count and — for linear cascades, where a verdict -i tells the stages entered — its stage counts."""
    _, a = cascades(casc)
    for seed in range(4):
        f = synth.frame(("smooth", "noise", "blocks", "smooth")[seed], seed, h, w)
        v, _ = so.level_verdicts(a, f, 2)
        ro, st = oracle.detect_opencvlike(a, f)
        assert set(ro["scale_idx"].tolist()) <= {0}
        # the walk: endX = cvRound((W - win_w) / 2) positions, border rule x + win_w >= W + 1 (never here: x <= W - win_w)
        end_x, end_y = round_half_even((w - a.win_w) / 2), round_half_even((h - a.win_h) / 2)
        assert end_x <= v.shape[1] and end_y <= v.shape[0]      # every position the walk can visit is on the exhaustive grid
        hits, windows, entered = [], 0, np.zeros(a.n_stages, np.int64)
        is_tree = bool(np.any(a.stage_next != -1))
        for iy in range(end_y):
            ix = 0
            while ix < end_x:
                windows += 1
                r = int(v[iy, ix])
                entered[:(a.n_stages if r > 0 else -r + 1)] += 1
                if r > 0:
                    hits.append((0, 2 * ix, 2 * iy, a.win_w, a.win_h))
                ix += 2 if r == 0 else 1
        assert sorted(hits) == rows(ro) and windows == st["windows"]
        if not is_tree:
            assert entered.tolist() == st["stage_entered"]


def round_half_even(v: float) -> int:
    return int(np.rint(v))


def test_gpu_premises(oracle, cascades):
    """Every frame / cascade pair of the GPU file: at least 10 raw rectangles on at least three levels, and a result that differs
    from the scale-cascade path's (so the parent commit, which ignores the flag, fails the GPU comparisons)."""
    def check(a, f, **kw):
        r, st = so.detect_scale_image(a, f, **kw)
        assert len(r) >= 10 and st["n_levels"] >= 3, (len(r), st["n_levels"])
        ro, sto = oracle.detect_opencvlike(a, f, **kw)
        assert rows(r) != rows(ro) and st["windows"] != sto["windows"]
        return r, st
    for casc, seeds in so.CASES.items():
        _, a = cascades(casc)
        for s in seeds:
            r, _ = check(a, so.faces_frame(s, so.FRAME_H, so.FRAME_W))
            assert len(set(r["scale_idx"].tolist())) >= 3
    _, a = cascades("frontalface_alt")
    for seed, kw in so.PARAM_CASES:
        check(a, so.faces_frame(seed, so.FRAME_H, so.FRAME_W), **kw)
    r, st = check(a, so.face_grid_frame(so.GRID_SEED), scale_factor=2.0)
    assert (160, 120) in st["levels"] and any(w * 2.0 > 2 * 20 for w in r["w"])    # the 2:1 area level, and a level with ystep = 1
    _, st = so.detect_scale_image(a, so.faces_frame(7, so.FRAME_H, so.FRAME_W), min_size=(40, 40))
    assert st["levels"][0] != (so.FRAME_W, so.FRAME_H)                             # leading levels skipped


def test_level_enumeration_and_grid(cascades):
    """240 x 180, 20 x 20, factor 1.1: level k is (cvRound(240 / 1.1^k), cvRound(180 / 1.1^k)); the loop ends at the first level
    lower than the window; windows = sum of ceil((w - 20) / ystep) * ceil((h - 20) / ystep)."""
    _, a = cascades("frontalface_alt")
    _, st = so.detect_scale_image(a, synth.frame("smooth", 1, 180, 240))
    want, f, windows = [], 1.0, 0
    while True:
        w, h = round_half_even(240 / f), round_half_even(180 / f)
        if w - 20 + 1 <= 0 or h - 20 + 1 <= 0:
            break
        want.append((w, h))
        step = 1 if f > 2 else 2
        windows += len(range(0, w - 20, step)) * len(range(0, h - 20, step))
        f *= 1.1
    assert st["levels"] == want and st["windows"] == windows
