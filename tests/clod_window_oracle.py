"""Test restatement, in numpy, of the clod profile's path for ONE window at an arbitrary binary32 scale — setupScale's geometry
(clod.cpp:371-415 without the loop-side rejections), computeVariance (:418-446), the stage sums of clod.cl:49-82 on the node table
of precomputeKernelCascade (:529-578; taken from the committed oracle's oc_feature_table) and runCascade's return value (:736-787;
stage trees: the walk of tempcv.cpp:834-861) — and the window lists and frames of the GPU cases (tests/test_gpu_clod_windows.py),
whose premises tests/test_clod_windows_cpu.py asserts.  Windows are vectors; every f32 operation is rounded on its own."""
from __future__ import annotations

import numpy as np

from oracle import np_oracle
from oracle.oracle import CascadeArrays, OcScale, Oracle
from scale_image_oracle import faces_frame

F = np.float32
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
OUTSIDE = INT32_MIN                  # VJ_WINDOW_OUTSIDE
WIN_MAX = 1 << 20                    # sw / sh are clamped here
FRAME_H, FRAME_W = 180, 240

# the cascades of the GPU cases -> seed of scale_image_oracle.faces_frame at 180 x 240: the first seed from 1 upwards whose full
# list shows the premises (list_premises; tests/test_clod_windows_cpu.py asserts them).  eye_tree_eyeglasses: the drawn faces have
# no eyes it accepts — no seed of 1 .. 29 gives a pass —, so its seed is the first with a reject in one of its last three stages,
# and its passes and late stages are reached with start_stage instead (EYE_START_STAGES).
SEEDS = {
    "frontalface_alt": 1,
    "frontalface_alt2": 1,
    "eye_tree_eyeglasses": 17,
    "frontalface_alt_tree": 1,
    "mcs_mouth": 1,
}
TILTED = ("eye_tree_eyeglasses", "mcs_mouth")       # need VJ_FLAG_TILTED_AS_UPRIGHT
CHAIN_STEPS = (0, 3, 6, 9)          # members of the chain 1.1f^k (the floats of the enumeration: repeated f32 multiplication)
OFF_CHAIN = (2.5, 1.37)             # 2.5: round() ties (5 * 2.5 = 12.5, 3 * 2.5 = 7.5, ...: half away from zero)
SHUFFLE_SEED, N_DUPLICATES = 5, 64
EYE_START_STAGES = (20, 25, 29)
BATCH_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8, 9)   # nine distinct frames
_ORACLE = None


def _oracle() -> Oracle:
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = Oracle()
    return _ORACLE


def round_half_away(v) -> int:
    """(cl_uint)round(v) of a non-negative f32, clamped to WIN_MAX before the conversion."""
    v = float(v)
    return int(np.floor(v + 0.5)) if v < WIN_MAX else WIN_MAX


def geometry(c: CascadeArrays, scale) -> dict:
    """setupScale (clod.cpp:387-388, :404-408) for current_scale = float32(scale): int x f32 products, rounded half away from zero."""
    s = F(scale)
    g = {"scale": s,
         "sw": round_half_away(F(F(c.win_w) * s)), "sh": round_half_away(F(F(c.win_h) * s)),
         "ex": round_half_away(s),
         "ew": round_half_away(F(F(c.win_w - 2) * s)), "eh": round_half_away(F(F(c.win_h - 2) * s))}
    g["area"] = g["ew"] * g["eh"]
    return g


def chain_scale(k: int, scale_factor: float = 1.1) -> np.float32:
    s = F(1)
    for _ in range(k):
        s = F(s * F(scale_factor))
    return s


def case_scales() -> list:
    return [chain_scale(k) for k in CHAIN_STEPS] + [F(v) for v in OFF_CHAIN]


class ClodWindowOracle:
    """The cascade on one gray frame: run(xy, scale, start_stage, signed_mean) -> (results int32, stage sums f32, variances f32)."""

    def __init__(self, c: CascadeArrays, gray: np.ndarray):
        assert gray.dtype == np.uint8 and gray.ndim == 2
        self.c = c
        self.H, self.W = gray.shape
        self.stride = self.W + 1
        ii, qq = np_oracle.integral(gray)
        pad = 3 * self.stride                                              # slack rows: a feature may overshoot its window by one
        self.ii = np.concatenate([ii.reshape(-1), np.zeros(pad, np.uint32)])
        self.qq = np.concatenate([qq.reshape(-1), np.zeros(pad, np.uint64)])
        self.present = c.node_weight.reshape(-1, 3) != 0
        self.linear = bool(np.all(c.stage_next == -1))
        self._tables = {}

    def table(self, g: dict):
        key = F(g["scale"]).tobytes()
        if key not in self._tables:
            sc = OcScale()
            sc.scale, sc.area = float(g["scale"]), g["area"]
            self._tables[key] = _oracle().feature_table(self.c, sc, self.W)   # (n_nodes, 3, 4) element offsets lt rt lb rb; (n_nodes, 3) weights
        return self._tables[key]

    def _node_sum(self, tab, n: int, o: np.ndarray) -> np.ndarray:
        """clod.cl:60-76: u32 corner sums, one f32 multiply per rectangle, added in rectangle order."""
        off, wts = tab
        tot = None
        for q in range(3):
            if q == 2 and not self.present[n, 2]:
                break
            lt, rt, lb, rb = (int(v) for v in off[n, q])
            v = (self.ii[o + lt] - self.ii[o + rt] - self.ii[o + lb] + self.ii[o + rb]).astype(np.uint32)
            t = (v.astype(F) * wts[n, q]).astype(F)
            tot = t if tot is None else (tot + t).astype(F)
        return tot

    def stage_leaves(self, tab, stage: int, o: np.ndarray, var: np.ndarray) -> np.ndarray:
        """(windows, trees): the leaf value every tree of the stage gives every window."""
        c = self.c
        t0, nt = int(c.stage_first_tree[stage]), int(c.stage_n_trees[stage])
        out = np.zeros((len(o), nt), F)
        for t in range(t0, t0 + nt):
            n0, nn, a0 = int(c.tree_first_node[t]), int(c.tree_n_nodes[t]), int(c.tree_first_alpha[t])
            if nn == 1:                                                    # clod.cl:81: alpha[rect_sum >= norm_threshold]
                thr = (c.node_threshold[n0] * var).astype(F)
                out[:, t - t0] = np.where(self._node_sum(tab, n0, o) >= thr, c.alpha[a0 + 1], c.alpha[a0])
                continue
            cur = np.zeros(len(o), np.int64)                               # tempcv.cpp:771-792 in f32
            val = np.zeros(len(o), F)
            done = np.zeros(len(o), bool)
            for k in range(nn):
                m = np.flatnonzero(~done & (cur == k))
                if len(m) == 0:
                    continue
                thr = (c.node_threshold[n0 + k] * var[m]).astype(F)
                nxt = np.where(self._node_sum(tab, n0 + k, o[m]) < thr, int(c.node_left[n0 + k]), int(c.node_right[n0 + k]))
                leaf = nxt <= 0
                val[m[leaf]] = c.alpha[a0 - nxt[leaf]]
                done[m[leaf]] = True
                cur[m[~leaf]] = nxt[~leaf]
            out[:, t - t0] = val
        return out

    def stage_sum(self, tab, stage, o, var):
        return np_oracle.in_order_sum(self.stage_leaves(tab, stage, o, var))   # one f32 accumulator, in tree order (clod.cl:81)

    def run(self, xy, scale, start_stage: int = 0, signed_mean: bool = False):
        c = self.c
        p = np.asarray(xy, np.int64).reshape(-1, 2)
        x, y = p[:, 0], p[:, 1]
        g = geometry(c, scale)
        assert g["sw"] > 0 and g["sh"] > 0 and g["area"] > 0, "the reference divides by zero here"
        res = np.full(len(p), OUTSIDE, np.int64)
        sums = np.zeros(len(p), F)
        variances = np.zeros(len(p), F)
        inside = (x >= 0) & (y >= 0) & (x + g["sw"] <= self.W) & (y + g["sh"] <= self.H)
        idx = np.flatnonzero(inside)
        if len(idx) == 0:
            return res.astype(np.int32), sums, variances
        o_all = y[idx] * self.stride + x[idx]
        # computeVariance (clod.cpp:418-446)
        a = o_all + g["ex"] * self.stride + g["ex"]
        b, cc, d = a + g["ew"], a + g["eh"] * self.stride, a + g["eh"] * self.stride + g["ew"]
        S = (self.ii[a] - self.ii[b] - self.ii[cc] + self.ii[d]).astype(np.uint32)
        Q = (self.qq[a] - self.qq[b] - self.qq[cc] + self.qq[d]).astype(np.uint64)
        area = F(g["area"])
        mean = ((S.astype(np.int32).astype(F) if signed_mean else S.astype(F)) / area).astype(F)
        var_raw = ((Q.astype(F) / area).astype(F) - (mean * mean).astype(F)).astype(F)
        with np.errstate(invalid="ignore"):
            var_all = np.where(var_raw >= 0, np.sqrt(np.maximum(var_raw, F(0))), F(1)).astype(F)
        variances[idx] = var_all
        tab = self.table(g)
        if not self.linear:
            assert start_stage == 0, "a stage tree starts at its root"
            on_pass, on_fail = stage_links(c)
            target = np.zeros(len(idx), np.int64)                          # -1 accepted, -2 rejected
            last = np.zeros(len(idx), F)
            for stg in np_oracle._topo_order(c):
                m = np.flatnonzero(target == stg)
                if len(m) == 0:
                    continue
                ssum = self.stage_sum(tab, stg, o_all[m], var_all[m])
                last[m] = ssum
                target[m] = np.where(ssum >= c.stage_threshold[stg], on_pass[stg], on_fail[stg])
            assert np.all(target < 0)
            res[idx] = np.where(target == -1, 1, 0)
            sums[idx] = last
            return res.astype(np.int32), sums, variances
        res[idx] = 1                                                       # cl_int exit_stage = 1 (clod.cpp:752)
        alive = np.arange(len(idx))
        for stg in range(start_stage, c.n_stages):
            if len(alive) == 0:
                break
            ssum = self.stage_sum(tab, stg, o_all[alive], var_all[alive])
            sums[idx[alive]] = ssum
            failed = ssum < c.stage_threshold[stg]                         # exit_stage = -stage_index (:769-770)
            res[idx[alive[failed]]] = -stg
            alive = alive[~failed]
        return res.astype(np.int32), sums, variances


def stage_links(c: CascadeArrays):
    """tempcv.cpp:834-861 flattened: the stage after a pass / a fail of every stage; -1 accept, -2 reject."""
    on_pass = [int(v) if int(v) != -1 else -1 for v in c.stage_child]
    on_fail = []
    for s in range(c.n_stages):
        ptr = s
        while ptr != -1 and c.stage_next[ptr] == -1:
            ptr = int(c.stage_parent[ptr])
        on_fail.append(-2 if ptr == -1 else int(c.stage_next[ptr]))
    return np.array(on_pass, np.int64), np.array(on_fail, np.int64)


def run_windows(c: CascadeArrays, frames, windows, scales, start_stage: int = 0, signed_mean: bool = False):
    """What vj_run_windows must return for rows of (frame, x, y, scale index): (results, stage sums, variances)."""
    w = np.asarray(windows, np.int64).reshape(-1, 4)
    res = np.zeros(len(w), np.int32)
    sums = np.zeros(len(w), F)
    variances = np.zeros(len(w), F)
    for f in np.unique(w[:, 0]):
        o = ClodWindowOracle(c, frames[int(f)])
        for k in np.unique(w[w[:, 0] == f, 3]):
            sel = np.flatnonzero((w[:, 0] == f) & (w[:, 3] == k))
            res[sel], sums[sel], variances[sel] = o.run(w[sel, 1:3], scales[int(k)], start_stage, signed_mean)
    return res, sums, variances


def grid_of(c: CascadeArrays, scale, W: int = FRAME_W, H: int = FRAME_H) -> np.ndarray:
    """Every grid position the detector's loop gives a scale (setupScale's step and end_point, clod.cpp:384, :411-412; positions
    lrint of the f32 product index * step, :514, as np_oracle.detect forms them): (n, 2) of x, y."""
    s = F(scale)
    g = geometry(c, s)
    step = F(max(2.0, float(s)))
    nx = max(int(np.rint(np.float64(F(F(W - g["sw"]) / step)))), 0) if g["sw"] <= W else 0
    ny = max(int(np.rint(np.float64(F(F(H - g["sh"]) / step)))), 0) if g["sh"] <= H else 0
    xs = np.rint((np.arange(nx, dtype=F) * step).astype(np.float64)).astype(np.int64)
    ys = np.rint((np.arange(ny, dtype=F) * step).astype(np.float64)).astype(np.int64)
    X, Y = np.meshgrid(xs, ys)
    return np.column_stack([X.reshape(-1), Y.reshape(-1)]).astype(np.int64).reshape(-1, 2)


def full_list(c: CascadeArrays, frame: int = 0) -> np.ndarray:
    """The full grid of the four chain scales and the two scales outside the chain, shuffled with a fixed seed, its first
    N_DUPLICATES windows once more at the end: rows of (frame, x, y, scale index into case_scales())."""
    rows = []
    for k, s in enumerate(case_scales()):
        g = grid_of(c, s)
        rows.append(np.column_stack([np.full(len(g), frame), g, np.full(len(g), k)]))
    w = np.concatenate(rows)
    w = w[np.random.default_rng(SHUFFLE_SEED).permutation(len(w))]
    return np.concatenate([w, w[:N_DUPLICATES]])


def edge_list(c: CascadeArrays, frame: int = 0) -> np.ndarray:
    """Both sides of every edge of the inside test at every scale of case_scales(): x + sw in {W - 1, W, W + 1, W + 2} (W is
    evaluated, W + 1 is outside), the same for y; x = -1, 0; y = -1, 0."""
    rows = []
    for k, s in enumerate(case_scales()):
        g = geometry(c, s)
        xs = [-1, 0] + [FRAME_W + d - g["sw"] for d in (-1, 0, 1, 2)]
        ys = [-1, 0] + [FRAME_H + d - g["sh"] for d in (-1, 0, 1, 2)]
        rows += [(frame, x, y, k) for y in ys for x in xs]
    return np.array(rows, np.int64)


def extreme_list(frame: int = 0) -> np.ndarray:
    """-1, INT32_MAX and INT32_MIN in x, in y and in both, at the first and the last scale of case_scales()."""
    ext = (-1, INT32_MAX, INT32_MIN, INT32_MAX - 19, INT32_MIN + 20)
    rows = []
    for k in (0, len(case_scales()) - 1):
        rows += [(frame, e, 10, k) for e in ext] + [(frame, 10, e, k) for e in ext] + [(frame, e, e2, k) for e in ext for e2 in ext]
    return np.array(rows, np.int64)


def outside_mask(c: CascadeArrays, windows, scales, W: int = FRAME_W, H: int = FRAME_H) -> np.ndarray:
    """The inside test on rows of (frame, x, y, scale index), negated, in Python's unbounded ints."""
    out = []
    for _, x, y, k in np.asarray(windows, np.int64).reshape(-1, 4).tolist():
        g = geometry(c, scales[k])
        out.append(not (x >= 0 and y >= 0 and x + g["sw"] <= W and y + g["sh"] <= H))
    return np.array(out, bool)


def list_premises(c: CascadeArrays, res: np.ndarray) -> bool:
    """What a full list must show: linear cascades rejects at six or more distinct stages, stage 0 among them; every cascade at
    least one pass and at least one reject."""
    if not np.all(c.stage_next == -1):
        return bool((res == 1).any() and (res == 0).any())
    stages = {int(-r) for r in res if r <= 0 and r != OUTSIDE}
    return len(stages) >= 6 and 0 in stages and bool((res == 1).any())
