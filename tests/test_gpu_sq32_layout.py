"""vj_detect and vj_stream on the u32 layout of the squared integral (values mod 2^32) against the C oracle
and against the same frames with VJ_SQ32=0, which keeps the u64 layout: rectangles, per-stage counts and windows, bit for bit.

Scales whose window holds at most 66 051 pixels read four dwords of the u32 image; larger windows walk their variance rectangle
in strips (csrc/vj_sq_strips.hpp).  The cases keep scales on both sides of that limit:
  * frontalface_alt on frames of about 300 x 300 and 400 x 320, the scales from 163 pixels up (a scale mask: windows of 163 ...
    288 pixels, the last two beyond the limit, the last one with a variance rectangle of 260 x 260 = two strips);
  * a crafted cascade from cases.geometry_cascade with a 257 x 257 base window and scale factor 1.004: windows of 257 (66 049
    pixels, the last dword scale), 258, 259, ... 262 pixels; its node thresholds are set to small negative values (they are 0 as
    crafted), so that a window's variance decides its nodes.
Content is bright, so that the squared sums are large: all 255, 255 with 1 % of the pixels 0, 255 with black blocks, and {0, 255}
noise.  Before anything runs on the GPU the test asserts on the CPU that several hundred visited windows of the strip scales
have a true squared sum of 2^32 or more and that a frame's full squared integral exceeds 2^32: a wrong high part cannot pass."""
import os

import numpy as np
import pytest

from cases import cascade_to_product, first_difference, geometry_cascade, rows_of, tunables
from clfacedetection_amd import VJ_FLAG_COUNTERS, Environment, default_params

pytestmark = pytest.mark.gpu

SQ32_MAX_AREA = 66051
SHAPES = {"300": (300, 300), "400x320": (320, 400)}           # (height, width)
ALT_MIN = (150, 150)                                         # frontalface_alt: the scales from 163 x 163 pixels up
GEO = dict(scale_factor=1.004, max_size=(262, 262))
# node thresholds of the crafted cascade (times the window's standard deviation, about 25 on the 1 % frame): of that frame's
# 2486 windows at 300 x 300 the oracle passes 1818 through the first stage and 1105 through the second
GEO_THRESHOLDS = (-0.0003, -0.0001, -0.0002)
SETTINGS = [(), (("concurrent", 0),), (("tile_accept_windows", 65536),), (("concurrent", 0), ("tile_accept_windows", 65536))]

_CACHE = {}


def frames_of(shape):
    """Four distinct bright frames: 1 % black pixels, all 255, {0, 255} noise, black blocks on 255."""
    if shape not in _CACHE:
        h, w = SHAPES[shape]
        rng = np.random.default_rng(h * 7 + w)
        sparse = np.where(rng.random((h, w)) < 0.01, 0, 255).astype(np.uint8)
        noise = rng.integers(0, 2, (h, w), dtype=np.uint8) * np.uint8(255)
        blocks = np.full((h, w), 255, np.uint8)
        for _ in range(6):
            y, x = int(rng.integers(0, h - 12)), int(rng.integers(0, w - 12))
            blocks[y:y + 12, x:x + 12] = 0
        _CACHE[shape] = np.stack([sparse, np.full((h, w), 255, np.uint8), noise, blocks])
    return _CACHE[shape]


def case(oracle, cascades, casc, shape):
    """(product cascade, oracle arrays, product params, counted params, oracle keyword arguments, accepted oracle scales)."""
    key = ("case", casc, shape)
    if key not in _CACHE:
        h, w = SHAPES[shape]
        if casc == "frontalface_alt":
            c, a = cascades(casc)
            scales = [s for s in oracle.plan_scales(a, w, h, ALT_MIN, (0, 0)) if s.accepted and s.nx > 0 and s.ny > 0]
            kw = dict(scales=[s.scale_idx for s in scales])          # the product takes the mask, the oracle the size limit
            okw = dict(min_size=ALT_MIN)
        else:
            a = geometry_cascade(257, 257, "upright")
            a.node_threshold = np.array([GEO_THRESHOLDS[k % 3] for k in range(a.n_nodes)], np.float32)
            c = cascade_to_product(a)
            scales = [s for s in oracle.plan_scales(a, w, h, (0, 0), GEO["max_size"], GEO["scale_factor"]) if s.accepted and s.nx > 0 and s.ny > 0]
            kw = dict(scale_factor=GEO["scale_factor"], max_w=GEO["max_size"][0], max_h=GEO["max_size"][1])
            okw = dict(max_size=GEO["max_size"], scale_factor=GEO["scale_factor"])
            assert [s.win_w for s in scales[:2]] == [257, 258]
        _CACHE[key] = (c, a, default_params(**kw), default_params(flags=VJ_FLAG_COUNTERS, **kw), okw, scales)
    return _CACHE[key]


def oracle_of(oracle, cascades, casc, shape):
    key = ("oracle", casc, shape)
    if key not in _CACHE:
        _, a, _, _, okw, _ = case(oracle, cascades, casc, shape)
        _CACHE[key] = [oracle.detect(a, f, **okw) for f in frames_of(shape)]
    return _CACHE[key]


def assert_large_squared_sums(oracle, cascades, casc, shape):
    """On the CPU: the strip scales' visited windows whose TRUE squared sum needs more than 32 bits, over the four frames."""
    scales = case(oracle, cascades, casc, shape)[5]
    below = [s for s in scales if s.win_w * s.win_h <= SQ32_MAX_AREA]
    strips = [s for s in scales if s.win_w * s.win_h > SQ32_MAX_AREA]
    assert below and strips, f"{casc} {shape}: scales on both sides of {SQ32_MAX_AREA} pixels: {[(s.win_w, s.win_h) for s in scales]}"
    assert any(-(-s.equ_h // (SQ32_MAX_AREA // s.equ_w)) >= 2 for s in strips), "no scale walks more than one strip"
    big = 0
    for f in frames_of(shape):
        q = np.zeros((f.shape[0] + 1, f.shape[1] + 1), np.uint64)
        np.cumsum(np.cumsum(f.astype(np.uint64) ** 2, axis=0), axis=1, out=q[1:, 1:])
        for s in strips:
            xs = np.rint(np.arange(s.nx, dtype=np.float32) * np.float32(s.step)).astype(np.int64) + s.equ_x    # lrint(i * step), f32 product
            ys = np.rint(np.arange(s.ny, dtype=np.float32) * np.float32(s.step)).astype(np.int64) + s.equ_y
            y0, x0 = np.meshgrid(ys, xs, indexing="ij")
            v = q[y0 + s.equ_h, x0 + s.equ_w] - q[y0 + s.equ_h, x0] - q[y0, x0 + s.equ_w] + q[y0, x0]
            big += int((v >= np.uint64(2**32)).sum())
    full = max(int((f.astype(np.uint64) ** 2).sum()) for f in frames_of(shape))
    assert full >= 2**32, f"{shape}: the largest full squared integral is {full}"
    return big


@pytest.fixture(scope="module")
def env_u64():
    """A second environment created with VJ_SQ32=0 (read when one is created): 64-bit corners on the u64 layout."""
    old = os.environ.get("VJ_SQ32")
    os.environ["VJ_SQ32"] = "0"
    try:
        e = Environment(0)
    finally:
        if old is None:
            del os.environ["VJ_SQ32"]
        else:
            os.environ["VJ_SQ32"] = old
    yield e
    e.close()


def check(e, c, frames, want, p_timed, p_counted, label):
    """A counted and a timed vj_detect against the oracle's per-frame results; returns the counted result."""
    r = e.detect(c, frames, p_counted)
    entered, windows = [0] * c.info.n_stages, 0
    for i, (ro, st) in enumerate(want):
        mine = rows_of(r.rects[r.rects["frame"] == i])
        assert mine == rows_of(ro), f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: {first_difference(r.stage_entered, entered)}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"
    r2 = e.detect(c, frames, p_timed)
    assert np.array_equal(r2.rects, r.rects), f"{label}: the timed kernels' rectangles differ from the counted ones"
    return r


def test_cases_reach_squared_sums_beyond_32_bits(oracle, cascades):
    """(CPU arithmetic only.)  Summed over the cases: hundreds of strip-scale windows beyond 2^32 per cascade."""
    for casc in ("frontalface_alt", "geometry"):
        big = {shape: assert_large_squared_sums(oracle, cascades, casc, shape) for shape in SHAPES}
        print(f"{casc}: strip-scale windows with a true squared sum >= 2^32: {big}")
        assert big["300"] >= 1 and sum(big.values()) >= (300 if casc == "geometry" else 20), (casc, big)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("casc", ["frontalface_alt", "geometry"])
def test_detect_matches_the_oracle_and_the_u64_layout(env, env_u64, oracle, cascades, casc, shape, n):
    big = assert_large_squared_sums(oracle, cascades, casc, shape)
    assert big >= (300 if casc == "geometry" else 1), (casc, shape, big)
    c, _, p, pc, _, _ = case(oracle, cascades, casc, shape)
    sel = slice(0, 1) if n == 1 else slice(1, 4)
    frames, want = frames_of(shape)[sel], oracle_of(oracle, cascades, casc, shape)[sel]
    assert any(0 < st["stage_entered"][1] < st["windows"] for _, st in want), "the first stage decides nothing on these frames"
    for settings in SETTINGS:
        label = f"{casc} {shape} n={n} {dict(settings)}"
        out = []
        for e, name in ((env, "u32 layout"), (env_u64, "VJ_SQ32=0")):
            with tunables(e, *settings):
                out.append(check(e, c, frames, want, p, pc, f"{label} {name}"))
        assert np.array_equal(out[0].rects, out[1].rects), label
        assert (out[0].stage_entered, out[0].windows) == (out[1].stage_entered, out[1].windows), label
        if ("tile_accept_windows", 65536) in settings:
            assert not any(l["kind"] == "tile" for l in out[0].launches), f"{label}: {[l['kind'] for l in out[0].launches]}"


@pytest.mark.parametrize("casc", ["frontalface_alt", "geometry"])
def test_sub_batches(env, env_u64, oracle, cascades, casc):
    """max_subbatch 2 with four frames: two integrals and two cascade runs behind one call, each on the call's layout."""
    c, _, p, pc, _, _ = case(oracle, cascades, casc, "300")
    frames, want = frames_of("300"), oracle_of(oracle, cascades, casc, "300")
    out = []
    for e, name in ((env, "u32 layout"), (env_u64, "VJ_SQ32=0")):
        with tunables(e, ("max_subbatch", 2)):
            out.append(check(e, c, frames, want, p, pc, f"{casc} sub-batches {name}"))
    assert np.array_equal(out[0].rects, out[1].rects)


@pytest.mark.parametrize("casc", ["frontalface_alt", "geometry"])
def test_stream_with_two_batches_in_flight(env, env_u64, oracle, cascades, casc):
    """vj_stream: two different batches submitted before the first is collected (they share the integral buffers), each
    against the oracle, on both layouts."""
    c, _, p, _, _, _ = case(oracle, cascades, casc, "400x320")
    frames, want = frames_of("400x320"), oracle_of(oracle, cascades, casc, "400x320")
    h, w = SHAPES["400x320"]
    batches = (slice(0, 2), slice(2, 4))
    for e, name in ((env, "u32 layout"), (env_u64, "VJ_SQ32=0")):
        s = e.stream(c, w, h, 2, p)
        try:
            for _ in range(2):          # (the second round reuses both lanes)
                for b in batches:
                    s.submit(frames[b])
                for b in batches:
                    r = s.collect()
                    for i, (ro, _) in enumerate(want[b]):
                        mine = rows_of(r.rects[r.rects["frame"] == i])
                        assert mine == rows_of(ro), f"{casc} stream {name}: batch {b}, frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        finally:
            s.close()
