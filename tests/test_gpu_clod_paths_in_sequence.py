"""Every driver path of the clod profile one after the other on ONE environment.  The paths share the lane's counters block and its
ticket ranges, the detection buffer, the region buffers and their caps, the fork / join events and the plan cache (csrc/vj_detect.cpp:
enqueue_cascade and its steps, finish_batch, the stream; csrc/vj_detect_regions.cpp: run_region_pass_until_fit), so a step that
leaves state behind for the next one is how they can go wrong together.  Every visit is compared exactly with the oracle restatement
test_gpu_detect.py and test_gpu_modes.py use for that call — oc_detect in the visit's mode on the frame or on the region's sub-image,
the oracle's grouping of the oracle's candidates — and with the first visit of the same path; counted visits compare stage_entered too.

The frames are 300 x 420, the smallest of the sizes those tests use at which the plan of frontalface_alt puts scales on tiles AND
keeps gather units (asserted below from plan_tiles and from the result's launch list), in a batch of 3 with max_subbatch 2 — a
sub-batch boundary falls inside every call — and a detection buffer of ONE entry before every visit, so that every overflow-and-redo
loop runs (finish_batch's, the chain's, a stream lane's)."""
import numpy as np
import pytest

from cases import make_frame
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_SKIP_LIST, VJ_FLAG_SKIP_ROW, Environment, default_params

pytestmark = pytest.mark.gpu
H, W, BATCH = 300, 420, 3
# regions of three sizes for the detect_rois visits: (frame, x, y, w, h)
ROIS = [(0, 10, 20, 200, 180), (0, 180, 60, 230, 230), (1, 0, 0, 420, 300), (1, 100, 90, 200, 180), (2, 150, 40, 230, 230), (2, 5, 5, 200, 180)]
# (name, call, first cascade, second cascade, first cascade's min_neighbors, flags of the (last) cascade, group_max, rois_on_device)
VISITS = (("detect alt", "detect", "frontalface_alt", None, 0, 0, None, 1),
          ("detect alt_tree", "detect", "frontalface_alt_tree", None, 0, 0, None, 1),
          ("detect alt2", "detect", "frontalface_alt2", None, 0, 0, None, 1),
          ("detect skip list", "detect", "frontalface_alt", None, 0, VJ_FLAG_SKIP_LIST, None, 1),
          ("detect counted", "detect", "frontalface_alt", None, 0, VJ_FLAG_COUNTERS, None, 1),
          ("rois on device", "rois", "eye", None, 0, VJ_FLAG_COUNTERS, None, 1),
          ("rois per size", "rois", "eye", None, 0, VJ_FLAG_COUNTERS, None, 0),
          ("chain raw", "chain", "frontalface_alt2", "eye", 0, VJ_FLAG_COUNTERS, None, 1),
          ("chain grouped", "chain", "frontalface_alt2", "eye", 3, VJ_FLAG_COUNTERS, None, 1),
          ("chain grouped on the host", "chain", "frontalface_alt2", "eye", 3, VJ_FLAG_COUNTERS, 1, 1),
          ("chain skip row", "chain", "frontalface_alt2", "eye", 0, VJ_FLAG_COUNTERS | VJ_FLAG_SKIP_ROW, None, 1),
          ("stream", "stream", "frontalface_alt", None, 0, 0, None, 1))
ORACLE_MODE = {0: None, VJ_FLAG_COUNTERS: None, VJ_FLAG_SKIP_LIST: 2, VJ_FLAG_COUNTERS | VJ_FLAG_SKIP_ROW: 3}   # (None: the cascade's own walk)


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


@pytest.fixture(scope="module")
def frames(oracle):
    return np.stack([make_frame(k, 310 + i, H, W, oracle) for i, k in enumerate(("faces", "noise", "blocks"))])


def _inside(oracle, arr, frames, regions, mode):
    """The oracle on every region's sub-image: per region its rows, and stage_entered summed over the regions"""
    per_region, entered = [], None
    for f, x, y, w, h in regions:
        ro, st = oracle.detect(arr, np.ascontiguousarray(frames[f][y:y + h, x:x + w]), mode=mode)
        per_region.append(rows(ro))
        e = np.array(st["stage_entered"], np.int64)
        entered = e if entered is None else entered + e
    return per_region, (entered.tolist() if entered is not None else None)


@pytest.fixture(scope="module")
def expected(oracle, cascades, frames):
    """visit name -> what the oracle says (computed once, left unchanged).  detect / stream: per frame the rows, stage_entered summed;
    rois: per region the rows, stage_entered; chain: the first result as (x, y, w, h, weight or 0, frame), then the same per region."""
    want, on_frames = {}, {}
    for name, call, c1, c2, mn, flags, _, _ in VISITS:
        a1 = cascades(c1)[1]
        mode = ORACLE_MODE[flags]
        if call in ("detect", "stream"):
            if (c1, mode) not in on_frames:
                on_frames[c1, mode] = [oracle.detect(a1, f, mode=mode) for f in frames]
            res = on_frames[c1, mode]
            want[name] = ([rows(ro) for ro, _ in res], np.sum([st["stage_entered"] for _, st in res], 0).tolist())
            assert sum(len(r) for r in want[name][0]) >= 10, name   # (no visit compares empty lists)
        elif call == "rois":
            want[name] = _inside(oracle, a1, frames, ROIS, mode)
            assert sum(len(r) for r in want[name][0]) >= 10, name
        else:
            first = []
            for f in range(BATCH):
                ro, _ = oracle.detect(a1, frames[f])
                if mn:
                    xywh = np.stack([ro[k] for k in ("x", "y", "w", "h")], 1) if len(ro) else np.zeros((0, 4), np.int32)
                    g, wt = oracle.group_rectangles(xywh, mn)
                    first += [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(n), f) for r, n in zip(g, wt)]
                else:   # the raw result's order: (frame, scale, y, x)
                    first += [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), 0, f) for r in sorted(ro, key=lambda r: (r["scale_idx"], r["y"], r["x"]))]
            regions = [(f, x, y, w, h) for x, y, w, h, _, f in first]
            want[name] = (first,) + _inside(oracle, cascades(c2)[1], frames, regions, mode)
            assert len(first) >= 3 and sum(len(r) for r in want[name][1]) >= 1, name   # (grouped faces hold few eyes: stage_entered says more)
    # a frame must overflow group_max = 1 for the host route of the grouped chain: more than one raw candidate in it
    assert max(len(oracle.detect(cascades("frontalface_alt2")[1], f)[0]) for f in frames) > 1
    return want


def _check_chain(r1, r2, want, name):
    first, per_region, entered = want
    assert [(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"]), int(r["weight"]), int(r["frame"])) for r in r1.rects] == first, name
    for i in range(len(first)):
        assert rows(r2.rects[r2.rects["frame"] == i]) == per_region[i], (name, i)
    assert len(r2.rects) == sum(len(r) for r in per_region) and r2.stage_entered == entered, name


@pytest.mark.parametrize("concurrent", [1, 0])
def test_every_clod_driver_path_in_sequence_on_one_environment(cascades, frames, expected, concurrent):
    env = Environment(0)
    try:
        first = {}
        for name, call, c1, c2, mn, flags, group_max, rois_on_device in VISITS + VISITS[::-1]:
            for key, value in (("max_subbatch", 2), ("concurrent", concurrent), ("det_cap", 1), ("rois_on_device", rois_on_device),
                               ("group_max", group_max or 2048)):
                env.configure(key, value)
            casc = cascades(c1)[0]
            p = default_params(flags=flags)
            if call == "detect":
                r = env.detect(casc, frames, p)
                got = [r.rects]
                for f in range(BATCH):
                    assert rows(r.rects[r.rects["frame"] == f]) == expected[name][0][f], (name, concurrent, f, name in first)
                if flags & VJ_FLAG_COUNTERS:
                    assert r.stage_entered == expected[name][1], name
                if name == "detect alt":   # the path the frame size was chosen for: tile launches AND the gather chain
                    info, tiles = casc.plan_tiles(W, H, BATCH, tile_split=-1.0)
                    assert sum(info.class_tiles) > 0 and info.cut.gather_units > 0
                    assert {"tile", "grid", "queue"} <= {l["kind"] for l in r.launches}, r.launches
            elif call == "rois":
                r = env.detect_rois(casc, frames, ROIS, p)
                got = [r.rects]
                for i in range(len(ROIS)):
                    assert rows(r.rects[r.rects["frame"] == i]) == expected[name][0][i], (name, concurrent, i)
                assert r.stage_entered == expected[name][1], name
            elif call == "chain":
                r1, r2 = env.detect_chain(casc, cascades(c2)[0], frames, default_params(min_neighbors=mn), p)
                got = [r1.rects, r2.rects]
                _check_chain(r1, r2, expected[name], name)
            else:   # two batches submitted, then two collected (a stream's batch fits one launch sequence: max_subbatch frames)
                st = env.stream(casc, W, H, 2, p)
                try:
                    st.submit(frames[:2])
                    st.submit(frames[1:])
                    got = [st.collect().rects, st.collect().rects]
                finally:
                    st.close()
                for b, f0 in enumerate((0, 1)):
                    for f in range(2):
                        assert rows(got[b][got[b]["frame"] == f]) == expected[name][0][f0 + f], (name, concurrent, b, f)
            assert all(len(g) > 0 for g in got), name
            if name in first:
                assert all(np.array_equal(a, b) for a, b in zip(got, first[name])), (name, concurrent)
            first.setdefault(name, [g.copy() for g in got])
    finally:
        env.close()
