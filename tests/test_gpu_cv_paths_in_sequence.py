"""The four launch paths of vj_detect_opencv one after the other on ONE environment.  The paths share their two-stream fork and join,
the reject bitmap and its memsets, the tile ticket counters and the detection buffer (csrc/vj_cv.cpp: begin_cv_tiles / end_cv_tiles,
launch_cv_tile_classes, enqueue_cv_attempt), so a path that leaves state behind for the next one is how they can go wrong together.
Every visit is compared exactly with the restatement of its mode — the oracle's oc_detect_opencvlike as
test_gpu_opencv_profile.py::test_lds_tile_path_equals_the_row_kernel_and_the_oracle does, tests/scale_image_oracle.c,
tests/canny_oracle.c — and with the first visit of the same path.

The frames are 300 x 420, the smallest cell of that test whose plans put scales on tiles AND keep a rest on the row kernel (asserted
from cv_plan_info below), in a batch of 3 with max_subbatch 2: a sub-batch boundary falls inside every call."""
import numpy as np
import pytest

import canny_oracle as co
import scale_image_oracle as so
from cases import make_frame
from clfacedetection_amd import VJ_FLAG_CV_CANNY_PRUNING, VJ_FLAG_CV_SCALE_IMAGE, Environment

pytestmark = pytest.mark.gpu
H, W, BATCH = 300, 420, 3
# (name, cascade, flags, cv_tiles)
VISITS = (("plain tiles", "frontalface_alt", 0, 1),
          ("scale-image tiles", "frontalface_alt", VJ_FLAG_CV_SCALE_IMAGE, 1),
          ("stage-tree tiles", "frontalface_alt_tree", 0, 1),
          ("canny pruning on tiles", "frontalface_alt", VJ_FLAG_CV_CANNY_PRUNING, 1),
          ("rows only", "frontalface_alt", 0, 0))


def rows(rects):
    return sorted(tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects)


@pytest.fixture(scope="module")
def frames(oracle):
    return np.stack([make_frame(k, 310 + i, H, W, oracle) for i, k in enumerate(("faces", "noise", "blocks"))])


@pytest.fixture(scope="module")
def expected(oracle, cascades, frames):
    """visit name -> per frame, the restatement's rectangles (computed once, left unchanged)"""
    alt, tree = cascades("frontalface_alt")[1], cascades("frontalface_alt_tree")[1]
    want = {"plain tiles": [rows(oracle.detect_opencvlike(alt, f)[0]) for f in frames],
            "scale-image tiles": [rows(so.detect_scale_image(alt, f)[0]) for f in frames],
            "stage-tree tiles": [rows(oracle.detect_opencvlike(tree, f)[0]) for f in frames],
            "canny pruning on tiles": [rows(co.detect_opencvlike(alt, f)[0]) for f in frames]}
    want["rows only"] = want["plain tiles"]
    assert all(sum(len(r) for r in per_frame) >= 20 for per_frame in want.values())   # (no visit compares empty lists)
    return want


def n_scales(c):
    """The factors cvHaarDetectObjects enumerates for an H x W frame (tempcv.cpp:1344-1349)"""
    n, factor = 0, 1.0
    while factor * c.info.win_w < W - 10 and factor * c.info.win_h < H - 10:
        n, factor = n + 1, factor * 1.1
    return n


@pytest.mark.parametrize("concurrent", [1, 0])
def test_every_launch_path_in_sequence_on_one_environment(cascades, frames, expected, concurrent):
    env = Environment(0)
    try:
        env.configure("max_subbatch", 2)
        env.configure("concurrent", concurrent)
        first = {}
        for name, casc, flags, cv_tiles in VISITS + VISITS[::-1]:
            c = cascades(casc)[0]
            env.configure("cv_tiles", cv_tiles)   # (the one setting that is not a flag of the call: what "rows only" means)
            # the path this visit takes: scales on tiles with a rest on the row kernel — a stage tree with its survivor queue —, or none
            info = env.cv_plan_info(c, W, H, BATCH, flags=flags)
            if cv_tiles:
                assert 0 < info.n_tile_scales < n_scales(c), (name, info.n_tile_scales)
                assert (info.tree_queue in (1, 2)) == (name == "stage-tree tiles"), (name, info.tree_queue)
            else:
                assert info.n_tile_scales == 0 and info.tree_queue == 0, name
            r = env.detect_opencv(c, frames, flags=flags)
            for f in range(BATCH):
                assert rows(r.rects[r.rects["frame"] == f]) == expected[name][f], (name, concurrent, f, name in first)
            if name in first:
                assert np.array_equal(r.rects, first[name]), (name, concurrent)
            first.setdefault(name, r.rects.copy())
    finally:
        env.close()
