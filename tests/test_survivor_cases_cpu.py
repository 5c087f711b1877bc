"""The survivor-heavy cascades and frames of tests/cases.py (test_gpu_survivors.py) on the CPU: they load through the
product's loader, every window enters every stage of the all-pass prefix in both profiles of the oracle, and the
detections follow the dots rather than the window count."""
import numpy as np
import pytest

from cases import SURVIVOR_FORMS, cascade_to_product, dot_frame, survivor_cascade

CAP = 1 << 21


@pytest.mark.parametrize("form", SURVIVOR_FORMS)
def test_survivor_cascade_prefix_passes_every_window(oracle, form):
    a = survivor_cascade(form, n_pass=2)
    c = cascade_to_product(a)
    assert c.info.n_stages == a.n_stages
    img = dot_frame(3, 240, 320, n_dots=20)
    for profile, fn in (("clod", oracle.detect), ("opencv", oracle.detect_opencvlike)):
        r, st = fn(a, img, cap=CAP)
        assert st["windows"] > 0
        assert st["stage_entered"][:3] == [st["windows"]] * 3, f"{profile}: the prefix rejected windows: {st['stage_entered']}"
        if form == "accept_all":
            assert len(r) == st["windows"], profile
        else:
            assert 0 < len(r) < st["windows"] // 20, f"{profile}: {len(r)} detections of {st['windows']} windows"


@pytest.mark.parametrize("form", [f for f in SURVIVOR_FORMS if f != "accept_all"])
def test_survivor_detections_follow_the_dots(oracle, form):
    """Without dots no window passes the selective stages; with them some do."""
    a = survivor_cascade(form)
    plain = dot_frame(4, 240, 320, n_dots=0)
    for fn in (oracle.detect, oracle.detect_opencvlike):
        assert len(fn(a, plain, cap=CAP)[0]) == 0
        r, _ = fn(a, dot_frame(4, 240, 320, n_dots=10), cap=CAP)
        assert len(r) > 0


def test_stage_tree_forms():
    """chain_tree is the as_stage_tree shape (two chains after the prefix), branch_tree a tree whose rejects inside one run
    of stages go to two different places."""
    ch, br = survivor_cascade("chain_tree"), survivor_cascade("branch_tree")
    assert list(ch.stage_parent) == [-1, 0, 1, 1, 2, 3] and list(ch.stage_next) == [-1, -1, 3, -1, -1, -1]
    assert list(br.stage_parent) == [-1, 0, 1, 2, 2, 1] and list(br.stage_next) == [-1, -1, 5, 4, -1, -1]
    assert list(br.stage_child) == [1, 2, 3, -1, -1, -1]
    lin = survivor_cascade("stumps")
    assert np.all(lin.stage_next == -1)
