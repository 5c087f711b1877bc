"""The premises of tests/test_gpu_stream_order.py, on the oracles and restatements alone: a call that read its memory before the
pending work had written it returns A's result, one that read it afterwards B's (tests/stream_order_cases.py) — so the two must
differ for every reference the GPU file compares with, and the detector must find something in both."""
import numpy as np

import extract_cases as ec
import mixed_cases as mc
import prep_cases as pc
import stream_order_cases as sc

A, B = sc.A, sc.B


def test_the_frames_differ(oracle):
    assert not np.array_equal(sc.prepared(oracle, A), sc.prepared(oracle, B))
    assert not np.array_equal(pc.e2e_frames()[A], pc.e2e_frames()[B])
    assert not np.array_equal(ec.e2e_bgr()[A], ec.e2e_bgr()[B])
    assert sc.prepared(oracle, A).shape == (pc.E2E_SIZE[1], pc.E2E_SIZE[0])


def test_raw_lists_differ_in_both_profiles(oracle, cascades):
    c, a = cascades(pc.CASC)
    for profile in ("clod", "cv"):
        lists = [mc.rows(r) for r, _ in sc.detect_lists(oracle, a, profile)]
        print(profile, [len(x) for x in lists])
        assert [len(x) for x in lists] == [69, 69, 40]
        assert lists[0] != lists[1] and lists[0] != lists[2] and lists[1] != lists[2]


def test_restated_preprocess_outputs_differ(oracle):
    want = [pc.restate(oracle, pc.e2e_frames()[k], **sc.PREP_KW) for k in (A, B)]
    assert np.array_equal(want[A], sc.prepared(oracle, A)) and np.array_equal(want[B], sc.prepared(oracle, B))
    assert want[A].shape == want[B].shape and not np.array_equal(want[A], want[B])


def test_restated_extract_outputs_differ(oracle):
    a, b = sc.extracted(oracle, A), sc.extracted(oracle, B)
    assert a.shape == b.shape == (len(sc.EXTRACT_RECTS), sc.EXTRACT_SIZE[1], sc.EXTRACT_SIZE[0], 3)
    assert all(not np.array_equal(a[k], b[k]) for k in range(len(a)))          # every region, not only some


def test_window_list_verdicts_differ(oracle, cascades):
    c, a = cascades(pc.CASC)
    ra, sa = sc.cv_verdicts(oracle, a, A)
    rb, sb = sc.cv_verdicts(oracle, a, B)
    assert len(ra) == len(rb) == sc.N_WINDOWS and not np.array_equal(ra, rb) and not np.array_equal(sa, sb)
    ra, sa, va = sc.clod_verdicts(oracle, a, A)
    rb, sb, vb = sc.clod_verdicts(oracle, a, B)
    assert len(ra) == len(rb) == sc.N_WINDOWS and not np.array_equal(ra, rb) and not np.array_equal(va, vb)


def test_restated_canny_equalize_and_resize_differ(oracle):
    for f in (sc.canny, sc.equalized, sc.resized):
        assert f(oracle, A).shape == f(oracle, B).shape and not np.array_equal(f(oracle, A), f(oracle, B)), f.__name__
    assert sc.resized(oracle, A).shape == sc.RESIZE_TO[::-1]
