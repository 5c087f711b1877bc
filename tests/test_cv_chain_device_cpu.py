"""vj_detect_opencv_chain's device hand-off without a GPU: the flag and the getter exist in the header and in the Python mirror
with the same value and layout, and the premises of the cases tests/test_gpu_cv_chain_device.py adds (tests/cv_chain_device_cases.py)
hold on the oracle alone."""
import ctypes as C
import os
import re

import numpy as np

import cv_chain_device_cases as dc
import cv_rois_cases as cc
from clfacedetection_amd.api import DATA_DIR
from oracle.oracle import load_vjc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(name):
    return load_vjc(os.path.join(DATA_DIR, f"haarcascade_{name}.vjc"))


def _header():
    return open(os.path.join(ROOT, "include", "vj.h")).read()


def test_the_flag_in_the_header_and_the_python_mirror():
    import clfacedetection_amd as pkg
    from clfacedetection_amd import api
    bits = dict(re.findall(r"(VJ_FLAG_[A-Z0-9_]+)\s*=\s*1u << (\d+)", _header()))
    assert bits["VJ_FLAG_CV_CHAIN_DEVICE"] == "10"
    assert pkg.VJ_FLAG_CV_CHAIN_DEVICE == api.VJ_FLAG_CV_CHAIN_DEVICE == 1 << 10
    assert [n for n, b in bits.items() if b == "10"] == ["VJ_FLAG_CV_CHAIN_DEVICE"]      # no other flag shares the bit


def test_the_getter_in_the_header_and_the_signatures():
    from clfacedetection_amd.api import CvChainInfo, Environment, _SIGNATURES
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int\s+vj_cv_chain_info_get\s*\(\s*const vj_env\*\s*e,\s*vj_cv_chain_info\*\s*out\s*\)", text)
    restype, argtypes = _SIGNATURES["vj_cv_chain_info_get"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(CvChainInfo)]
    assert callable(Environment.cv_chain_info)
    # the struct of the header, member for member
    body = re.search(r"typedef struct vj_cv_chain_info \{(.*?)\} vj_cv_chain_info;", text, re.S).group(1)
    members = re.findall(r"(int32_t|uint64_t|float)\s+(\w+);", body)
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in members] == list(CvChainInfo._fields_)
    assert {"handoff", "sub_batches", "sub_batches_device", "reruns", "regions", "units", "windows", "handoff_ms"} <= {n for _, n in members}
    assert C.sizeof(CvChainInfo) == 48 and CvChainInfo.units.size == 8 and CvChainInfo.windows.size == 8


def test_the_library_answers_null_arguments(lib):
    from clfacedetection_amd.api import CvChainInfo
    info = CvChainInfo()
    assert lib.vj_cv_chain_info_get(None, C.byref(info)) == 1                              # VJ_ERR_ARG
    assert lib.vj_cv_chain_info_get(None, None) == 1


def test_stage_tree_case(oracle):
    first, second, seeds, mn = dc.TREE_CASE
    a2 = _arrays(second)
    assert any(int(v) != -1 for v in a2.stage_next)                                        # a stage tree
    regions, res = cc.oracle_chain(oracle, _arrays(first), a2, dc.tree_frames(), mn)
    assert len(regions) == 9 and sum(len(r) for r, _ in res) == 15
    assert sum(int(st["stage_entered"][a2.n_stages - 1]) for _, st in res) >= 1            # the last stage is entered


def test_frames_that_give_nothing(oracle):
    a1 = _arrays(dc.NOTHING_CASE[0])
    raw, _ = oracle.detect_opencvlike(a1, dc.constant_frame())
    assert len(raw) == 0
    raw, _ = oracle.detect_opencvlike(a1, dc.smooth_frame())
    assert len(raw) == 1
    frames = dc.nothing_frames()
    regions, res = cc.oracle_chain(oracle, a1, _arrays(dc.NOTHING_CASE[1]), frames, 3)
    assert sorted(set(regions[:, 0].tolist())) == [0, 3] and sum(len(r) for r, _ in res) >= 10    # frames 1 and 2: no group
    regions, _ = cc.oracle_chain(oracle, a1, _arrays(dc.NOTHING_CASE[1]), frames[1:3], 0)
    assert regions[:, 0].tolist() == [1]                                                    # raw: the smooth frame's one candidate


def test_raw_candidate_counts_of_the_group_max_case(oracle):
    a1 = _arrays("frontalface_alt2")
    for seed, n in dc.RAW_COUNTS.items():
        raw, _ = oracle.detect_opencvlike(a1, dc.faces(seed))
        assert len(raw) == n, seed
    counts = [dc.RAW_COUNTS[s] for s in dc.GROUP_MAX_SEEDS]
    assert [c <= 100 for c in counts] == [True, False, False] and min(counts) > 96
