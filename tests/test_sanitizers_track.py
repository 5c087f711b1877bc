"""AddressSanitizer + UBSan run on the CPU of the host planner of vj_track (csrc/vj_track_host.cpp: the argument checks, the two
vj_extract layouts of a call, the scratch layout, the slices, the box of a match) and the planners it uses, behind
tests/track_asan_driver.cpp, a stand-alone program: rows inside, across and outside frames of 1, 3 and 4 channels, the ends of t and
r, whole and in slices — every patch inside a scratch block of exactly the layout's bytes, the match kernel's index arithmetic
walked over it — and the error cases.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_track_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "track_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "track_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_track_host.cpp", "vj_extract_host.cpp", "vj_prep_host.cpp", "vj_atlas_host.cpp",
                                           "vj_cv_roi_levels_host.cpp", "vj_cv_roi_host.cpp", "vj_cascade.cpp", "vj_group.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "track_asan_driver: OK" in r.stdout
