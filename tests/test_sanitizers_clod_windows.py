"""AddressSanitizer + UBSan run on the CPU of the host code vj_run_windows adds (csrc/vj_points_host.cpp: argument checks, what a
scale gives, the scatter of the verdicts) and of the grouping it reuses (csrc/vj_cv_points_host.cpp) behind
tests/clod_windows_asan_driver.cpp, a program of its own, fed degenerate lists: empty and null, one window, 2^20 windows of one
scale, every window its own scale, extreme coordinates, indices out of range, every flag bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_clod_windows_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "clod_windows_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "clod_windows_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_points_host.cpp", "vj_cv_points_host.cpp", "vj_cv_roi_host.cpp", "vj_group.cpp",
                                           "vj_cascade.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "clod_windows_asan_driver: OK" in r.stdout
