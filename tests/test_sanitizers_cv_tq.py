"""AddressSanitizer + UBSan run on the CPU of the tree queue's sizing (csrc/vj_cv_tq_host.hpp: cv_tq_sizing) behind
tests/cv_tq_asan_driver.cpp, a stand-alone program: against brute force over shifts 0..4, 1..64 tile scales of random grids, 1..200
frames and window counts that put the queue next to CV_TQ_MAX — a queue holds every scale's sub-queue (cv_tq_first / cv_tq_cap of
csrc/vj_device.hpp) without overlap, a resplit names the largest frame count that fits, and the rows take the call exactly when not
even one frame fits.  The boundary is otherwise reached only by a 96 x 1080p GPU run.  Nothing is loaded into Python under a
sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_cv_tq_sizing_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cv_tq_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cv_tq_asan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cv_tq_asan_driver: OK" in r.stdout
