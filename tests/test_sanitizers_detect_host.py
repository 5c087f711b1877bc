"""AddressSanitizer + UBSan run on the CPU of the clod detect drivers' layouts and arithmetic (csrc/vj_detect_host.hpp) behind
tests/detect_host_asan_driver.cpp, a stand-alone program: the counters block's named ranges marked in a byte map, the grouped
hand-off buffer's layout against the formula restated, the detection offset's decode over a whole batch and at the 2^32 edge,
max_frames over a grid with zeros and the 32-bit edges, and the pass schedule against a literal restatement of enqueue_cascade's
decisions.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_detect_host_layouts_and_arithmetic_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "detect_host_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "detect_host_asan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "detect_host_asan_driver: OK" in r.stdout
