"""AddressSanitizer + UBSan run on the CPU of the byte-moving half of the frame-processing calls (csrc/vj_stage_host.hpp, DESIGN.md
§4.24) behind tests/stage_asan_driver.cpp, a stand-alone program: the block layout against the formulas the drivers used to spell
out, packed and rounded to 16; gather_rows from sources at every address mod 4 whose heap blocks end with their last row, into
destinations whose pad bytes keep a canary; the write-back of painted spans into canary-filled strided destinations of exact size
— only [x0, x0 + span) x [y0, y1) changes —; and the touched rows of frames of one plane and of three against a brute-force
min / max, through a round trip that writes the union of overlapping records and nothing else.  Nothing is loaded into Python under
a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_stage_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "stage_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "stage_asan_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "stage_asan_driver: OK" in r.stdout
