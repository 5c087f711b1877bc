"""AddressSanitizer + UBSan run on the CPU of the host planner of vj_yuv_to_bgr / vj_bgr_to_yuv (csrc/vj_yuv_host.cpp: the argument
checks, the layouts, the frame records of a slice) behind tests/yuv_asan_driver.cpp, a stand-alone program: all layouts, both channel
counts, widths 2 .. 10 and 254 .. 258, heights 2, 4, 6, whole and in slices — the work units, decoded as the kernels decode them,
cover every output byte and pad byte once and read only inside the sources — and the error cases.  Nothing is loaded into Python
under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_yuv_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "yuv_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "yuv_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_yuv_host.cpp", "vj_cascade.cpp", "vj_group.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "yuv_asan_driver: OK" in r.stdout
