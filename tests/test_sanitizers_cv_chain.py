"""AddressSanitizer + UBSan run on the CPU of the device-free host code of vj_detect_opencv_chain's device hand-off
(csrc/vj_cv_roi_host.cpp: the route a call takes, the region -> out_first index remap with duplicate keys absent and present, empty
lists, out-of-range indices refused, the info record, the state block's errors) and of the unit builder's restatement the device
shares with the host (csrc/vj_cv_roi_units.hpp), checked for every region size 1..640 x every factor slot against
cv_roi_build_units, behind tests/cv_chain_asan_driver.cpp.  A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_cv_chain_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "cv_chain_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "cv_chain_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_cv_roi_host.cpp", "vj_cascade.cpp", "vj_group.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cv_chain_asan_driver: OK" in r.stdout
