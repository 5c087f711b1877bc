"""AddressSanitizer + UBSan run on the CPU of the host planner of vj_extract_yuv / vj_extract_affine_yuv
(csrc/vj_extract_yuv_host.cpp: the argument checks through the planners of vj_yuv_to_bgr, vj_extract and vj_extract_affine, the region
records with their planes, the taps and the work units of a slice) behind tests/extract_yuv_asan_driver.cpp, a stand-alone program:
all layouts, planes and the destination at every address mod 4, regions and affines inside, across and outside their frames, every
flag combination, whole calls and slices of 1, 2 and 3 frames — every output byte covered once, every tap inside its run, every
clamped Y and chroma index inside its plane, a 2-byte load only at an even address — and the error cases.  Nothing is loaded into
Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_extract_yuv_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "extract_yuv_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "extract_yuv_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_extract_yuv_host.cpp", "vj_extract_host.cpp", "vj_affine_host.cpp", "vj_yuv_host.cpp", "vj_prep_host.cpp",
                                           "vj_atlas_host.cpp", "vj_cv_roi_levels_host.cpp", "vj_cv_roi_host.cpp", "vj_cascade.cpp", "vj_group.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "extract_yuv_asan_driver: OK" in r.stdout
