"""AddressSanitizer + UBSan run on the CPU of the host planner of vj_paint_yuv (csrc/vj_paint_yuv_host.cpp on top of vj_paint's and
vj_yuv_to_bgr's planners) behind tests/paint_yuv_asan_driver.cpp, a stand-alone program: NV12, NV21 and I420 frames with planes at
every address mod 4, regions inside, across and outside them, every mode with and without the ellipse, whole and in slices of 1, 2
and 3 frames — the units, decoded as the kernels decode them, cover every byte of every K and Kc row and every scratch element
exactly once, the scratch ranges are disjoint and inside the reported bytes, the chroma overlap lists equal a brute-force search
over Kc, the rectangles' row sets equal the painted-set test, the slices hold whole frames — and the error cases.  Nothing is loaded
into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_paint_yuv_planner_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "paint_yuv_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "paint_yuv_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_paint_yuv_host.cpp", "vj_paint_host.cpp", "vj_yuv_host.cpp", "vj_extract_host.cpp", "vj_prep_host.cpp",
                                           "vj_atlas_host.cpp", "vj_cv_roi_levels_host.cpp", "vj_cv_roi_host.cpp", "vj_cascade.cpp", "vj_group.cpp")] + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "paint_yuv_asan_driver: OK" in r.stdout
