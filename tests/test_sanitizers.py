"""AddressSanitizer + UBSan runs on the CPU (GPU sanitizers are not available on the pool):
  * the library's HOST sources (cascade parser / loader, planning, sharding, grouping) behind tests/host_asan_driver.cpp,
    fed truncated and corrupted .vjc files, mutated XML, garbage arrays and degenerate rectangle lists;
  * the oracle (libvjoracle_asan.so, the Makefile target) on small detections of every mode."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_host_sources_under_asan_ubsan_legal_windows(tmp_path):
    """The driver's embedded XML cascade keeps every rectangle inside the window, and a copy with one tilted rectangle
    outside it is refused."""
    exe = str(tmp_path / "host_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
           "-DVJ_BUILDING", os.path.join(ROOT, "tests", "host_asan_driver.cpp")] + \
          [os.path.join(CSRC, f) for f in ("vj_cascade.cpp", "vj_plan.cpp", "vj_clod_plan.cpp", "vj_group.cpp", "vj_cv_plan.cpp", "vj_cv_roi_host.cpp",
                                          "vj_cv_roi_levels_host.cpp")] + ["-o", exe]
    subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe, os.path.join(ROOT, "clfacedetection_amd", "data"), str(tmp_path)], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "host_asan_driver: OK" in r.stdout


_ORACLE_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from oracle.oracle import Oracle, load_vjc
from clfacedetection_amd import synth
o = Oracle(sys.argv[2])
d = sys.argv[1] + "/clfacedetection_amd/data/haarcascade_%s.vjc"
img = synth.frame("blocks", 3, 97, 131)
a = load_vjc(d % "frontalface_alt")
for mode in (0, 1, 2, 3):
    o.detect(a, img, mode=mode)
o.detect(a, img, signed_mean=True, min_size=(24, 24), max_size=(60, 60))
o.detect(load_vjc(d % "frontalface_alt_tree"), img)
o.detect(load_vjc(d % "frontalface_alt2"), img)
for name in ("frontalface_alt", "frontalface_alt_tree", "frontalface_alt2", "fullbody", "eye_tree_eyeglasses"):
    o.detect_opencvlike(load_vjc(d % name), img)
o.integral(img); o.integral_tilted(img); o.integral_tilted(np.zeros((1, 1), np.uint8))
o.bgr2gray(np.zeros((5, 7, 3), np.uint8))
o.group_rectangles(np.array([[1, 2, 20, 20], [2, 2, 20, 20], [3, 3, 21, 21], [100, 100, 30, 30]]), 1)
print("oracle asan: OK")
'''


@pytest.mark.skipif(_asan_runtime() is None, reason="no libasan in this toolchain")
def test_oracle_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "libvjoracle_asan.so"], check=True, capture_output=True)
    env = dict(os.environ, LD_PRELOAD=_asan_runtime(), ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([sys.executable, "-c", _ORACLE_SCRIPT, ROOT, os.path.join(ROOT, "oracle", "libvjoracle_asan.so")],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "oracle asan: OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
