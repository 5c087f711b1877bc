"""The part ranges of the grid pass's unit list (csrc/vj_grid_parts.hpp, shared by the kernel and the host) on the CPU, behind
tests/grid_parts_driver.cpp, a program of its own built with AddressSanitizer + UBSan where the toolchain has them: for every
total from 0 to 4100 the eight ranges are disjoint, ascending and cover [0, total)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def test_grid_part_ranges_cover_every_total(tmp_path):
    exe = str(tmp_path / "grid_parts")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _asan_runtime() else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", *san, "-I", CSRC, os.path.join(ROOT, "tests", "grid_parts_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "grid_parts_driver: OK" in r.stdout
