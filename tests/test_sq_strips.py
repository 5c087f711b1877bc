"""The strip rule of the u32 squared integral (csrc/vj_sq_strips.hpp, shared by the kernels and the host) on the CPU, behind
tests/sq_strips_driver.cpp, a program of its own built with AddressSanitizer + UBSan where the toolchain has them.

A window of w x h pixels, w <= 66 051, is cut into horizontal strips of floor(66 051 / w) rows.  For w x h over 1 ... 1100 at
coarse steps and the edges of the rule (257 x 257 = 66 049 px: one strip, 258 x 256 = 66 048 px, 258 x 258, 1 x 66 051,
1 x 66 052, w = 66 051) the driver prints the row boundaries at which the shared function reads its corners and checks the
function's own sums on all-255 and random {0, 255} images.  Here the boundaries must be disjoint, ascending strips that cover
the window and hold at most 66 051 pixels each, and — on images held as numpy uint64 integrals — the strips' sums from the
integral reduced mod 2^32 must add up to the true sum of squares."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")
SQ32_MAX_AREA = 66051
assert 255 * 255 * SQ32_MAX_AREA < 2**32 <= 255 * 255 * (SQ32_MAX_AREA + 1)

COARSE = [1, 2, 37, 61, 256, 257, 258, 300, 512, 777, 1080, 1100]
CASES = [(w, h) for w in COARSE for h in COARSE] + [
    (257, 257), (258, 256), (258, 258), (256, 258), (1, 66051), (1, 66052), (2, 66052), (66051, 1), (66051, 2), (66051, 5), (33026, 4)]


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.fixture(scope="module")
def strips(tmp_path_factory):
    """{(w, h): (rows per strip, [row boundaries])} as the shared function walks them."""
    exe = str(tmp_path_factory.mktemp("sq_strips") / "sq_strips")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _asan_runtime() else []
    cmd = ["g++", "-std=c++17", "-O1", "-g", *san, "-I", CSRC, os.path.join(ROOT, "tests", "sq_strips_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], input="".join(f"{w} {h}\n" for w, h in CASES), capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"sq_strips_driver: OK {len(CASES)}"
    out = {}
    for line in lines[:-1]:
        v = [int(t) for t in line.split()]
        assert len(v) == 4 + v[3] + 1, line
        out[(v[0], v[1])] = (v[2], v[4:])
    assert set(out) == set(CASES)
    return out


def test_strips_are_disjoint_ascending_and_cover_the_window(strips):
    for (w, h), (rows, b) in strips.items():
        assert rows == SQ32_MAX_AREA // w, (w, h)
        assert b[0] == 0 and b[-1] == h, (w, h, b)
        assert all(lo < hi for lo, hi in zip(b, b[1:])), (w, h, b)           # ascending, none empty; consecutive: disjoint, no gaps
        assert all((hi - lo) * w <= SQ32_MAX_AREA for lo, hi in zip(b, b[1:])), (w, h, b)
        assert len(b) - 1 == -(-h // rows), (w, h, b)                          # k = ceil(h / floor(66051 / w))
    assert len(strips[(257, 257)][1]) == 2 and len(strips[(258, 256)][1]) == 2      # one strip each
    assert strips[(258, 258)][1] == [0, 256, 258]
    assert strips[(1, 66051)][1] == [0, 66051] and strips[(1, 66052)][1] == [0, 66051, 66052]
    assert strips[(66051, 5)][1] == [0, 1, 2, 3, 4, 5]


def _integral_u64(img):
    q = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.uint64)
    np.cumsum(np.cumsum(img.astype(np.uint64) ** 2, axis=0), axis=1, out=q[1:, 1:])
    return q


@pytest.mark.parametrize("content", ["all255", "random"])
def test_strip_sums_from_the_reduced_integral_are_exact(strips, content):
    rng = np.random.default_rng(14)
    x0, y0 = 3, 2      # the window's origin inside its image (margins all round: no corner is a zero of the integral)
    wrapped = big = 0
    for (w, h), (_, b) in strips.items():
        shape = (h + y0 + 1, w + x0 + 2)
        img = np.full(shape, 255, np.uint8) if content == "all255" else (rng.integers(0, 2, shape, dtype=np.uint8) * np.uint8(255))
        q = _integral_u64(img)
        lo = (q & np.uint64(0xffffffff)).astype(np.uint32)
        want = int(q[y0 + h, x0 + w]) - int(q[y0 + h, x0]) - int(q[y0, x0 + w]) + int(q[y0, x0])
        got = 0
        for r0, r1 in zip(b, b[1:]):
            c = [int(lo[y0 + r1, x0 + w]), int(lo[y0 + r1, x0]), int(lo[y0 + r0, x0 + w]), int(lo[y0 + r0, x0])]
            got += (c[0] - c[1] - c[2] + c[3]) % 2**32
        assert got == want, (w, h, content)
        wrapped += int(q[-1, -1]) >= 2**32
        big += want >= 2**32
    # the cases reach what they are for: integrals that wrapped, and windows whose true sum needs more than 32 bits
    assert wrapped >= 20 and big >= 20, (wrapped, big)
