"""The queues of the gather chain's linear kernels (csrc/vj_gather_queue.hpp, shared by the kernel and the host) on the CPU: the
capacity a wave gets out of the workgroup's 2048 entries for 1 ... 8 waves, the clamp of the stump-parallel tail whose scratch lives
in that queue, and the first-pass units the plan cuts to that capacity — behind tests/gather_queue_driver.cpp, a program of its own
built with AddressSanitizer + UBSan where the toolchain has them.  The units are checked on the grids of frontalface_alt's plans for
320 x 240 and 640 x 480 (Cascade.plan_tiles gives every scale's grid and the rows the tiles keep): every unit <= cap windows, the
units of a scale disjoint and covering its rows, for every wave count and a set of block widths.

The tail's scratch is T entries + T x 9 verdict words = 80 T bytes of a queue of 8 cap bytes.  The clamp moves in steps of 8 and
never beyond the 48 the tunable has always had (48 at 512 entries, 32 at 384 and 320, 24 at 256): it fits at the clamp and does
not fit one step above it; at 320 entries, where the fit is exact, it does not fit at clamp + 1 either.  (At 512 and 256 entries
clamp + 1 would still fit — 49 x 80 = 3920 <= 4096, 25 x 80 = 2000 <= 2048 — the clamps there are the ones the design lists.)"""
import os
import subprocess

import pytest

from clfacedetection_amd import Cascade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clfacedetection_amd", "csrc")
LDS_ENTRIES = 2048
CAPS = {1: 512, 2: 512, 3: 512, 4: 512, 5: 384, 6: 320, 7: 256, 8: 256}     # 64 * floor(2048 / (64 w)), at most 512
TAILS = {512: 48, 384: 32, 320: 32, 256: 24}
SIZES = [(320, 240), (640, 480)]
_RUN = {}


def _asan_runtime():
    p = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


def plan_grids(W, H, n_frames):
    """(nx, ny, first gather row) of every scale of the shipped plan, and the plan's own count of first-pass units."""
    info, tiles = Cascade.load("frontalface_alt").plan_tiles(W, H, n_frames, tile_split=-1.0)
    return [(t.nx, t.ny, t.tile_row_end if t.lds_class >= 0 else 0) for t in tiles], info.cut.gather_units


def run_driver(tmp_path_factory, W, H, n_frames):
    key = (W, H, n_frames)
    if key not in _RUN:
        d = tmp_path_factory.mktemp("gather_queue")
        exe = str(d / "gather_queue")
        if "exe" not in _RUN:
            san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if _asan_runtime() else []
            cmd = ["g++", "-std=c++17", "-O1", "-g", *san, "-I", CSRC, os.path.join(ROOT, "tests", "gather_queue_driver.cpp"), "-o", exe]
            r = subprocess.run(cmd, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-4000:]
            _RUN["exe"] = exe
        grids, plan_units = plan_grids(W, H, n_frames)
        path = str(d / "grids.txt")
        with open(path, "w") as f:
            f.write("".join(f"{nx} {ny} {row0}\n" for nx, ny, row0 in grids))
        r = subprocess.run([_RUN["exe"], path], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert f"gather_queue_driver: OK ({len(grids)} grids)" in r.stdout
        rows = [ln.split() for ln in r.stdout.splitlines()]
        _RUN[key] = ({int(x[1]): (int(x[2]), int(x[3])) for x in rows if x[0] == "cap"},
                     {int(x[1]): int(x[2]) for x in rows if x[0] == "units"}, grids, plan_units)
    return _RUN[key]


def test_capacity_and_tail_clamp_for_one_to_eight_waves(tmp_path_factory):
    caps, _, _, _ = run_driver(tmp_path_factory, 320, 240, 1)
    assert sorted(caps) == list(range(1, 9))
    for w in range(1, 9):
        cap, tail = caps[w]
        assert cap == CAPS[w] and cap % 64 == 0 and w * cap <= LDS_ENTRIES, (w, cap)
        assert tail == TAILS[cap], (w, cap, tail)
        assert 80 * tail <= 8 * cap, (w, cap, tail)              # T entries + T x 9 verdict words fit the queue at the clamp
        assert tail == 48 or 80 * (tail + 8) > 8 * cap, (w, cap, tail)   # ... and not one step above it (48: the tunable's own limit)
    assert 80 * (TAILS[320] + 1) > 8 * 320                       # the exact fit


@pytest.mark.parametrize("n_frames", [1, 9])
@pytest.mark.parametrize("W,H", SIZES)
def test_first_pass_units_partition_every_scale(tmp_path_factory, W, H, n_frames):
    """The driver walks the units of every grid as the grid pass does, for 1 ... 8 waves (4, 6 and 8 among them), block widths 0
    (row runs), 1, 16, 32, 48, 64, 300 and 512, from row 0 (every scale a gather scale) and from the plan's own cut; it fails on a unit
    above cap, a window in two units or in none.  The plan's own unit count is the driver's at the shipped wave count."""
    _, units, grids, plan_units = run_driver(tmp_path_factory, W, H, n_frames)
    # (the plans have tile scales, whose rows the tiles keep, and gather scales; all but the single 320 x 240 frame's have gather
    # grids of more than 512 windows, which shorter queues cut into more units)
    assert len(grids) >= 8 and any(row0 >= ny for _, ny, row0 in grids) and any(row0 == 0 for _, _, row0 in grids), grids
    assert sorted(units) == list(range(1, 9))
    assert units[1] == units[2] == units[3] == units[4] <= units[5] <= units[6] <= units[7] == units[8], units
    if any(nx * (ny - row0) > 512 for nx, ny, row0 in grids if row0 < ny):
        assert units[8] > units[4], units
    else:
        assert (W, H, n_frames) == (320, 240, 1), grids
    shipped_waves = 8 if n_frames >= 8 else 3
    assert plan_units == units[shipped_waves], (plan_units, units)
