"""By-hand measurement of vj_extract_affine (run on the GPU box; not collected by pytest):
    python tests/measure_extract_affine.py [out.json]
Workload: tests/measure_extract.py's — 64 device-resident frames of 1920 x 1080, 16 regions of about 300 x 300 on each (280 .. 320 on a
side, some across the frame's border), to 112 x 112 — cut three ways per case: by vj_extract's bilinear call (the yardstick: it is
in the parent commit and does comparable loads per output byte), by vj_extract_affine with affine_from_rect of the same boxes, and
by vj_extract_affine with those matrices turned by 15 degrees about the box's centre.  Cases: BGR interleaved, BGR to gray, gray.
A time is the device time of one call by the library's events (vj_extract_timing / vj_extract_affine_timing), the median of nine
after two warm-ups; every side runs twice (the A/A pair), the sides alternating.  Bytes a call must move: the distinct source pixels
the boxes cover, once, plus the output, once (a turned box covers the same area); against the 8 TB/s HBM peak.  No gate."""
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

from measure_equalize import H_HD, N_HD, W_HD, hd_batch, write  # noqa: E402
from measure_extract import PER_FRAME, SIZE, must_move, regions  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP  # noqa: E402


def matrices(rects, deg):
    """(n, 7) rows: affine_from_rect of every box, turned by `deg` about the box's centre (the output's centre stays on it)."""
    from clfacedetection_amd import affine_from_rect
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    ox, oy = (SIZE[0] - 1) / 2, (SIZE[1] - 1) / 2
    rows = []
    for f, x, y, w, h in rects:
        m = affine_from_rect(x, y, w, h, SIZE)
        cx, cy = m[0] * ox + m[2], m[4] * oy + m[5]                      # where the output's centre lands
        a, b, d, e = m[0] * c, -m[0] * s, m[4] * s, m[4] * c              # the box's scaling after the turn
        rows.append([f, a, b, cx - a * ox - b * oy, d, e, cy - d * ox - e * oy])
    return np.array(rows, np.float64)


def main(out_path):
    import torch
    from clfacedetection_amd import Environment
    env = Environment(0)
    rects = regions()
    sides = {"extract": None, "affine_rect": matrices(rects, 0.0), "affine_rot15": matrices(rects, 15.0)}
    assert np.array_equal(sides["affine_rect"][:, [2, 4]], np.zeros((len(rects), 2)))
    result = {"device": env.device_name, "repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD], "regions_per_frame": PER_FRAME,
              "to": list(SIZE), "hbm_peak_gb_s": HBM_PEAK_GBS, "cases": {}}
    med = lambda xs: round(statistics.median(xs), 4)
    for name, ch, kw in (("bgr_interleaved", 3, {}), ("bgr_to_gray", 3, {"gray": True}), ("gray", 1, {})):
        d, keep = hd_batch("noise", ch)
        _, c, nbytes = env.extract_layout(d, rects, SIZE, **kw)
        assert env.extract_affine_layout(d, sides["affine_rect"], SIZE, **kw) == (c, nbytes)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        moved = must_move(rects, ch, nbytes)
        times = {s: [] for s in sides}
        for _ in range(2):                                              # the A/A pair, the sides alternating
            for s, rows in sides.items():
                t = []
                for k in range(WARMUP + REPEATS):
                    if rows is None:
                        env.extract(d, rects, SIZE, out=buf, **kw)
                        ms = env.extract_timing()
                    else:
                        env.extract_affine(d, rows, SIZE, out=buf, **kw)
                        ms = env.extract_affine_timing()
                    if k >= WARMUP:
                        t.append(ms)
                times[s].append(med(t))
        base = statistics.mean(times["extract"])
        case = {"regions": len(rects), "bytes": moved}
        for s, pair in times.items():
            ms = statistics.mean(pair)
            case[s] = {"ms": pair, "aa_spread_ms": round(abs(pair[0] - pair[1]), 4), "over_extract": round(ms / base, 3),
                       "tb_per_s": round(moved / ms / 1e9, 3), "fraction_of_hbm_peak": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)}
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del d, keep, buf
    env.close()
    write("call", result, out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "extract_affine.json"))
