"""By-hand measurement of vj_track (run on the GPU box; not collected by pytest):
    python tests/measure_track.py [out.json]
Workload: 64 device-resident 1920 x 1080 BGR frames of random bytes, 8 rows per frame of 200-pixel boxes (row k of frame f looks
for its box in frame f + 1; the last frame's rows point back), t, r = (32, 8) and (64, 16).  A time is the device time of one call
by the library's events (vj_track_timing: around its copies and launches, and around the match launch alone), the median of nine
calls after two warm-ups, and every side runs twice (the A/A pair: the spread between its two medians is what a difference has to
exceed).  The match does n * (2 r + 1)^2 * t^2 absolute differences; the peak they are set against is the plain vector-ALU issue
rate of the micro-architecture guide — 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz — times the 16 differences one
v_qsad_pk_u16_u8 does per lane: 1.26e15 per second.  Whether that instruction issues at the plain rate is not in the guide, so the
fraction is a lower bound of the kernel's distance from what the hardware can do.  The yardstick from before this stage, in the
same run: extract() of the same 512 boxes to 64 x 64 gray (vj_extract_timing), the part of the work that existed already."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

from measure_equalize import H_HD, N_HD, W_HD, write  # noqa: E402
from measure_mixed import REPEATS, WARMUP  # noqa: E402

ROWS_PER_FRAME, BOX = 8, 200
SAD_PEAK = 256 * 4 * 32 * 2.4e9 * 16


def main(out_path):
    import numpy as np
    import torch
    from clfacedetection_amd import DeviceFrames, Environment
    env = Environment(0)
    result = {"device": env.device_name, "repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD], "rows": N_HD * ROWS_PER_FRAME,
              "box": BOX, "sad_peak_per_s": SAD_PEAK, "cases": {}}
    med = lambda xs: round(statistics.median(xs), 4)
    gen = torch.Generator(device="cuda").manual_seed(1)
    bgr = torch.randint(0, 256, (N_HD, H_HD, W_HD, 3), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    frames = DeviceFrames.from_torch(bgr)
    rng = np.random.default_rng(2)
    rows, rects = [], []
    for f in range(N_HD):
        for _ in range(ROWS_PER_FRAME):
            x, y = int(rng.integers(0, W_HD - BOX)), int(rng.integers(0, H_HD - BOX))
            rows.append((f, f + 1 if f + 1 < N_HD else f - 1, x, y, BOX, BOX))
            rects.append((f, x, y, BOX, BOX))

    def measure(name, call, timing, extra):
        pairs, shares = [], []
        for _ in range(2):                                  # the A/A pair
            t, m = [], []
            for k in range(WARMUP + REPEATS):
                call()
                if k >= WARMUP:
                    v = timing()
                    t.append(v[0] if isinstance(v, tuple) else v)
                    m.append(v[1] if isinstance(v, tuple) else 0.0)
            pairs.append(med(t))
            shares.append(med(m))
        c = {"ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4)}
        c.update(extra(statistics.mean(pairs), statistics.mean(shares), shares))
        result["cases"][name] = c
        print(name, json.dumps(c), flush=True)

    out = torch.empty(len(rects) * 64 * 64, dtype=torch.uint8, device="cuda")
    measure("extract_512_boxes_to_64x64_gray", lambda: env.extract(frames, rects, (64, 64), gray=True, out=out), env.extract_timing,
            lambda ms, _m, _s: {})
    for t, r in ((32, 8), (64, 16)):
        diffs = len(rows) * (2 * r + 1) ** 2 * t * t
        measure(f"track_t{t}_r{r}", lambda: env.track(frames, rows, tmpl=t, radius=r), env.track_timing,
                lambda ms, match, shares: {"match_ms": shares, "match_share": round(match / ms, 4), "abs_differences": diffs,
                                           "abs_differences_per_s": round(diffs / (match * 1e-3), 1),
                                           "fraction_of_sad_peak": round(diffs / (match * 1e-3) / SAD_PEAK, 5),
                                           "everything_but_the_match_ms": round(ms - match, 4)})
    base = statistics.mean(result["cases"]["extract_512_boxes_to_64x64_gray"]["ms"])
    for name, c in result["cases"].items():
        c["over_the_extract_yardstick"] = round(statistics.mean(c["ms"]) / base, 3)
    env.close()
    print(json.dumps(result))
    write("stage", result, out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "track.json"))
