"""CV_HAAR_DO_CANNY_PRUNING timing: 64 x 1080p frontalface_alt through vj_detect_opencv, flags 0 against the pruning flag, on
xorshift noise and on flat-with-patches content (tests/canny_oracle.py).  Per setting the median over --steps calls of
integral_ms (with the flag: + Canny and the edge integral), cascade_ms and the wall time of a call; then windows and
stage_entered[0] of one counted call.  Writes profiles/r07_canny.log (or --out).
    python tools/cv_canny_time.py [--frames 64] [--steps 7] [--out profiles/r07_canny.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import canny_oracle as co  # noqa: E402
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_CANNY_PRUNING, Cascade, Environment  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_canny.log"))
    args = ap.parse_args()
    env = Environment(0)
    c = Cascade.load("frontalface_alt")
    o = Oracle()
    contents = {
        "xorshift": np.stack([o.xorshift_noise(1000 + i, 1080, 1920) for i in range(args.frames)]),
        "patches": np.stack([co.patches_frame(1000 + i, 1080, 1920) for i in range(args.frames)]),
    }
    lines = [f"# {env.device_name}: {args.frames} x 1920x1080 frontalface_alt, vj_detect_opencv, median of {args.steps} calls (ms)",
             "content   flag     integral  canny+edge  cascade   wall      windows      stage_entered[0]"]
    for name, frames in contents.items():
        base_int = None
        for flag, label in ((0, "0"), (VJ_FLAG_CV_CANNY_PRUNING, "canny")):
            env.detect_opencv(c, frames, flags=flag)   # warm-up: plan, buffers
            ti, tc, tw = [], [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                r = env.detect_opencv(c, frames, flags=flag)
                tw.append((time.perf_counter() - t0) * 1e3)
                ti.append(r.integral_ms)
                tc.append(r.cascade_ms)
            k = env.detect_opencv(c, frames, flags=flag | VJ_FLAG_COUNTERS)
            mi = statistics.median(ti)
            if base_int is None:
                base_int = mi
            lines.append(f"{name:9s} {label:8s} {mi:8.3f}  {mi - base_int:9.3f}  {statistics.median(tc):8.3f}  "
                         f"{statistics.median(tw):8.2f}  {k.windows:11d}  {k.stage_entered[0]:11d}")
            print(lines[-1], flush=True)
    env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
