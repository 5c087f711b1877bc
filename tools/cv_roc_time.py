"""What reject levels cost: N x 1080p (crude faces on a textured background, tests/scale_image_oracle.faces_frame) through
vj_detect_opencv_roc against the plain vj_detect_opencv call with VJ_FLAG_CV_SCALE_IMAGE on the same frames, frontalface_alt and
frontalface_alt_tree.  Both calls are warmed up, then alternate; per call the median (min .. max) over --steps of cascade_ms and of
the wall time, the rectangles of each, and the ratio of the medians.  Writes profiles/cv_roc_time.log (or --out).
    python tools/cv_roc_time.py [--frames 16] [--steps 9] [--out profiles/cv_roc_time.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import scale_image_oracle as so  # noqa: E402
from clfacedetection_amd import VJ_FLAG_CV_SCALE_IMAGE, Cascade, Environment  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cv_roc_time.log"))
    args = ap.parse_args()
    env = Environment(0)
    frames = np.stack([so.faces_frame(1000 + i, 1080, 1920, n_faces=8) for i in range(args.frames)])
    lines = [f"# {env.device_name}: {args.frames} x 1920x1080, VJ_FLAG_CV_SCALE_IMAGE, plain and ROC calls alternating, "
             f"median (min .. max) of {args.steps} calls (ms)",
             "cascade               call   cascade_ms                  wall_ms                     rectangles"]
    for name in ("frontalface_alt", "frontalface_alt_tree"):
        c = Cascade.load(name)
        calls = {"plain": lambda: env.detect_opencv(c, frames, flags=VJ_FLAG_CV_SCALE_IMAGE),
                 "roc": lambda: env.detect_opencv_roc(c, frames)}
        t = {k: ([], []) for k in calls}
        n = {}
        for _ in range(2):                      # warm-up of both: plans, buffers (the ROC call's grown detection buffer)
            for k, call in calls.items():
                call()
        for _ in range(args.steps):
            for k, call in calls.items():
                t0 = time.perf_counter()
                r = call()
                t[k][1].append((time.perf_counter() - t0) * 1e3)
                t[k][0].append(r.cascade_ms)
                n[k] = len(r.rects)
        for k in calls:
            tc, tw = t[k]
            lines.append(f"{name:21s} {k:6s} {statistics.median(tc):8.3f} ({min(tc):8.3f} .. {max(tc):8.3f})  "
                         f"{statistics.median(tw):8.2f} ({min(tw):8.2f} .. {max(tw):8.2f})  {n[k]:9d}")
            print(lines[-1], flush=True)
        lines.append(f"{name:21s} roc / plain: cascade {statistics.median(t['roc'][0]) / statistics.median(t['plain'][0]):.3f}, "
                     f"wall {statistics.median(t['roc'][1]) / statistics.median(t['plain'][1]):.3f}")
        print(lines[-1], flush=True)
    env.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
