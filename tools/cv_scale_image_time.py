"""CV_HAAR_SCALE_IMAGE timing: 64 x 1080p frontalface_alt through vj_detect_opencv with VJ_FLAG_CV_SCALE_IMAGE and, in the same run,
without it (the scale-cascade profile: the yardstick), on xorshift noise and on frames with crude faces.  Per setting the median
over --steps calls of integral_ms (with the flag: the pyramid launch + the integrals of the canvas), cascade_ms and the wall time of
a call; then windows per frame and stage_entered[0] of one counted call, and the cascade time per million windows evaluated.
Writes profiles/r09_scale_image.log (or --out).  The kernel-stats summary next to it (profiles/r09_scale_image_kernel_stats.csv) is
rocprofv3 --kernel-trace --stats of this tool with --only scale_image --steps 3, a run of its own.
    python tools/cv_scale_image_time.py [--frames 64] [--steps 7] [--only scale_image] [--out profiles/r09_scale_image.log]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_SCALE_IMAGE, Cascade, Environment, synth  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def faces_frame(seed: int, h: int, w: int, n_faces: int) -> np.ndarray:
    """Crude faces of several sizes on a smooth background: hits on several levels of the pyramid."""
    rng = np.random.default_rng(seed)
    f = synth.frame("smooth", seed, h, w).copy()
    for _ in range(n_faces):
        s = int(rng.integers(max(24, min(h, w) // 8), max(25, min(h, w) // 2)))
        y, x = int(rng.integers(0, h - s + 1)), int(rng.integers(0, w - s + 1))
        f[y:y + s, x:x + s] = synth.crude_face(s)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_scale_image.log"))
    ap.add_argument("--only", default="", help="time this setting alone: 0 or scale_image (kernel traces)")
    args = ap.parse_args()
    env = Environment(0)
    c = Cascade.load("frontalface_alt")
    o = Oracle()
    contents = {
        "xorshift": np.stack([o.xorshift_noise(1000 + i, 1080, 1920) for i in range(args.frames)]),
        "faces": np.stack([faces_frame(1000 + i, 1080, 1920, 8) for i in range(args.frames)]),
    }
    lines = [f"# {env.device_name.strip() or 'gfx950'}: {args.frames} x 1920x1080 frontalface_alt, vj_detect_opencv, median of {args.steps} calls (ms)",
             "content   flag         pyr+integral  cascade    wall      windows/frame  stage_entered[0]/frame  cascade us/Mwindow  rects"]
    for name, frames in contents.items():
        for flag, label in ((0, "0"), (VJ_FLAG_CV_SCALE_IMAGE, "scale_image")):
            if args.only and args.only != label:
                continue
            env.detect_opencv(c, frames, flags=flag)   # warm-up: plan, buffers
            ti, tc, tw = [], [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                r = env.detect_opencv(c, frames, flags=flag)
                tw.append((time.perf_counter() - t0) * 1e3)
                ti.append(r.integral_ms)
                tc.append(r.cascade_ms)
            k = env.detect_opencv(c, frames, flags=flag | VJ_FLAG_COUNTERS)
            mc = statistics.median(tc)
            lines.append(f"{name:9s} {label:12s} {statistics.median(ti):11.3f}  {mc:9.3f}  {statistics.median(tw):8.2f}  "
                         f"{k.windows // args.frames:13d}  {k.stage_entered[0] // args.frames:21d}  {mc * 1e3 / (k.windows / 1e6):17.2f}  "
                         f"{len(r.rects)}")
            print(lines[-1], flush=True)
    env.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
