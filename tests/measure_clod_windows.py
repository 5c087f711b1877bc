"""By-hand measurement of vj_run_windows (run on the GPU box: `python tests/measure_clod_windows.py [repeats] [out.json]`; not
collected by pytest).  One 1920 x 1080 drawn-faces frame, frontalface_alt, every grid position of the 1.1f chain (setupScale's
step and end_point, positions lrint of the f32 product) as ONE list.  Reported: the median over `repeats` calls after a warm-up of
the pass's DEVICE time (vj_run_windows_timing: hipEvents around the kernel launch) and windows/s from it, next to the integral's
device time and the wall time of the whole call.  The yardstick, in the same run on the same list: vj_run_windows_opencv (the f64
profile's pass, its scales the same values as doubles).  The two profiles differ in arithmetic, in the edge rule and in the
stump-parallel tail only the OpenCV pass has, so their verdicts are not compared.  No pass mark.  Writes profiles/clod_windows.json
(or the given file)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 1080, 1920


def chain_grid(c, width, height):
    """(scales float32[k], windows int32[n, 4]): the accepted scales of Cascade.plan_scales and every position of their grids."""
    scales, rows = [], []
    for s in c.plan_scales(width, height):
        if not s.accepted or s.nx <= 0 or s.ny <= 0:
            continue
        step = np.float32(s.step)
        xs = np.rint((np.arange(s.nx, dtype=np.float32) * step).astype(np.float64)).astype(np.int32)
        ys = np.rint((np.arange(s.ny, dtype=np.float32) * step).astype(np.float64)).astype(np.int32)
        g = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
        rows.append(np.column_stack([np.zeros(len(g), np.int32), g, np.full(len(g), len(scales), np.int32)]))
        scales.append(np.float32(s.scale))
    return np.array(scales, np.float32), np.ascontiguousarray(np.concatenate(rows).astype(np.int32))


def main(argv):
    sys.path.insert(0, ROOT)
    try:
        import torch  # noqa: F401  (first: see conftest.py)
    except Exception:
        pass
    from clfacedetection_amd import Cascade, Environment, run_windows, run_windows_opencv, synth

    repeats = int(argv[1]) if len(argv) > 1 else 9
    out_path = os.path.abspath(argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "clod_windows.json"))
    env = Environment(0)
    c = Cascade.load("frontalface_alt")
    frame = synth.frame("faces", 1, H, W)
    scales, windows = chain_grid(c, W, H)

    def timed(call):
        wall, integral, dev = [], [], []
        for i in range(repeats + 1):                 # the first call is the warm-up (tables, buffers)
            t0 = time.perf_counter()
            res = call()[0]
            t1 = time.perf_counter()
            if i:
                ims, pms = env.run_windows_timing()
                wall.append((t1 - t0) * 1e3)
                integral.append(ims)
                dev.append(pms)
        return res, wall, integral, dev

    def entry(res, wall, integral, dev):
        pass_ms = statistics.median(dev)
        return {"pass_ms_median": round(pass_ms, 3), "pass_ms_min_max": [round(min(dev), 3), round(max(dev), 3)],
                "windows_per_s": round(len(windows) / (pass_ms * 1e-3)), "integral_ms_median": round(statistics.median(integral), 3),
                "call_wall_ms_median": round(statistics.median(wall), 3), "passes": int((res == 1).sum())}

    clod = entry(*timed(lambda: run_windows(frame, c, env, windows, scales)))
    cv = entry(*timed(lambda: run_windows_opencv(frame, c, env, windows, scales.astype(np.float64))))
    result = {"device": env.device_name, "size": [W, H], "cascade": "frontalface_alt", "scales": int(len(scales)),
              "windows": int(len(windows)), "repeats": repeats, "run_windows": clod, "run_windows_opencv": cv,
              "clod_over_opencv_pass_time": round(clod["pass_ms_median"] / cv["pass_ms_median"], 3)}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main(sys.argv)
