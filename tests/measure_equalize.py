"""By-hand measurement of VJ_FLAG_EQUALIZE_HIST (run on the GPU box; not collected by pytest):
    python tests/measure_equalize.py compare PARENT_LIB [out.json]     the parent's offering on the parent's library against the flag
    python tests/measure_equalize.py stage [out.json] [NAME=LIB ...]   the stage alone, for this tree's library and other builds of it
PARENT_LIB is libvjhip.so built from the parent commit.  `compare`: what a caller had before — vj_grayscale per frame, equalization
on the host in numpy (the restatement's arithmetic, vectorised; a caller with OpenCV would call cv::equalizeHist, which is faster),
detect_opencv on the gray frames — against ONE call with the flag.  Workloads: `hd`, 64 device-resident BGR frames of 1920 x 1080
through detect_opencv; `A`, the 64 sizes of tests/measure_mixed.py (host, gray) through detect_opencv_mixed, the parent's side with
one call per size.  Every side runs in a process of its own, the sides alternate, each side runs twice (the A/A pair: the spread
between its two medians is what a difference has to exceed), a time is the median wall time of nine calls after two warm-up calls,
and the rectangles are compared by hash.
`stage`: 64 device-resident frames of 1920 x 1080 — gray noise, gray constant, gray smooth, BGR noise — through detect_opencv with and without the
flag (min_size 800: a short cascade pass; the stage does not depend on it): the stage's device time is the difference of
vj_timing.integral_ms (events around the memset, the three launches and the integral launches), median of nine after two warm-ups,
twice (the A/A pair); bytes moved = 3 per gray pixel (one read per pass, one write), 2 * channels + 1 per colour pixel, against the
8 TB/s HBM peak.  And the headline step (detect, clod profile, the gray noise batch) with and without the flag, wall time.
NAME=LIB: the same in a process that binds LIB — builds with other -DEQ_HIST_COPIES / -DEQ_HIST_BALLOT (csrc/vj_equalize.hip)."""
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

from measure_mixed import REPEATS, WARMUP, HBM_PEAK_GBS, digest, frames_of, loop_per_size, timed, use_library  # noqa: E402

EQ = 1 << 11
N_HD, H_HD, W_HD = 64, 1080, 1920


def equalize_host(gray):
    """tests/equalize_oracle.py's arithmetic without the Python loop."""
    hist = np.bincount(gray.reshape(-1), minlength=256)
    i = int(np.flatnonzero(hist)[0])
    if hist[i] == gray.size:
        return gray.copy()
    scale = np.float32(255.0) / np.float32(gray.size - int(hist[i]))
    sums = np.cumsum(np.where(np.arange(256) > i, hist, 0))
    lut = np.clip(np.rint(sums.astype(np.float32) * scale), 0, 255).astype(np.uint8)
    return lut[gray]


def hd_batch(kind, channels):
    """64 frames of 1920 x 1080 on the device -> (DeviceFrames, the tensor that owns them)."""
    import torch
    from clfacedetection_amd import DeviceFrames, synth
    if kind == "constant":
        host = np.full((N_HD, H_HD, W_HD), 128, np.uint8)
    else:
        host = np.stack([synth.frame(kind, 1 + i, H_HD, W_HD) for i in range(N_HD)])
    if channels > 1:
        host = np.ascontiguousarray(np.stack([host, host[:, ::-1], host[:, :, ::-1]] + [host] * (channels - 3), axis=3))
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return DeviceFrames.from_torch(t), t


def grayscale_device(env, frames, i):
    """vj_grayscale on frame i of a device-resident batch (Environment.grayscale takes host arrays only)."""
    import ctypes as C
    from clfacedetection_amd.api import _Image, _check, load_library
    im = _Image(frames.ptr + i * frames.stride * frames.height, frames.width, frames.height, frames.stride, 1, frames.channels)
    g = np.empty((frames.height, frames.width), np.uint8)
    _check(load_library().vj_grayscale(env._h, C.byref(im), g.ctypes.data, g.strides[0]), "vj_grayscale")
    return g


def child_compare(side, workload, lib_path):
    if lib_path:
        use_library(lib_path)
    from clfacedetection_amd import Cascade, Environment
    env, c = Environment(0), Cascade.load("frontalface_alt")
    if workload == "hd":
        d, keep = hd_batch("faces", 3)
        if side == "parent":
            fn = lambda: env.detect_opencv(c, np.stack([equalize_host(grayscale_device(env, d, i)) for i in range(d.n)])).rects
        else:
            fn = lambda: env.detect_opencv(c, d, flags=EQ).rects
    else:
        frames = frames_of(workload)
        if side == "parent":
            fn = lambda: loop_per_size(lambda b: env.detect_opencv(c, b), [equalize_host(f) for f in frames])
        else:
            fn = lambda: env.detect_opencv_mixed(c, frames, flags=EQ).rects
    rects, t = timed(fn)
    env.close()
    print("RESULT " + json.dumps(dict(t, side=side, workload=workload, rects=len(rects), hash=digest(rects))))


def child_stage(lib_path):
    if lib_path:
        use_library(lib_path)
    from clfacedetection_amd import Cascade, Environment, default_params
    env, c = Environment(0), Cascade.load("frontalface_alt")
    out = {"device": env.device_name, "frames": [N_HD, W_HD, H_HD], "batches": {}}
    med = lambda xs: round(statistics.median(xs), 4)
    for name, kind, ch in (("gray_noise", "noise", 1), ("gray_constant", "constant", 1), ("gray_smooth", "smooth", 1), ("bgr_noise", "noise", 3)):
        d, keep = hd_batch(kind, ch)
        pairs = []
        for _ in range(2):                                  # the A/A pair
            t = {0: [], EQ: []}
            for k in range(WARMUP + REPEATS):
                for flags in (0, EQ):                       # alternating
                    r = env.detect_opencv(c, d, min_size=(800, 800), flags=flags)
                    if k >= WARMUP:
                        t[flags].append(r.integral_ms)
            pairs.append(round(med(t[EQ]) - med(t[0]), 4))
        moved = N_HD * H_HD * W_HD * (2 * ch + 1)
        stage = statistics.mean(pairs)
        out["batches"][name] = {"stage_ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4), "integral_ms_without": med(t[0]),
                                "bytes": moved, "tb_per_s": round(moved / stage / 1e9, 3), "fraction_of_hbm_peak": round(moved / stage / 1e6 / HBM_PEAK_GBS, 4)}
        if name == "gray_noise":                            # the headline step with and without the flag
            step = {}
            for _ in range(2):
                for flags in (0, EQ):
                    _, tt = timed(lambda: env.detect(c, d, default_params(flags=flags)))
                    step.setdefault("with" if flags else "without", []).append(tt["median"])
            out["headline_step_ms"] = step
        del d, keep
    env.close()
    print("RESULT " + json.dumps(out))


def write(key, value, out_path):
    """Both modes keep their results in one file, under a key each."""
    result = json.load(open(out_path)) if os.path.exists(out_path) else {}
    result[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out_path)


def run_child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def compare(parent_lib, out_path):
    result = {"repeats": REPEATS, "warmup": WARMUP, "cascade": "frontalface_alt", "workloads": {}}
    for workload in ("hd", "A"):
        runs = [run_child("compare", s, workload, lib) for s, lib in (("parent", parent_lib), ("flag", ""), ("parent", parent_lib), ("flag", ""))]
        assert len({x["hash"] for x in runs}) == 1, runs        # the same rectangles in the same order
        parent, flag = [runs[0]["median"], runs[2]["median"]], [runs[1]["median"], runs[3]["median"]]
        w = {"rects": runs[0]["rects"], "parent_ms": parent, "flag_ms": flag,
             "aa_spread_ms": round(max(abs(parent[0] - parent[1]), abs(flag[0] - flag[1])), 3),
             "flag_over_parent": round(statistics.mean(flag) / statistics.mean(parent), 3)}
        print(workload, json.dumps(w))
        result["workloads"][workload] = w
    write("compare", result, out_path)


def stage(out_path, builds):
    result = {"repeats": REPEATS, "warmup": WARMUP, "builds": {}}
    for name, lib in [("tree", "")] + builds:
        result["builds"][name] = run_child("stage", lib)
        print(name, json.dumps(result["builds"][name]))
    write("stage", result, out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "child" and sys.argv[2] == "compare":
        child_compare(sys.argv[3], sys.argv[4], sys.argv[5] or None)
    elif mode == "child" and sys.argv[2] == "stage":
        child_stage(sys.argv[3] or None)
    elif mode == "compare":
        compare(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "equalize.json"))
    elif mode == "stage":
        rest = sys.argv[2:]
        out = rest.pop(0) if rest and "=" not in rest[0] else os.path.join(ROOT, "profiles", "equalize.json")
        stage(out, [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in rest])
    else:
        raise SystemExit(__doc__)
