"""By-hand measurement of the mixed-size entry points against what the library offered before them (run on the GPU box; not
collected by pytest):
    python tests/measure_mixed.py compare PARENT_LIB [out.json]    the caller's loop on the parent's library against the new call
    python tests/measure_mixed.py sweep [out.json]                 groups of equal frames: on the atlas against a call of their own
PARENT_LIB is libvjhip.so built from the parent commit.  What is compared: the parent's offering — a loop with one detect_opencv
(and one detect) call per distinct frame size, frames of equal size batched together — and ONE detect_opencv_mixed (detect_mixed)
call.  Every side runs in a process of its own (`child`), the sides alternate, each side runs twice (the A/A pair: the spread
between its two medians is what a difference has to exceed), a time is the median wall time of nine calls after two warm-up calls,
and the results are compared by hash.  Workloads, drawn-faces frames with fixed seeds, frontalface_alt:
    A  64 frames of 64 distinct sizes, widths 160 .. 640 and heights 120 .. 480
    B  64 frames of 4 sizes x 16
    C  8 frames of 8 distinct sizes near 1920 x 1080
The sweep runs on this commit alone: groups of 1, 2, 4, 8 and 16 equal frames of 320 x 240 and of 1280 x 720 through
detect_opencv_mixed with own_call_px = never (atlas) and = 1 (a batched call of their own), alternating; the break-even in group
pixels, rounded to a power of two, is the default of vj_mixed_opts::own_call_px.  Both write under profiles/."""
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

REPEATS, WARMUP = 9, 2
NEVER = 2**64 - 1
HBM_PEAK_GBS = 8000.0     # MI355X: 8 TB/s


def sizes_of(workload):
    if workload == "A":
        return [(160 + round(i * 480 / 63), 120 + round(((i * 37) % 64) * 360 / 63)) for i in range(64)]
    if workload == "B":
        return [s for s in [(320, 240), (480, 360), (640, 480), (240, 320)] for _ in range(16)]
    return [(1920 - 8 * i, 1080 - 6 * i) for i in range(8)]


def frames_of(workload):
    from clfacedetection_amd import synth
    return [synth.frame("faces", 1 + i, h, w) for i, (w, h) in enumerate(sizes_of(workload))]


def use_library(path):
    """Bind the given libvjhip.so instead of the tree's (a parent build lacks the newest symbols: they stay unbound)."""
    import clfacedetection_amd.api as api
    lib = C.CDLL(path)
    for name, (res, args) in api._SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    api._lib = lib


def digest(rects):
    h = hashlib.sha256()
    for k in ("frame", "scale_idx", "y", "x", "w", "h"):
        h.update(np.ascontiguousarray(rects[k]).tobytes())
    return h.hexdigest()[:16]


def loop_per_size(detect, frames):
    """The caller's loop: one call per distinct size, frames of equal size batched; -> rectangles in the mixed call's order."""
    by_size = {}
    for i, f in enumerate(frames):
        by_size.setdefault(f.shape, []).append(i)
    parts = []
    for shape, idx in by_size.items():
        r = detect(np.stack([frames[i] for i in idx])).rects
        r["frame"] = np.asarray(idx, np.int32)[r["frame"]]
        parts.append(r)
    r = np.concatenate(parts)
    return r[np.argsort(r["frame"], kind="stable")]


def timed(fn):
    for _ in range(WARMUP):
        out = fn()
    t = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return out, {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def child(side, workload, lib_path):
    if lib_path:
        use_library(lib_path)
    from clfacedetection_amd import Cascade, Environment
    env, c = Environment(0), Cascade.load("frontalface_alt")
    frames = frames_of(workload)
    out = {"side": side, "workload": workload, "frames": len(frames), "sizes": len({f.shape for f in frames})}
    for profile in ("opencv", "clod"):
        if side == "loop":
            fn = (lambda: loop_per_size(lambda b: env.detect_opencv(c, b), frames)) if profile == "opencv" else \
                 (lambda: loop_per_size(lambda b: env.detect(c, b), frames))
            rects, t = timed(fn)
        else:
            fn = (lambda: env.detect_opencv_mixed(c, frames)) if profile == "opencv" else (lambda: env.detect_mixed(c, frames))
            r, t = timed(fn)
            rects = r.rects
            i = env.mixed_info()
            # bytes the pack launches moved, read and written (gray frames): known here only when every frame went onto an atlas
            moved = 2 * sum(f.size for f in frames) if i.frames_atlas == len(frames) else None
            out[profile + "_info"] = {"atlases": i.atlases, "atlas": [i.atlas_w, i.atlas_h], "on_atlas": i.frames_atlas, "own_calls": i.own_calls,
                                      "pack_ms": round(i.pack_ms, 4), "pack_bytes": moved,
                                      "pack_fraction_of_hbm_peak": round(moved / max(i.pack_ms, 1e-6) / 1e6 / HBM_PEAK_GBS, 4) if moved else None,
                                      "integral_ms": round(r.integral_ms, 3), "cascade_ms": round(r.cascade_ms, 3)}
        out[profile] = dict(t, rects=len(rects), hash=digest(rects))
    env.close()
    print("RESULT " + json.dumps(out))


def run_child(side, workload, lib_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", side, workload, lib_path or ""], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child {side} {workload} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def compare(parent_lib, out_path):
    result = {"repeats": REPEATS, "warmup": WARMUP, "cascade": "frontalface_alt", "workloads": {}}
    for workload in ("A", "B", "C"):
        runs = [run_child("loop", workload, parent_lib), run_child("mixed", workload, None),      # alternating, an A/A pair per side
                run_child("loop", workload, parent_lib), run_child("mixed", workload, None)]
        w = {"frames": runs[0]["frames"], "sizes": runs[0]["sizes"]}
        for profile in ("opencv", "clod"):
            loop, mixed = [runs[0][profile], runs[2][profile]], [runs[1][profile], runs[3][profile]]
            assert len({x["hash"] for x in loop + mixed}) == 1, (workload, profile, loop, mixed)   # the same rectangles in the same order
            med = lambda xs: [x["median"] for x in xs]
            spread = max(abs(med(loop)[0] - med(loop)[1]), abs(med(mixed)[0] - med(mixed)[1]))
            w[profile] = {"rects": loop[0]["rects"], "loop_ms": med(loop), "mixed_ms": med(mixed), "aa_spread_ms": round(spread, 3),
                          "mixed_over_loop": round(statistics.mean(med(mixed)) / statistics.mean(med(loop)), 3),
                          "info": runs[3][profile + "_info"]}
            print(workload, profile, json.dumps(w[profile]))
        result["workloads"][workload] = w
    write(result, out_path)


def sweep(out_path):
    from clfacedetection_amd import Cascade, Environment, synth
    env, c = Environment(0), Cascade.load("frontalface_alt")
    result = {"device": env.device_name, "repeats": REPEATS, "cascade": "frontalface_alt", "groups": []}
    for (w, h) in ((320, 240), (1280, 720)):
        for n in (1, 2, 4, 8, 16):
            frames = [synth.frame("faces", 1 + i, h, w) for i in range(n)]
            routes = {"atlas": lambda: env.detect_opencv_mixed(c, frames, own_call_px=NEVER), "own_call": lambda: env.detect_opencv_mixed(c, frames, own_call_px=1)}
            t, hashes = {k: [] for k in routes}, set()
            for fn in routes.values():
                for _ in range(WARMUP):
                    fn()
            for _ in range(REPEATS):                     # alternating
                for k, fn in routes.items():
                    t0 = time.perf_counter()
                    r = fn()
                    t[k].append((time.perf_counter() - t0) * 1e3)
                    hashes.add(digest(r.rects))
            assert len(hashes) == 1
            e = {"size": [w, h], "frames": n, "group_px": w * h * n, "atlas_ms": round(statistics.median(t["atlas"]), 3),
                 "own_call_ms": round(statistics.median(t["own_call"]), 3)}
            result["groups"].append(e)
            print(json.dumps(e))
    env.close()
    write(result, out_path)


def write(result, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "child":
        child(sys.argv[2], sys.argv[3], sys.argv[4] or None)
    elif mode == "compare":
        compare(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "mixed_sizes.json"))
    elif mode == "sweep":
        sweep(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "mixed_sizes_sweep.json"))
    else:
        raise SystemExit(__doc__)
