"""By-hand measurement of the OpenCV profile's chain against what the library offered before it (run on the GPU box:
`python tests/measure_cv_rois.py [frames] [repeats] [out.json]`; not collected by pytest).  The BASELINE config 5 shape in this
profile: frontalface_alt2 grouped with min_neighbors 3, then haarcascade_eye inside every face, on drawn-faces frames of 1280 x 720.
  (a) detect_opencv_chain: one upload and one set of integral images per sub-batch for both cascades, all regions in one pass;
  (b) detect_opencv, then one detect_opencv call per region size on sub-image views — every call uploads and integrates its
      sub-images again.
The two routes alternate after a warm-up call of each; a time is the median wall time of a route (both end in the library's own
stream synchronise), next to the device's integral and cascade times summed over the route's calls.  `windows` comes from one counted
run of each route.  Writes profiles/cv_rois.json (or the given file)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass
from clfacedetection_amd import VJ_FLAG_COUNTERS, Cascade, Environment, synth  # noqa: E402

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cv_rois.json")
H, W = 720, 1280

env = Environment(0)
first, second = Cascade.load("frontalface_alt2"), Cascade.load("eye")
frames = np.stack([synth.frame("faces", 1 + k, H, W) for k in range(n_frames)])


def route_chain(flags=0):
    r1, r2 = env.detect_opencv_chain(first, second, frames, min_neighbors=3, flags=flags, flags_second=flags)
    return r1, [r2]


def route_per_size(flags=0):
    r1 = env.detect_opencv(first, frames, min_neighbors=3, flags=flags)
    by_size = {}
    for r in r1.rects:
        by_size.setdefault((int(r["w"]), int(r["h"])), []).append(r)
    parts = []
    for (w, h), rs in sorted(by_size.items()):
        views = [frames[int(r["frame"])][int(r["y"]):int(r["y"]) + h, int(r["x"]):int(r["x"]) + w] for r in rs]
        parts.append(env.detect_opencv(second, views, flags=flags))
    return r1, parts


routes = {"chain": route_chain, "per_region_size": route_per_size}
result = {"device": env.device_name, "frames": n_frames, "size": [W, H], "first": "frontalface_alt2", "min_neighbors": 3, "second": "eye",
          "repeats": repeats, "routes": {}}
for name, fn in routes.items():          # warm-up (plans, tables, buffers) and the counted run
    fn()
    r1, parts = fn(VJ_FLAG_COUNTERS)
    result["routes"][name] = {"regions": len(r1.rects), "region_sizes": len({(int(r["w"]), int(r["h"])) for r in r1.rects}),
                              "second_calls": len(parts), "windows_first": r1.windows, "windows_second": sum(p.windows for p in parts),
                              "rects_second": sum(len(p.rects) for p in parts), "wall_ms": [], "integral_ms": [], "cascade_ms": [],
                              "second_cascade_ms": []}
for _ in range(repeats):                 # alternating
    for name, fn in routes.items():
        t0 = time.perf_counter()
        r1, parts = fn()
        e = result["routes"][name]
        e["wall_ms"].append((time.perf_counter() - t0) * 1e3)
        e["integral_ms"].append(r1.integral_ms + sum(p.integral_ms for p in parts))
        e["cascade_ms"].append(r1.cascade_ms + sum(p.cascade_ms for p in parts))
        e["second_cascade_ms"].append(sum(p.cascade_ms for p in parts))
for name in routes:
    e = result["routes"][name]
    for k in ("wall_ms", "integral_ms", "cascade_ms", "second_cascade_ms"):
        v = e[k]
        e[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    print(name, json.dumps(e))
a, b = result["routes"]["chain"], result["routes"]["per_region_size"]
assert a["regions"] == b["regions"] and a["windows_second"] == b["windows_second"] and a["rects_second"] == b["rects_second"]
result["wall_ratio_chain_over_per_region_size"] = round(a["wall_ms"]["median"] / b["wall_ms"]["median"], 3)
print("chain / per-region-size wall:", result["wall_ratio_chain_over_per_region_size"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", out_path)
