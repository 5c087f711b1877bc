"""By-hand measurement of CV_HAAR_FIND_BIGGEST_OBJECT against the plain OpenCV-profile path (run on the GPU box:
`python tests/measure_find_biggest.py [frames] [repeats] [out.json]`; not collected by pytest).  64 frames of 1920 x 1080,
frontalface_alt, min_neighbors 3:
  (a) frames with one crude face of about 400 pixels each, at differing positions and sizes;
  (b) faceless frames — the worst case of the search: every scale, one round each.
Both on the find-biggest path and on the plain path of the same build, alternating, after a warm-up call of each; a time is the
median wall time of a call that ends in the library's own stream synchronise (detect_opencv returns results), next to the device's
integral and cascade times.  `windows` comes from one counted call of each.  Writes profiles/find_biggest.json (or the given file)."""
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
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_FIND_BIGGEST, Cascade, Environment, synth  # noqa: E402

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 64
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "find_biggest.json")
H, W = 1080, 1920


def face_frames(n):
    rng = np.random.default_rng(2024)
    frames = []
    for k in range(n):
        f = synth.frame("smooth", 500 + k, H, W).copy()
        s = int(rng.integers(360, 441))
        y, x = int(rng.integers(0, H - s + 1)), int(rng.integers(0, W - s + 1))
        f[y:y + s, x:x + s] = synth.crude_face(s)
        frames.append(f)
    return np.stack(frames)


def faceless_frames(n):
    return np.stack([synth.frame("smooth", 900 + k, H, W) for k in range(n)])


env = Environment(0)
c = Cascade.load("frontalface_alt")
result = {"device": env.device_name, "frames": n_frames, "size": [W, H], "cascade": "frontalface_alt", "min_neighbors": 3,
          "repeats": repeats, "sets": {}}
for label, frames in (("faces", face_frames(n_frames)), ("faceless", faceless_frames(n_frames))):
    paths = {"find_biggest": VJ_FLAG_CV_FIND_BIGGEST, "plain": 0}
    entry = {}
    for name, flags in paths.items():       # warm-up (plans, tables, buffers) and the counted call
        env.detect_opencv(c, frames, min_neighbors=3, flags=flags)
        r = env.detect_opencv(c, frames, min_neighbors=3, flags=flags | VJ_FLAG_COUNTERS)
        entry[name] = {"windows": r.windows, "rects": len(r.rects), "frames_with_rects": len(set(int(x["frame"]) for x in r.rects)), "wall_ms": [],
                       "cascade_ms": [], "integral_ms": [], "n_cascade_launches": r.n_cascade_launches}
    for _ in range(repeats):                # alternating
        for name, flags in paths.items():
            t0 = time.perf_counter()
            r = env.detect_opencv(c, frames, min_neighbors=3, flags=flags)
            entry[name]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            entry[name]["cascade_ms"].append(r.cascade_ms)
            entry[name]["integral_ms"].append(r.integral_ms)
    for name in paths:
        for k in ("wall_ms", "cascade_ms", "integral_ms"):
            v = entry[name][k]
            entry[name][k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    entry["wall_ratio_find_biggest_over_plain"] = round(entry["find_biggest"]["wall_ms"]["median"] / entry["plain"]["wall_ms"]["median"], 3)
    entry["window_ratio_find_biggest_over_plain"] = round(entry["find_biggest"]["windows"] / max(1, entry["plain"]["windows"]), 4)
    result["sets"][label] = entry
    print(label, json.dumps(entry))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", out_path)
