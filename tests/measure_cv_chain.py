"""By-hand measurement of vj_detect_opencv_chain's device hand-off (VJ_FLAG_CV_CHAIN_DEVICE) against the unflagged route of the same
build (run on the GPU box: `python tests/measure_cv_chain.py [frames] [repeats] [out.json]`; not collected by pytest).  DESIGN.md
§4.10's workload: drawn-faces frames of 1280 x 720, frontalface_alt2 then haarcascade_eye, in two legs — the grouped faces
(min_neighbors 3) and the raw candidates (min_neighbors 0) as regions, the latter a second time with "det_cap" 2^21.
Per leg: one warm-up call of each route and one counted call (regions, units, windows, rectangles — the two routes must agree), then
an A/A pair — the unflagged call measured twice, `repeats` times each, alternating — to show the spread between two series of one
route in this process, then flagged and unflagged alternating, `repeats` times each.  A time is the median wall time of a call (both
routes end in the library's own stream synchronise), next to the device times: integral and cascade of both results (`timing`) and
the hand-off kernels (vj_cv_chain_info's handoff_ms).  Writes profiles/cv_chain_device.json (or the given file).
Measured on an MI355X (the committed record): the flagged route is 0.79 ms of 9.77 faster grouped, 2.43 ms of 49.11 faster raw and
9.41 ms faster raw with det_cap 2^21, against A/A spreads of 0.02 / 0.06 / 0.17 ms; what that means for the default: DESIGN.md §4.10."""
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
from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_CHAIN_DEVICE, Cascade, Environment, synth  # noqa: E402

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 16
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cv_chain_device.json")
H, W = 720, 1280

env = Environment(0)
first, second = Cascade.load("frontalface_alt2"), Cascade.load("eye")
frames = np.stack([synth.frame("faces", 1 + k, H, W) for k in range(n_frames)])


def call(mn, device, flags=0):
    t0 = time.perf_counter()
    r1, r2 = env.detect_opencv_chain(first, second, frames, min_neighbors=mn, flags=flags | (VJ_FLAG_CV_CHAIN_DEVICE if device else 0),
                                     flags_second=flags)
    wall = (time.perf_counter() - t0) * 1e3
    return r1, r2, env.cv_chain_info(), wall


def series():
    return {"wall_ms": [], "integral_ms": [], "first_cascade_ms": [], "second_cascade_ms": [], "handoff_ms": []}


def take(e, r1, r2, info, wall):
    e["wall_ms"].append(wall)
    e["integral_ms"].append(r1.integral_ms + r2.integral_ms)
    e["first_cascade_ms"].append(r1.cascade_ms)
    e["second_cascade_ms"].append(r2.cascade_ms)
    e["handoff_ms"].append(info.handoff_ms)


def summary(e):
    return {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in e.items()}


result = {"device": env.device_name, "frames": n_frames, "size": [W, H], "first": "frontalface_alt2", "second": "eye",
          "repeats": repeats, "legs": {}}
# (the flagged route's buffers start at "det_cap" in every call — 4 x det_cap units: the raw leg's 1.76 M units take one regrow and so one
# re-enqueued chain per call at the default 65536; the third leg gives them room, as a caller who knows the workload would)
for leg, mn, det_cap in (("grouped", 3, None), ("raw", 0, None), ("raw_det_cap_2m", 0, 1 << 21)):
    env.configure("defaults", "")
    if det_cap:
        env.configure("det_cap", str(det_cap))
    counted = {}
    for device in (False, True):            # warm-up (plans, tables, buffers) and the counted run
        call(mn, device)
        r1, r2, info, _ = call(mn, device, VJ_FLAG_COUNTERS)
        counted[device] = {"handoff": info.handoff, "sub_batches": info.sub_batches, "sub_batches_device": info.sub_batches_device,
                           "reruns": info.reruns, "regions": info.regions, "units": info.units, "windows": info.windows,
                           "windows_visited_second": r2.windows, "rects_first": len(r1.rects), "rects_second": len(r2.rects)}
    same = ("regions", "units", "windows", "windows_visited_second", "rects_first", "rects_second")
    assert all(counted[False][k] == counted[True][k] for k in same), counted
    assert counted[True]["handoff"] == 1 and counted[True]["sub_batches_device"] == counted[True]["sub_batches"], counted
    aa = [series(), series()]
    for _ in range(repeats):                # A/A: the unflagged route against itself
        for e in aa:
            take(e, *call(mn, False))
    host, dev = series(), series()
    for _ in range(repeats):                # alternating
        take(host, *call(mn, False))
        take(dev, *call(mn, True))
    aa, host, dev = [summary(e) for e in aa], summary(host), summary(dev)
    spread = abs(aa[0]["wall_ms"]["median"] - aa[1]["wall_ms"]["median"])
    diff = host["wall_ms"]["median"] - dev["wall_ms"]["median"]
    result["legs"][leg] = {"min_neighbors": mn, "det_cap": det_cap or "default", "counted_host": counted[False], "counted_device": counted[True], "aa_host": aa,
                           "host": host, "device": dev, "aa_wall_spread_ms": round(spread, 3),
                           "wall_ms_host_minus_device": round(diff, 3), "device_faster_beyond_spread": bool(diff > spread)}
    print(leg, json.dumps(result["legs"][leg]))
env.configure("defaults", "")
result["flip_default"] = all(result["legs"][k]["device_faster_beyond_spread"] for k in ("grouped", "raw"))
print("device route faster than the unflagged one by more than the A/A spread on both legs:", result["flip_default"])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print("wrote", out_path)
