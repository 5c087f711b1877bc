"""By-hand measurement of detect_opencv_rois with VJ_FLAG_CV_SCALE_IMAGE against the parent commit (run on the GPU box:
`python tests/measure_cv_rois_scale_image.py PARENT_ROOT [repeats] [out.json]`; not collected by pytest).  PARENT_ROOT is a built
checkout of the commit to compare with (its clfacedetection_amd package with libvjhip.so in it); this tree is the other side.
Workload: 16 drawn-faces frames of 640 x 360; the regions are what frontalface_alt2 finds in them — its raw candidates
(min_neighbors 0) and its grouped faces (min_neighbors 3); the second cascade is mcs_lefteye with VJ_FLAG_CV_SCALE_IMAGE inside
every region.  At the parent that call is one detect_opencv call per region size; here it is one pass per canvas of level images.
Each side runs in processes of its own, alternating parent / this / parent / this: the two processes of ONE side are its A/A pair,
and their difference is the spread a difference between the sides has to exceed.  A process warms both workloads up, then takes the
median of `repeats` calls: wall time (the call ends in the library's stream synchronise) and the device time the result reports
(integral_ms, which holds the pyramid launches, + cascade_ms).  The rectangles of both sides must be equal.  Writes
profiles/cv_rois_scale_image.json (or the given file)."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES, H, W = 16, 360, 640
WORKLOADS = {"raw": 0, "grouped": 3}   # name -> min_neighbors of frontalface_alt2


def child(root, repeats):
    sys.path.insert(0, root)
    try:
        import torch  # noqa: F401  (first: see conftest.py)
    except Exception:
        pass
    import numpy as np
    from clfacedetection_amd import VJ_FLAG_COUNTERS, VJ_FLAG_CV_SCALE_IMAGE, Cascade, Environment, synth
    env = Environment(0)
    first, second = Cascade.load("frontalface_alt2"), Cascade.load("mcs_lefteye")
    frames = np.stack([synth.frame("faces", 1 + k, H, W) for k in range(N_FRAMES)])
    out = {"root": root, "device": env.device_name, "workloads": {}}
    for name, mn in WORKLOADS.items():
        r1 = env.detect_opencv(first, frames, min_neighbors=mn)
        rois = np.array([(int(r["frame"]), int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in r1.rects], np.int32).reshape(-1, 5)
        env.detect_opencv_rois(second, frames, rois, flags=VJ_FLAG_CV_SCALE_IMAGE)                       # warm-up
        counted = env.detect_opencv_rois(second, frames, rois, flags=VJ_FLAG_CV_SCALE_IMAGE | VJ_FLAG_COUNTERS)
        e = {"regions": len(rois), "region_sizes": len({(int(r[3]), int(r[4])) for r in rois}), "windows": counted.windows,
             "rects": len(counted.rects), "rects_sha1": hashlib.sha1(np.ascontiguousarray(counted.rects).tobytes()).hexdigest()}
        if hasattr(env, "cv_rois_info"):
            i = env.cv_rois_info()
            e["info"] = {"route": i.route, "level_images": i.level_images, "canvases": i.canvases, "canvas": [i.canvas_w, i.canvas_h]}
        wall, dev, pyr = [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            r = env.detect_opencv_rois(second, frames, rois, flags=VJ_FLAG_CV_SCALE_IMAGE)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(r.integral_ms + r.cascade_ms)
            if hasattr(env, "cv_rois_info"):
                pyr.append(env.cv_rois_info().pyramid_ms)
        for k, v in (("wall_ms", wall), ("device_ms", dev), ("pyramid_ms", pyr)):
            if v:
                e[k] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
        out["workloads"][name] = e
    print("RESULT " + json.dumps(out))


def main():
    parent = os.path.abspath(sys.argv[1])
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, "profiles", "cv_rois_scale_image.json")
    assert repeats >= 7
    runs = []
    for side, root in (("parent", parent), ("this", HERE), ("parent", parent), ("this", HERE)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, str(repeats)], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"{side} process failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        runs.append(dict(json.loads(line[7:]), side=side))
        print(side, line[7:])
    result = {"frames": N_FRAMES, "size": [W, H], "first": "frontalface_alt2", "second": "mcs_lefteye", "repeats": repeats, "runs": runs,
              "summary": {}}
    for name in WORKLOADS:
        per = {s: [r["workloads"][name] for r in runs if r["side"] == s] for s in ("parent", "this")}
        assert len({e["rects_sha1"] for es in per.values() for e in es}) == 1, f"{name}: the two sides' rectangles differ"
        s = {}
        for k in ("wall_ms", "device_ms"):
            med = {side: [e[k]["median"] for e in es] for side, es in per.items()}
            s[k] = {"parent": med["parent"], "this": med["this"],
                    "aa_spread": round(max(abs(v[0] - v[1]) for v in med.values()), 3),
                    "parent_minus_this": round(statistics.mean(med["parent"]) - statistics.mean(med["this"]), 3),
                    "this_over_parent": round(statistics.mean(med["this"]) / statistics.mean(med["parent"]), 4)}
        result["summary"][name] = s
        print(name, json.dumps(s))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) > 1:
        main()
    else:
        sys.exit(__doc__)
