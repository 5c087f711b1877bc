"""By-hand measurement of vj_preprocess (run on the GPU box; not collected by pytest):
    python tests/measure_preprocess.py compare PARENT_LIB [out.json]    the parent's offering on the parent's library against preprocess
    python tests/measure_preprocess.py stage [out.json] [NAME=LIB ...]  the stage alone, for this tree's library and other builds of it
PARENT_LIB is libvjhip.so built from the parent commit.  Workload of `compare`: 64 device-resident BGR frames of 1920 x 1080 to
960 x 540, equalized, then detect_opencv with frontalface_alt.  The parent's side is what a caller had before: vj_resize_linear per
frame to the host, equalization on the host in numpy (the restatement's arithmetic, vectorised), detect_opencv on the host frames;
the other side is preprocess(), then detect_opencv on its output.  Every side runs in a process of its own, the sides alternate,
each side runs twice (the A/A pair: the spread between its two medians is what a difference has to exceed), a time is the median
wall time of nine calls after two warm-up calls, and the rectangles are compared by hash.
`stage`: the device time of one preprocess() call by the library's events (vj_preprocess_timing: around its copy of the records and
taps, the memset and the launches), median of nine after two warm-ups, twice (the A/A pair), for 64 x 1080p gray and BGR to half size
with and without equalization, the eleven sizes of tests/mixed_cases.py to half size (device-resident), and 64 x 1080p gray without
a resize, equalized — next to §4.15's stage on the same frames in the same run (the difference of vj_timing.integral_ms of
detect_opencv with and without VJ_FLAG_EQUALIZE_HIST, as tests/measure_equalize.py takes it).  Bytes a call must move: the source once,
the output once, and with equalization the output once more in each direction (the table is applied in place); against the 8 TB/s
HBM peak.  NAME=LIB: the same in a process that binds LIB — a build with -DPREP_UNFUSED_HIST (prep_resize<false>, then a histogram
pass over the output); the builds alternate, each runs twice.
(What the four-pixel dword store buys over pyramid_levels' byte stores is measured by tools/microbench/prep_stores.hip, a stand-alone
program: no entry point launches pyramid_levels on a batch of one level per frame.)"""
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

from measure_equalize import EQ, H_HD, N_HD, W_HD, equalize_host, hd_batch, write  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP, digest, timed, use_library  # noqa: E402

HALF = (W_HD // 2, H_HD // 2)


def hd_faces_bgr():
    """hd_batch("faces", 3), the host array kept in the temporary directory between the processes of one measurement."""
    import tempfile
    import torch
    from clfacedetection_amd import DeviceFrames, synth
    path = os.path.join(tempfile.gettempdir(), f"measure_preprocess_faces_{N_HD}x{H_HD}x{W_HD}x3.npy")
    if os.path.exists(path):
        host = np.load(path)
    else:
        gray = np.stack([synth.frame("faces", 1 + i, H_HD, W_HD) for i in range(N_HD)])
        host = np.ascontiguousarray(np.stack([gray, gray[:, ::-1], gray[:, :, ::-1]], axis=3))
        np.save(path + ".tmp.npy", host)
        os.replace(path + ".tmp.npy", path)
    t = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return DeviceFrames.from_torch(t), t


def child_compare(side, lib_path):
    if lib_path:
        use_library(lib_path)
    from clfacedetection_amd import Cascade, DeviceFrames, Environment
    env, c = Environment(0), Cascade.load("frontalface_alt")
    d, keep = hd_faces_bgr()
    if side == "parent":
        def fn():
            frames = []
            for i in range(d.n):
                one = DeviceFrames(d.ptr + i * d.stride * d.height, 1, d.height, d.width, d.stride, d.channels)
                frames.append(equalize_host(env.resize_linear(one, *HALF)))
            return env.detect_opencv(c, np.stack(frames)).rects
    else:
        fn = lambda: env.detect_opencv(c, env.preprocess(d, size=HALF, equalize=True)[0]).rects
    rects, t = timed(fn)
    env.close()
    print("RESULT " + json.dumps(dict(t, side=side, rects=len(rects), hash=digest(rects))))


def child_stage(lib_path):
    import torch
    if lib_path:
        use_library(lib_path)
    import mixed_cases as mc
    from clfacedetection_amd import Cascade, DeviceFrames, Environment
    env, c = Environment(0), Cascade.load("frontalface_alt")
    out = {"device": env.device_name, "cases": {}}
    med = lambda xs: round(statistics.median(xs), 4)

    def measure(name, frames, src_bytes, **kw):
        recs, nbytes = env.preprocess_layout(frames, **kw)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        dst_px = sum(w * h for _, w, h, _ in recs)
        moved = src_bytes + dst_px * (3 if kw.get("equalize") else 1)
        pairs = []
        for _ in range(2):                                  # the A/A pair
            t = []
            for k in range(WARMUP + REPEATS):
                env.preprocess(frames, out=buf, **kw)
                if k >= WARMUP:
                    t.append(env.preprocess_timing())
            pairs.append(med(t))
        ms = statistics.mean(pairs)
        out["cases"][name] = {"ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4), "bytes": moved,
                              "tb_per_s": round(moved / ms / 1e9, 3), "fraction_of_hbm_peak": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)}

    for ch, label in ((1, "gray"), (3, "bgr")):
        d, keep = hd_batch("noise", ch)
        src = N_HD * H_HD * W_HD * ch
        measure(f"hd_{label}_half", d, src, size=HALF)
        measure(f"hd_{label}_half_equalize", d, src, size=HALF, equalize=True)
        if ch == 1:
            measure("hd_gray_no_resize_equalize", d, src, equalize=True)
            pairs = []                                      # §4.15's stage on the same frames
            for _ in range(2):
                t = {0: [], EQ: []}
                for k in range(WARMUP + REPEATS):
                    for flags in (0, EQ):
                        r = env.detect_opencv(c, d, min_size=(800, 800), flags=flags)
                        if k >= WARMUP:
                            t[flags].append(r.integral_ms)
                pairs.append(round(med(t[EQ]) - med(t[0]), 4))
            out["cases"]["hd_gray_equalize_flag_stage"] = {"ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4)}
        del d, keep
    keep = [torch.from_numpy(np.array(f)).cuda() for f in mc.frames()]
    torch.cuda.synchronize()
    items = [DeviceFrames.from_torch(t[None]) for t in keep]
    measure("mixed_eleven_half_equalize", items, sum(f.size for f in mc.frames()), fx=0.5, fy=0.5, equalize=True)
    env.close()
    print("RESULT " + json.dumps(out))


def run_child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *args], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def compare(parent_lib, out_path):
    runs = [run_child("compare", s, lib) for s, lib in (("parent", parent_lib), ("prep", ""), ("parent", parent_lib), ("prep", ""))]
    assert len({x["hash"] for x in runs}) == 1, runs            # the same rectangles in the same order
    parent, prep = [runs[0]["median"], runs[2]["median"]], [runs[1]["median"], runs[3]["median"]]
    result = {"repeats": REPEATS, "warmup": WARMUP, "cascade": "frontalface_alt", "frames": [N_HD, W_HD, H_HD, 3], "to": list(HALF),
              "rects": runs[0]["rects"], "parent_ms": parent, "preprocess_ms": prep,
              "aa_spread_ms": round(max(abs(parent[0] - parent[1]), abs(prep[0] - prep[1])), 3),
              "preprocess_over_parent": round(statistics.mean(prep) / statistics.mean(parent), 4)}
    print(json.dumps(result))
    write("compare", result, out_path)


def stage(out_path, builds):
    result = {"repeats": REPEATS, "warmup": WARMUP, "builds": {}}
    for rnd in range(2):                                        # the builds alternate, each runs twice
        for name, lib in [("tree", "")] + builds:
            r = run_child("stage", lib)
            result["builds"].setdefault(name, []).append(r)
            print(name, rnd, json.dumps(r))
    write("stage", result, out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    default_out = os.path.join(ROOT, "profiles", "preprocess.json")
    if mode == "child" and sys.argv[2] == "compare":
        child_compare(sys.argv[3], sys.argv[4] or None)
    elif mode == "child" and sys.argv[2] == "stage":
        child_stage(sys.argv[3] or None)
    elif mode == "compare":
        compare(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else default_out)
    elif mode == "stage":
        rest = sys.argv[2:]
        out = rest.pop(0) if rest and "=" not in rest[0] else default_out
        stage(out, [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in rest])
    else:
        raise SystemExit(__doc__)
