"""By-hand measurement of vj_extract (run on the GPU box; not collected by pytest):
    python tests/measure_extract.py call [out.json] [NAME=LIB ...]      the call itself, for this tree's library and other builds of it
    python tests/measure_extract.py compare PARENT_LIB [out.json]       the parent's way on the parent's library against extract()
Workload: 64 device-resident BGR frames of 1920 x 1080, 16 regions of about 300 x 300 on each (280 .. 320 on a side, some across the
frame's border), to 112 x 112.
`call`: the device time of one extract() call by the library's events (vj_extract_timing: around its copy of the records and taps and
the launch), median of nine after two warm-ups, twice (the A/A pair), interleaved, planar and to gray; and the same regions made
exactly 224 x 224 (the 2 x 2 mean) and 112 x 112 (the copy), in colour and from gray frames (the wide loads).  Bytes a call must
move: the distinct source pixels the crops cover, once, plus the output, once; against the 8 TB/s HBM peak.  NAME=LIB: the same in a
process that binds LIB — a build of csrc/vj_extract.hip with -DEXTRACT_BYTE_STORES; the builds alternate, each runs twice.
`compare`: what a caller had before — download the frames, crop and resize on the host with the restatement's arithmetic
(tests/extract_cases.py) — on the parent's library against extract() on this tree's; every side in a process of its own, the sides
alternate, each runs twice, a time is the median wall time of nine calls after two warm-ups (the parent's side: three after one,
it takes seconds), and the bytes are compared by hash.  The ratio describes what the call replaces; it is no gate."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

from measure_equalize import H_HD, N_HD, W_HD, hd_batch, write  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP, use_library  # noqa: E402

SIZE = (112, 112)
PER_FRAME = 16


def regions(side=None):
    """16 regions per frame; side: every region exactly side x side and inside its frame (the mean and the copy)."""
    rng = np.random.default_rng(17)
    rows = []
    for f in range(N_HD):
        for _ in range(PER_FRAME):
            w, h = (side, side) if side else (int(rng.integers(280, 321)), int(rng.integers(280, 321)))
            lo = 0 if side else -40
            rows.append((f, int(rng.integers(lo, W_HD - w - lo + 1)), int(rng.integers(lo, H_HD - h - lo + 1)), w, h))
    return np.array(rows, np.int32)


def must_move(rects, src_channels, out_bytes):
    """The distinct source pixels the crops cover (clipped to the frame), once, plus the output, once."""
    px = 0
    for f in range(N_HD):
        mask = np.zeros((H_HD, W_HD), bool)
        for _, x, y, w, h in rects[rects[:, 0] == f]:
            mask[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
        px += int(mask.sum())
    return px * src_channels + out_bytes


def child_call(lib_path):
    import torch
    if lib_path:
        use_library(lib_path)
    from clfacedetection_amd import Environment
    env = Environment(0)
    out = {"device": env.device_name, "cases": {}}
    med = lambda xs: round(statistics.median(xs), 4)

    def measure(name, frames, ch, rects, **kw):
        _, c, nbytes = env.extract_layout(frames, rects, SIZE, **kw)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        moved = must_move(rects, ch, nbytes)
        pairs = []
        for _ in range(2):                                  # the A/A pair
            t = []
            for k in range(WARMUP + REPEATS):
                env.extract(frames, rects, SIZE, out=buf, **kw)
                if k >= WARMUP:
                    t.append(env.extract_timing())
            pairs.append(med(t))
        ms = statistics.mean(pairs)
        out["cases"][name] = {"ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4), "regions": len(rects), "bytes": moved,
                              "tb_per_s": round(moved / ms / 1e9, 3), "fraction_of_hbm_peak": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4),
                              "hash": hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()[:16]}

    for ch, label in ((3, "bgr"), (1, "gray_source")):
        d, keep = hd_batch("noise", ch)
        if ch == 3:
            measure("bgr_interleaved", d, ch, regions())
            measure("bgr_planar", d, ch, regions(), planar=True)
            measure("bgr_to_gray", d, ch, regions(), gray=True)
        else:
            measure("gray_source_bilinear", d, ch, regions())
        measure(f"{label}_mean_224", d, ch, regions(224))
        measure(f"{label}_copy_112", d, ch, regions(112))
        del d, keep
    env.close()
    print("RESULT " + json.dumps(out))


def child_compare(side, lib_path):
    import torch
    if lib_path:
        use_library(lib_path)
    import extract_cases as ec
    from clfacedetection_amd import Environment
    from oracle.oracle import Oracle
    env = Environment(0)
    d, keep = hd_batch("noise", 3)
    rects = regions()
    if side == "parent":
        oracle = Oracle()
        fn = lambda: ec.restate(oracle, keep.cpu().numpy(), rects, SIZE)
        warm, reps = 1, 3
    else:
        fn = lambda: env.extract(d, rects, SIZE)
        warm, reps = WARMUP, REPEATS
    for _ in range(warm):
        res = fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    host = res if isinstance(res, np.ndarray) else res.cpu().numpy()
    env.close()
    print("RESULT " + json.dumps({"side": side, "median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3),
                                  "hash": hashlib.sha256(np.ascontiguousarray(host).tobytes()).hexdigest()[:16]}))


def run_child(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *args], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def call(out_path, builds):
    result = {"repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD], "regions_per_frame": PER_FRAME, "to": list(SIZE), "builds": {}}
    for rnd in range(2):                                        # the builds alternate, each runs twice
        for name, lib in [("tree", "")] + builds:
            r = run_child("call", lib)
            result["builds"].setdefault(name, []).append(r)
            print(name, rnd, json.dumps(r), flush=True)
    hashes = {k: {b: [x["cases"][k]["hash"] for x in runs] for b, runs in result["builds"].items()} for k in result["builds"]["tree"][0]["cases"]}
    assert all(len({h for hs in v.values() for h in hs}) == 1 for v in hashes.values()), hashes     # every build writes the same bytes
    write("call", result, out_path)


def compare(parent_lib, out_path):
    runs = [run_child("compare", s, lib) for s, lib in (("parent", parent_lib), ("extract", ""), ("parent", parent_lib), ("extract", ""))]
    print(json.dumps(runs), flush=True)
    assert len({x["hash"] for x in runs}) == 1, runs            # the same bytes
    parent, ext = [runs[0]["median"], runs[2]["median"]], [runs[1]["median"], runs[3]["median"]]
    result = {"frames": [N_HD, W_HD, H_HD, 3], "regions": N_HD * PER_FRAME, "to": list(SIZE), "parent_ms": parent, "extract_ms": ext,
              "aa_spread_ms": [round(abs(parent[0] - parent[1]), 3), round(abs(ext[0] - ext[1]), 3)],
              "parent_over_extract": round(statistics.mean(parent) / statistics.mean(ext), 1)}
    print(json.dumps(result))
    write("compare", result, out_path)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    default_out = os.path.join(ROOT, "profiles", "extract.json")
    if mode == "child" and sys.argv[2] == "call":
        child_call(sys.argv[3] or None)
    elif mode == "child" and sys.argv[2] == "compare":
        child_compare(sys.argv[3], sys.argv[4] or None)
    elif mode == "call":
        rest = sys.argv[2:]
        out = rest.pop(0) if rest and "=" not in rest[0] else default_out
        call(out, [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in rest])
    elif mode == "compare":
        compare(os.path.abspath(sys.argv[2]), sys.argv[3] if len(sys.argv) > 3 else default_out)
    else:
        raise SystemExit(__doc__)
