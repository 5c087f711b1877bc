"""By-hand measurement of vj_paint_yuv (run on the GPU box; not collected by pytest):
    python tests/measure_paint_yuv.py [out.json]
Workload: §4.20's — 64 device-resident frames of 1920 x 1080, as NV12, 16 regions of about 300 x 300 on each (1024 regions).  Modes:
FILL; OUTLINE with t = 3; PIXELATE with s = 8 and 32; BLUR with kk = 15, 31 and 61; BLUR 31 with the ellipse.  Two sides per mode,
in one process: "direct", the new call (vj_paint_yuv_timing), and "route", the parent's way — yuv_to_bgr + paint + bgr_to_yuv, the
sum of the three calls' device times by the library's events (vj_yuv_timing, vj_paint_timing, vj_yuv_timing).  Each timing is the
median of nine calls after two warm-ups; every side runs twice (the A/A pair) and the two sides alternate.  Painting is in place: a
later call blurs what an earlier one left, which changes no address and no count, so the frames are not restored between calls.
Bytes a side must move: direct — the painted bytes (the unions of the luma and of the chroma painted sets) read once and written
once, FILL and OUTLINE written only; route — the same for its 3-byte pixels plus the two conversions (each reads 1.5 and writes 3
bytes per pixel or the reverse), against the 8 TB/s HBM peak.  Device memory beside the frames: direct — the scratch; route — the BGR
copy, the second NV12 batch and paint's scratch."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

import paint_cases as pcs  # noqa: E402
import paint_yuv_cases as pyc  # noqa: E402
from measure_equalize import H_HD, N_HD, W_HD, hd_batch, write  # noqa: E402
from measure_extract import regions  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP  # noqa: E402

MODES = [("fill", dict(mode="fill", fill=(0, 0, 255))), ("outline_3", dict(mode="outline", size=3, fill=(0, 0, 255))),
         ("pixelate_8", dict(mode="pixelate", size=8)), ("pixelate_32", dict(mode="pixelate", size=32)),
         ("blur_15", dict(mode="blur", size=15)), ("blur_31", dict(mode="blur", size=31)), ("blur_61", dict(mode="blur", size=61)),
         ("blur_31_ellipse", dict(mode="blur", size=31, ellipse=True))]


def painted_samples(rects, kw):
    """(luma pixels, chroma samples) of the unions of the painted sets, over all frames."""
    mode = pcs.MODES[kw["mode"]]
    luma = chroma = 0
    for f in range(N_HD):
        mask = np.zeros((H_HD, W_HD), bool)
        cmask = np.zeros((H_HD // 2, W_HD // 2), bool)
        for _, x, y, w, h in rects[rects[:, 0] == f]:
            m = (int(x), int(y), int(w), int(h))
            k = pcs.clip(m, W_HD, H_HD)
            if k is not None:
                full = pyc.luma_mask(mode, m, k, pcs.size_of(mode, m[2], m[3], kw.get("size", 0), 0.25), kw.get("ellipse", False), W_HD, H_HD)
                mask |= full
                cmask |= pyc.chroma_mask(full)
        luma += int(mask.sum())
        chroma += int(cmask.sum())
    return luma, chroma


def main(out_path):
    import torch
    from clfacedetection_amd import Environment
    env = Environment(0)
    bgr0, keep = hd_batch("noise", 3)
    yuv = env.bgr_to_yuv(bgr0, "nv12")
    del bgr0, keep
    torch.cuda.empty_cache()
    rects = regions()
    frame_px = N_HD * W_HD * H_HD
    bgr_buf = torch.empty(env.yuv_to_bgr_layout(yuv)[1], dtype=torch.uint8, device="cuda")
    yuv_buf = torch.empty(env.bgr_to_yuv_layout(env.yuv_to_bgr(yuv, out=bgr_buf)[0], "nv12")[1], dtype=torch.uint8, device="cuda")
    med = lambda xs: round(statistics.median(xs), 4)

    def direct(kw):
        env.paint_yuv(yuv, rects, **kw)
        return env.paint_yuv_timing()

    def route(kw):
        bgr = env.yuv_to_bgr(yuv, out=bgr_buf)
        ms = env.yuv_timing()
        env.paint(bgr, rects, **kw)
        ms += env.paint_timing()
        env.bgr_to_yuv(bgr[0], "nv12", out=yuv_buf)
        return ms + env.yuv_timing()

    times = {name: {"direct": [], "route": []} for name, _ in MODES}
    for _ in range(2):                                          # the A/A pair; the two sides alternate
        for name, kw in MODES:
            for side, fn in (("direct", direct), ("route", route)):
                t = [fn(kw) for _ in range(WARMUP + REPEATS)][WARMUP:]
                times[name][side].append(med(t))
            print(name, times[name], flush=True)
    result = {"device": env.device_name, "repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD, "nv12"], "regions": len(rects),
              "frames_bytes": frame_px * 3 // 2, "route_extra_device_bytes": int(bgr_buf.numel() + yuv_buf.numel()), "modes": {}}
    for name, kw in MODES:
        luma, chroma = painted_samples(rects, kw)
        rw = 1 if kw["mode"] in ("fill", "outline") else 2
        d_bytes = rw * (luma + 2 * chroma)
        r_bytes = rw * 3 * luma + 2 * (frame_px * 3 // 2 + frame_px * 3)
        row = {"painted_luma": luma, "painted_chroma": chroma}
        for side, nbytes in (("direct", d_bytes), ("route", r_bytes)):
            pair = times[name][side]
            ms = statistics.mean(pair)
            row[side] = {"ms": pair, "aa_spread_ms": round(abs(pair[0] - pair[1]), 4), "bytes": nbytes, "tb_per_s": round(nbytes / ms / 1e9, 3),
                         "fraction_of_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}
        lk = dict(size=kw.get("size", 0))
        row["direct"]["scratch_bytes"] = env.paint_yuv_layout(yuv, rects, kw["mode"], **lk)[4]
        row["route"]["scratch_bytes"] = env.paint_layout(env.yuv_to_bgr(yuv, out=bgr_buf), rects, kw["mode"], **lk)[2]
        spread = max(row["direct"]["aa_spread_ms"], row["route"]["aa_spread_ms"])
        excess = statistics.mean(times[name]["direct"]) - statistics.mean(times[name]["route"])
        row["direct_over_route"] = round(statistics.mean(times[name]["direct"]) / statistics.mean(times[name]["route"]), 3)
        row["condition_holds"] = bool(excess <= spread)          # direct must not exceed route by more than the larger A/A spread
        result["modes"][name] = row
    env.close()
    print(json.dumps(result))
    write("call", result, out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "paint_yuv.json"))
