"""By-hand measurement of vj_extract_yuv / vj_extract_affine_yuv (run on the GPU box; not collected by pytest):
    python tests/measure_extract_yuv.py [out.json]
Workload: §4.17's — 64 device-resident frames of 1920 x 1080, as NV12 and as I420, and 1024 regions of about 300 x 300 to 112 x 112.
Rows: BGR interleaved, BGR planar, BGRA, gray; exact 224 x 224 regions (the mean) and exact 112 x 112 regions (the copy); the affine call
on affine_from_rect of the same boxes; a sparse row, the same 64 frames with 16 regions in all, on 4 of the frames.  Two sides per
row, in one process: "direct", the new call (vj_extract_yuv_timing), and "route", the parent's way — yuv_to_bgr of all 64 frames
plus extract (or extract_affine), the sum of the calls' device times by the library's events.  For the sparse row the route is also
measured with only the 4 named frames converted ("route_picked": the best the parent can do).  Each timing is the median of nine
calls after two warm-ups; every side runs twice (the A/A pair) and the sides alternate.
Bytes a side must move: direct — the distinct Y and chroma bytes under the crops (clipped to the frame) once plus the output once;
route — the conversion's 1.5 bytes read and 3 (BGRA: 4) written per pixel of every converted frame, plus the distinct BGR bytes under
the crops and the output; against the 8 TB/s HBM peak.  Device memory beside the frames: direct 0; route the BGR copy."""
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

from measure_equalize import H_HD, N_HD, W_HD, hd_batch, write  # noqa: E402
from measure_extract import regions  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP  # noqa: E402

SIZE = (112, 112)
ROWS = [("bgr", None, dict()), ("bgr_planar", None, dict(planar=True)), ("bgra", None, dict(alpha=True)), ("gray", None, dict(gray=True)),
        ("mean_224", 224, dict()), ("copy_112", 112, dict()), ("affine", None, dict()), ("sparse", None, dict())]


def covered(rects):
    """(distinct luma pixels, distinct chroma samples) under the crops, clipped to the frames."""
    luma = chroma = 0
    for f in np.unique(rects[:, 0]):
        mask = np.zeros((H_HD, W_HD), bool)
        for _, x, y, w, h in rects[rects[:, 0] == f]:
            mask[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
        luma += int(mask.sum())
        chroma += int((mask[0::2, 0::2] | mask[0::2, 1::2] | mask[1::2, 0::2] | mask[1::2, 1::2]).sum())
    return luma, chroma


def main(out_path):
    import torch
    from clfacedetection_amd import Environment, affine_from_rect
    env = Environment(0)
    bgr0, keep = hd_batch("noise", 3)
    sources = {"nv12": env.bgr_to_yuv(bgr0, "nv12"), "i420": env.bgr_to_yuv(bgr0, "i420")}
    del bgr0, keep
    torch.cuda.empty_cache()
    frame_px = N_HD * W_HD * H_HD
    bgr_buf = torch.empty(env.yuv_to_bgr_layout(sources["nv12"], alpha=True)[1], dtype=torch.uint8, device="cuda")
    med = lambda xs: round(statistics.median(xs), 4)
    sparse = regions()[[0, 1, 2, 3, 16 * 20, 16 * 20 + 1, 16 * 20 + 2, 16 * 20 + 3, 16 * 40, 16 * 40 + 1, 16 * 40 + 2, 16 * 40 + 3, 16 * 63, 16 * 63 + 1,
                        16 * 63 + 2, 16 * 63 + 3]]
    assert sorted(set(sparse[:, 0].tolist())) == [0, 20, 40, 63]

    def rects_of(name, side):
        return sparse if name == "sparse" else regions(side)

    def affines_of(rects):
        return np.array([[r[0]] + list(affine_from_rect(r[1], r[2], r[3], r[4], SIZE)) for r in rects], np.float64)

    def picked(yuv, rects):
        """The frames the regions name as YuvFrames of their own, and the regions renumbered."""
        from clfacedetection_amd import YuvFrames
        named = sorted(set(rects[:, 0].tolist()))
        items = [YuvFrames(yuv.ptr_y + f * yuv.frame_bytes, yuv.ptr_c0 + f * yuv.frame_bytes, (yuv.ptr_c1 + f * yuv.frame_bytes) if yuv.ptr_c1 else 0, 1,
                           yuv.height, yuv.width, yuv.y_stride, yuv.c_stride, yuv.layout, 0, yuv.owner) for f in named]
        r = rects.copy()
        r[:, 0] = [named.index(f) for f in rects[:, 0].tolist()]
        return items, r

    def direct(yuv, name, rects, kw):
        if name == "affine":
            env.extract_affine_yuv(yuv, affines_of(rects), SIZE, **kw)
        else:
            env.extract_yuv(yuv, rects, SIZE, **kw)
        return env.extract_yuv_timing()

    def route(yuv, name, rects, kw, pick=False):
        if pick:
            yuv, rects = picked(yuv, rects)
        bgr = env.yuv_to_bgr(yuv, alpha=kw.get("alpha", False), out=bgr_buf)
        ms = env.yuv_timing()
        rkw = {k: v for k, v in kw.items() if k != "alpha"}
        if name == "affine":
            env.extract_affine(bgr, affines_of(rects), SIZE, **rkw)
            return ms + env.extract_affine_timing()
        env.extract(bgr, rects, SIZE, **rkw)
        return ms + env.extract_timing()

    result = {"device": env.device_name, "repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD], "size": list(SIZE),
              "frames_bytes": frame_px * 3 // 2, "direct_extra_device_bytes": 0, "route_extra_device_bytes": frame_px * 3, "layouts": {}}
    for lay, yuv in sources.items():
        sides = ["direct", "route"]
        times = {name: {s: [] for s in sides + (["route_picked"] if name == "sparse" else [])} for name, _, _ in ROWS}
        for _ in range(2):                                          # the A/A pair; the sides alternate
            for name, side_px, kw in ROWS:
                rects = rects_of(name, side_px)
                for s in times[name]:
                    fn = (lambda: direct(yuv, name, rects, kw)) if s == "direct" else (lambda: route(yuv, name, rects, kw, s == "route_picked"))
                    t = [fn() for _ in range(WARMUP + REPEATS)][WARMUP:]
                    times[name][s].append(med(t))
                print(lay, name, times[name], flush=True)
        rows = {}
        for name, side_px, kw in ROWS:
            rects = rects_of(name, side_px)
            luma, chroma = covered(rects)
            C = 1 if kw.get("gray") else 4 if kw.get("alpha") else 3
            bpp = 4 if kw.get("alpha") else 3
            out_bytes = len(rects) * SIZE[0] * SIZE[1] * C
            nbytes = {"direct": luma + 2 * chroma + out_bytes, "route": frame_px * 3 // 2 + frame_px * bpp + luma * bpp + out_bytes}
            if name == "sparse":
                nbytes["route_picked"] = 4 * W_HD * H_HD * 3 // 2 + 4 * W_HD * H_HD * bpp + luma * bpp + out_bytes
            row = {"regions": len(rects), "covered_luma": luma, "covered_chroma": chroma}
            for s, pair in times[name].items():
                ms = statistics.mean(pair)
                row[s] = {"ms": pair, "aa_spread_ms": round(abs(pair[0] - pair[1]), 4), "bytes": nbytes[s], "tb_per_s": round(nbytes[s] / ms / 1e9, 3),
                          "fraction_of_hbm_peak": round(nbytes[s] / ms / 1e6 / HBM_PEAK_GBS, 4)}
            spread = max(row["direct"]["aa_spread_ms"], row["route"]["aa_spread_ms"])
            d, r = statistics.mean(times[name]["direct"]), statistics.mean(times[name]["route"])
            row["direct_over_route"] = round(d / r, 3)
            row["condition_holds"] = bool(d - r <= spread)           # direct must not exceed the full route by more than the larger A/A spread
            if name == "sparse":
                row["direct_over_route_picked"] = round(d / statistics.mean(times[name]["route_picked"]), 3)
            rows[name] = row
        result["layouts"][lay] = rows
    env.close()
    print(json.dumps(result))
    write("call", result, out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "extract_yuv.json"))
