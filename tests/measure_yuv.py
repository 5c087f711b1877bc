"""By-hand measurement of vj_yuv_to_bgr / vj_bgr_to_yuv (run on the GPU box; not collected by pytest):
    python tests/measure_yuv.py [out.json]
Workload: 64 device-resident 1920 x 1080 frames of random bytes, each direction, NV12 and I420, 3 and 4 channels.  A time is the
device time of one call by the library's events (vj_yuv_timing: around its copy of the records and its launches), the median of nine
calls after two warm-ups, and every side runs twice (the A/A pair: the spread between its two medians is what a difference has to
exceed).  Bytes a call must move: 1.5 per pixel on the YUV side and 3 or 4 on the other; against the 8 TB/s HBM peak.  The yardstick
that exists without this stage, in the same run on the same frames' Y planes: preprocess() without resize or equalization —
prep_resize<false>'s copy path, one byte per pixel in and one out (vj_preprocess_timing)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (first: see conftest.py)
except Exception:
    pass

from measure_equalize import H_HD, N_HD, W_HD, write  # noqa: E402
from measure_mixed import HBM_PEAK_GBS, REPEATS, WARMUP  # noqa: E402


def main(out_path):
    import torch
    from clfacedetection_amd import DeviceFrames, Environment, YuvFrames
    env = Environment(0)
    px = N_HD * H_HD * W_HD
    result = {"device": env.device_name, "repeats": REPEATS, "warmup": WARMUP, "frames": [N_HD, W_HD, H_HD], "lane_pixels": 4, "cases": {}}
    med = lambda xs: round(statistics.median(xs), 4)

    def measure(name, call, timing, moved):
        pairs = []
        for _ in range(2):                                  # the A/A pair
            t = []
            for k in range(WARMUP + REPEATS):
                call()
                if k >= WARMUP:
                    t.append(timing())
            pairs.append(med(t))
        ms = statistics.mean(pairs)
        result["cases"][name] = {"ms": pairs, "aa_spread_ms": round(abs(pairs[0] - pairs[1]), 4), "bytes": moved,
                                 "tb_per_s": round(moved / ms / 1e9, 3), "fraction_of_hbm_peak": round(moved / ms / 1e6 / HBM_PEAK_GBS, 4)}
        print(name, json.dumps(result["cases"][name]), flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    yuv = torch.randint(0, 256, (N_HD, H_HD * 3 // 2, W_HD), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    # the yardstick: the copy path of prep_resize<false> on the Y planes
    luma = YuvFrames.from_torch(yuv).luma()
    _, nbytes = env.preprocess_layout(luma)
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    measure("preprocess_copy_of_the_y_planes", lambda: env.preprocess(luma, out=buf), env.preprocess_timing, 2 * px)
    del buf
    for layout in ("nv12", "i420"):
        frames = YuvFrames.from_torch(yuv, layout)
        for ch in (3, 4):
            _, nbytes = env.yuv_to_bgr_layout(frames, alpha=ch == 4)
            bgr = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            moved = px * 3 // 2 + px * ch
            measure(f"yuv_to_bgr_{layout}_{ch}ch", lambda: env.yuv_to_bgr(frames, alpha=ch == 4, out=bgr), env.yuv_timing, moved)
            src = DeviceFrames(bgr.data_ptr(), N_HD, H_HD, W_HD, W_HD * ch, ch, 0, bgr)       # 1920 * ch is a multiple of 4 and 1920 * 1080 * ch of 256
            assert nbytes == N_HD * H_HD * W_HD * ch
            _, nbytes = env.bgr_to_yuv_layout(src, layout=layout)
            out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            measure(f"bgr_to_yuv_{layout}_{ch}ch", lambda: env.bgr_to_yuv(src, layout=layout, out=out), env.yuv_timing, moved)
            del bgr, out, src
    base = result["cases"]["preprocess_copy_of_the_y_planes"]["fraction_of_hbm_peak"]
    for name, c in result["cases"].items():
        c["rate_over_the_copy_path"] = round(c["fraction_of_hbm_peak"] / base, 3)
    env.close()
    print(json.dumps(result))
    write("stage", result, out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "yuv.json"))
