"""How the tile kernel's dense sweep groups its chunks in stages 0-2 (sweep_stages<..., MULTI>).  Host only:
no GPU needed.  Reads the tile shapes of a plan (Cascade.plan_tiles) and the survival rates of tests/golden/fullsize.json
(config3.stage_entered), deals every tile's windows to its eight waves as the kernel does (whole chunks, the first n_chunks % 8
waves one more, windows outside the grid dropped), thins every wave by the fixture's rate after stage 0 and re-packs the tile's
survivors before stage 2 (shares of 64 * ceil(chunks / 8)), and counts per stage and lead shape the chunk x stump steps that run in
groups of 4, 3 and 2 and as lone chunks, and how full the lone chunks are — for the ladder up to round 15 (4, 2, lone) and the
present one (4, 3, 2, lone).  The rates are the batch's, over all scales: per scale and per tile they differ, so this is an
estimate of the shares, not an account of one launch.
Usage:  python tools/chunk_groups.py [CASCADE:WxH:FRAMES] [--tile-split S]   (default: the bench workload at the shipped balance)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clfacedetection_amd import Cascade


def ladder(n, three):
    """the chunk groups a wave with n entries sweeps a stage in"""
    g, base = [], 0
    while base + 192 < n:
        g.append(4)
        base += 256
    if three and base + 128 < n:
        g.append(3)
        base += 192
    elif base + 64 < n:
        g.append(2)
        base += 128
    if base < n:
        g.append(1)
    return g, (n - base if base < n else 0)


def wave_counts(t, lead):
    """per tile of member t: the eight waves' entries at stage 0"""
    tw, th = lead.tile_w, lead.tile_h
    n_tile = tw * th
    c_base, c_extra = divmod((n_tile + 63) // 64, 8)
    for iy0 in range(0, t.tile_row_end, th):
        rows = min(th, t.ny - iy0)
        for ix0 in range(0, t.nx, tw):
            cols = min(tw, t.nx - ix0)
            waves = []
            for w in range(8):
                b = min((w * c_base + min(w, c_extra)) * 64, n_tile)
                e = min(b + (c_base + (1 if w < c_extra else 0)) * 64, n_tile)
                # tile-local indices [b, e) whose row is below `rows` and whose column is below `cols`
                n = 0
                for ty in range(b // tw, min((e + tw - 1) // tw, rows)):
                    lo, hi = max(b, ty * tw), min(e, ty * tw + cols)
                    n += max(0, hi - lo)
                waves.append(n)
            yield waves


def shares(total):
    s = 64 * (((total + 63) // 64 + 7) // 8)
    return [min(s, total - min(w * s, total)) for w in range(8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("spec", nargs="?", default="frontalface_alt:1920x1080:64")
    ap.add_argument("--tile-split", type=float, default=None)
    args = ap.parse_args()
    name, size, frames = args.spec.split(":")
    W, H = (int(v) for v in size.split("x"))
    c = Cascade.load(name)
    entered = json.load(open(os.path.join(ROOT, "tests", "golden", "fullsize.json")))["config3"]["stage_entered"]
    rate = [entered[1] / entered[0], entered[2] / entered[1]]
    stumps = [int(s["n_trees"]) for s in c.stages[:3]]
    _, tiles = c.plan_tiles(W, H, int(frames), tile_split=args.tile_split)
    by_idx = {t.scale_idx: t for t in tiles}
    print(f"{name} {W}x{H}, {frames} frames per call, tile_split {'shipped' if args.tile_split is None else args.tile_split}: stumps of stages 0-2 "
          f"{stumps}, survival after stage 0 {rate[0]:.3f}, after stage 1 {rate[1]:.3f}")
    # acc[three][(lead shape, stage)] = [steps in groups of 4, of 3, of 2, lone, lone chunks, entries in lone chunks]
    acc = [{}, {}]
    for t in tiles:
        if t.tile_w == 0 or t.tile_row_end == 0:
            continue
        lead = by_idx[t.lead_scale_idx]
        shape = (t.lds_class, lead.tile_w, lead.tile_h)
        for waves in wave_counts(t, lead):
            per_stage = [waves, [round(n * rate[0]) for n in waves]]
            per_stage.append(shares(round(sum(per_stage[1]) * rate[1])))
            for st, counts in enumerate(per_stage):
                for three in (0, 1):
                    a = acc[three].setdefault((shape, st), [0] * 6)
                    for n in counts:
                        groups, lone = ladder(n, bool(three))
                        for g in groups:
                            a[{4: 0, 3: 1, 2: 2, 1: 3}[g]] += g * stumps[st]
                        if lone:
                            a[4] += 1
                            a[5] += lone
    for three, title in ((0, "ladder 4, 2, lone (up to round 15)"), (1, "ladder 4, 3, 2, lone")):
        print(f"\n== {title}: chunk x stump steps per frame, per LDS class and lead shape and stage")
        print("class shape   stage |   groups of 4   groups of 3   groups of 2    lone chunks | lone share | mean entries of a lone chunk")
        tot = [0] * 6
        tot_class = {}
        for (shape, st), a in sorted(acc[three].items()):
            steps = sum(a[:4])
            print(f"  c{shape[0]}  {shape[1]:2d}x{shape[2]:2d}    {st}   | {a[0]:13d} {a[1]:13d} {a[2]:13d} {a[3]:14d} |   {100.0 * a[3] / max(steps, 1):5.1f} %  | {a[5] / max(a[4], 1):5.1f}")
            tot = [x + y for x, y in zip(tot, a)]
            k = tot_class.setdefault(shape[0], [0] * 6)
            tot_class[shape[0]] = [x + y for x, y in zip(k, a)]
        for cls, a in sorted(tot_class.items()):
            print(f"  class {cls}, stages 0-2: lone {100.0 * a[3] / max(sum(a[:4]), 1):.1f} %, groups of 2 {100.0 * a[2] / max(sum(a[:4]), 1):.1f} %, "
                  f"of 3 {100.0 * a[1] / max(sum(a[:4]), 1):.1f} %, of 4 {100.0 * a[0] / max(sum(a[:4]), 1):.1f} %; mean lone chunk {a[5] / max(a[4], 1):.1f} entries")
        steps = sum(tot[:4])
        print(f"  all tile scales, stages 0-2: {steps} steps; lone {100.0 * tot[3] / steps:.1f} %, groups of 2 {100.0 * tot[2] / steps:.1f} %, "
              f"of 3 {100.0 * tot[1] / steps:.1f} %, of 4 {100.0 * tot[0] / steps:.1f} %; mean lone chunk {tot[5] / max(tot[4], 1):.1f} entries")


if __name__ == "__main__":
    main()
