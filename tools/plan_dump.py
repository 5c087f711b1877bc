"""Tile shapes of a plan, before and after the tiles grew into the LDS of the former stump-parallel finish (round 11).
Host only: no GPU needed.  Per tile scale: the shape, pitch, rows, LDS class and staged dwords per window, with the
former budget (VJ_PLAN_TILES_FORMER_SHAPES) and with the shipped one.
Usage:  python tools/plan_dump.py [CASCADE:WxH:FRAMES ...]   (default: the bench workload and config 5's two cascades)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clfacedetection_amd import Cascade
from clfacedetection_amd.api import VJ_PLAN_TILES_FORMER_SHAPES

DEFAULT = ["frontalface_alt:1920x1080:64", "frontalface_alt2:1280x720:64", "eye:1280x720:64"]


def fmt(t):
    if t.lds_class < 0:
        return "gather chain".ljust(44)
    nw = t.tile_w * t.tile_h
    return f"c{t.lds_class} {t.tile_w:2d}x{t.tile_h:2d}={nw:4d} pitch {t.pitch:3d} rows {t.rows:3d} {t.pitch * t.rows * 4:6d} B {t.pitch * t.rows / nw:5.2f} dw/win"


def staged_per_frame(tiles):
    """dwords the frame's tile list stages for one frame: a group stages once, in its lead's shape"""
    by_idx = {t.scale_idx: t for t in tiles}
    total, seen = 0, set()
    for t in tiles:
        if t.lds_class < 0 or t.lead_scale_idx in seen:
            continue
        seen.add(t.lead_scale_idx)
        L = by_idx[t.lead_scale_idx]
        members = [m for m in tiles if m.lds_class >= 0 and m.lead_scale_idx == L.scale_idx]
        nx, rows = max(m.nx for m in members), max(m.tile_row_end for m in members)
        total += -(-nx // L.tile_w) * -(-rows // L.tile_h) * L.pitch * L.rows
    return total


def dump(spec):
    name, size, frames = spec.split(":")
    W, H = (int(v) for v in size.split("x"))
    c = Cascade.load(name)
    i0, old = c.plan_tiles(W, H, int(frames), flags=VJ_PLAN_TILES_FORMER_SHAPES)
    i1, new = c.plan_tiles(W, H, int(frames))
    print(f"== {name} {W}x{H}, {frames} frames: header {i1.header_bytes} B, class blocks {list(i0.class_lds)[:i0.n_classes]} -> "
          f"{list(i1.class_lds)[:i1.n_classes]} B, tiles per frame {list(i0.class_tiles)[:i0.n_classes]} -> {list(i1.class_tiles)[:i1.n_classes]}")
    for a, b in zip(old, new):
        if a.lds_class < 0 and b.lds_class < 0:
            continue
        same = (a.lds_class, a.tile_w, a.tile_h, a.lead_scale_idx) == (b.lds_class, b.tile_w, b.tile_h, b.lead_scale_idx)
        print(f"scale {a.scale_idx:2d} s={a.scale:5.3f} grid {a.nx:4d}x{a.ny:4d} lead {a.lead_scale_idx:2d}->{b.lead_scale_idx:2d} rows<{b.tile_row_end:4d} | "
              f"{fmt(a)} | {fmt(b)}{'' if same else '  *'}")
    s0, s1 = staged_per_frame(old), staged_per_frame(new)
    print(f"staged dwords per frame (tile list): {s0} -> {s1} ({(s1 - s0) / max(s0, 1) * 100:+.1f} %)")


if __name__ == "__main__":
    for spec in sys.argv[1:] or DEFAULT:
        dump(spec)
