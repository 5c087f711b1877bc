"""Where the chain balance cuts the tile work, read from the host-only plan query (Cascade.plan_tiles(tile_split=...)), and
the cells of tests/test_gpu_tile_cut.py: each names a regime of the cut ("the lead of a group is cut while its members keep
every row"), a split that lands in it is searched through the query, and tests/test_tile_cut_cpu.py asserts that every cell
still finds one — nothing here restates the planner's rounding rule.

A call of 5 .. 7 frames caps its split at 0.5 (vj_env::split_for), so the cells that need a deeper cut run 8 frames."""
import math

import numpy as np

W, H = 310, 230
# fractions tried inside the scale a cell cuts, the middle first
FRACTIONS = [0.5, 0.4, 0.6, 0.3, 0.7, 0.25, 0.75, 0.2, 0.8, 0.15, 0.85, 0.1, 0.9, 0.05, 0.95, 0.35, 0.65, 0.45, 0.55]


def f32(x) -> float:
    """the split as the library holds it"""
    return float(np.float32(x))


def split_text(x) -> str:
    """... and as vj_env_configure reads it back to the same float"""
    return f"{np.float32(x):.9g}"


def tile_scales(tiles):
    return [t for t in tiles if t.lds_class >= 0]


def by_idx(tiles):
    return {t.scale_idx: t for t in tiles}


def lead_of(tiles, t):
    return by_idx(tiles)[t.lead_scale_idx]


def groups(tiles):
    """the scale groups of the tile list, smallest scale first, each a list of members with its lead last"""
    out = {}
    for t in tile_scales(tiles):
        out.setdefault(t.lead_scale_idx, []).append(t)
    return [out[k] for k in sorted(out)]


def partial(t):
    return 0 < t.tile_row_end < t.ny


def tile_windows(tiles):
    return sum(t.nx * t.tile_row_end for t in tile_scales(tiles))


def expected_class_tiles(info, tiles):
    """tiles per frame of each class launch: per group, the union of its members' tile rows in the lead's shape"""
    want = [0] * 4
    for g in groups(tiles):
        lead = g[-1]
        want[lead.lds_class] += (math.ceil(max(m.tile_row_end for m in g) / lead.tile_h) *
                                 math.ceil(max(m.nx for m in g) / lead.tile_w))
    return want


# ----------------------------------------------------------------------------- the regimes
# (selector, condition): the selector picks the scale the cut falls into from the plan at split 0, the condition is what the
# plan at the chosen split must show.  Groups are counted from the largest scales down and hold more than one member.
def _multi(tiles):
    return [g for g in reversed(groups(tiles)) if len(g) > 1]


def sel_height(h, cls=None):
    """the largest tile scale whose tiles are h rows high (its lead's shape) [and of LDS class cls]"""
    def pick(tiles):
        return next(t for t in reversed(tile_scales(tiles))
                    if lead_of(tiles, t).tile_h == h and (cls is None or lead_of(tiles, t).lds_class == cls))
    return pick


def sel_class(cls):
    """the largest tile scale of LDS class cls that stands alone or leads its group"""
    return lambda tiles: next(t for t in reversed(tile_scales(tiles)) if t.lds_class == cls and t.lead_scale_idx == t.scale_idx)


def sel_lead(g):
    return lambda tiles: _multi(tiles)[g][-1]


def sel_member(g, back):
    """member `back` places in front of the lead of group g (-1: the group's first member)"""
    return lambda tiles: _multi(tiles)[g][0] if back < 0 else _multi(tiles)[g][-1 - back]


def cond_partial(tiles, t):
    return partial(t)


def cond_one_row(tiles, t):
    return partial(t) and t.tile_row_end == lead_of(tiles, t).tile_h


def cond_several_rows(tiles, t):
    return partial(t) and t.tile_row_end >= 2 * lead_of(tiles, t).tile_h


def cond_zero_rows(tiles, t):
    """the scale keeps some rows by the balance (the next tile scale down is untouched) and none of them is a whole tile row"""
    below = [s for s in tile_scales(tiles) if s.scale_idx < t.scale_idx]
    return t.tile_row_end == 0 and (not below or below[-1].tile_row_end == below[-1].ny)


def cond_lead_cut(tiles, t):
    g = next(g for g in groups(tiles) if g[-1].scale_idx == t.scale_idx)
    return len(g) > 1 and partial(t) and all(m.tile_row_end == m.ny for m in g[:-1])


def cond_lead_gone(tiles, t):
    """t is cut, every member after it (the lead among them) has left the tiles, those in front of it keep every row"""
    g = next(g for g in groups(tiles) if any(m.scale_idx == t.scale_idx for m in g))
    i = [m.scale_idx for m in g].index(t.scale_idx)
    return (i < len(g) - 1 and partial(t) and all(m.tile_row_end == 0 for m in g[i + 1:]) and
            all(m.tile_row_end == m.ny for m in g[:i]))


def find_split(c, n_frames, select, cond, flags=0):
    """(split, info, tiles): the first split inside the selected scale whose plan meets the condition"""
    _, base = c.plan_tiles(W, H, n_frames, flags=flags, tile_split=0.0)
    target = select(base)
    above = sum(1 for t in tile_scales(base) if t.scale_idx > target.scale_idx)
    for f in FRACTIONS:
        split = f32(above + f)
        info, tiles = c.plan_tiles(W, H, n_frames, flags=flags, tile_split=split)
        if cond(tiles, by_idx(tiles)[target.scale_idx]):
            return split, info, tiles
    raise AssertionError(f"no split inside scale {target.scale_idx} meets {cond.__name__}")


def whole_split(c, n_frames, n, flags=0):
    """(split, info, tiles) of a whole number of scales: no scale is partial, the n largest tile scales have left"""
    split = f32(n)
    info, tiles = c.plan_tiles(W, H, n_frames, flags=flags, tile_split=split)
    ts = tile_scales(tiles)
    assert not any(partial(t) for t in ts), n
    assert [t.tile_row_end for t in ts] == [t.ny for t in ts[:max(0, len(ts) - n)]] + [0] * min(n, len(ts)), n
    return split, info, tiles


# frontalface_alt, 8 frames (the comments: where the shipped planner puts the cell)
REGIMES = {
    "h24_one_row": (sel_height(24), cond_one_row),                      # scale 13
    "h24_zero_rows": (sel_height(24), cond_zero_rows),                  # scale 13: rows stay by the balance, no whole tile row
    "h28_class1": (sel_height(28, 1), cond_partial),                    # scale 11
    "h20_one_row": (sel_height(20), cond_one_row),                      # scale 9
    "h20_several_rows": (sel_height(20), cond_several_rows),            # scale 9
    "h28_class0": (sel_height(28, 0), cond_partial),                    # scale 8
    "lead_cut_upper_group": (sel_lead(0), cond_lead_cut),               # lead 7 of 4..7 cut, 4..6 whole
    "lead_gone_upper_group": (sel_member(0, 1), cond_lead_gone),        # 7 gone, 6 cut, 4 and 5 whole
    "first_member_alone_upper_group": (sel_member(0, -1), cond_lead_gone),   # only scale 4 of 4..7 left, and cut
    "lead_cut_lower_group": (sel_lead(1), cond_lead_cut),               # lead 3 of 0..3 cut
    "lead_gone_lower_group": (sel_member(1, 1), cond_lead_gone),        # 3 gone, 2 cut
    "first_member_alone_lower_group": (sel_member(1, -1), cond_lead_gone),   # scale 0 cut alone
}
WHOLE = (1, 4, 8, 10)
# the subset that the other batch sizes, the tunables and the skip list run (a plan of another batch size has other scales on
# tiles: the cut that rounds to no tile row is looked for in its largest tile scale, whatever that one's height)
SUBSET = {
    "h20": (sel_height(20), cond_partial),
    "lead_gone_upper_group": REGIMES["lead_gone_upper_group"],
    "lead_gone_lower_group": REGIMES["lead_gone_lower_group"],
    "top_zero_rows": (lambda tiles: tile_scales(tiles)[-1], cond_zero_rows),
}
# two-node trees and the stage tree
TREE_REGIMES = {
    "class0": (sel_class(0), cond_partial),
    "class1": (sel_class(1), cond_partial),
    "lead_gone": (sel_member(0, 1), cond_lead_gone),
}
# VJ_TILE_GROUP=1: every scale is its own lead and is cut in its own height; =8: one long group
GROUP1_REGIMES = {
    "h28_own": (sel_height(28, 0), cond_partial),
    "h20_own": (sel_height(20), cond_partial),
    "h32_smallest": (lambda tiles: tile_scales(tiles)[0], cond_partial),
}
GROUP8_REGIMES = {
    "lead_cut": (sel_lead(0), cond_lead_cut),
    "lead_gone": (sel_member(0, 1), cond_lead_gone),
    "first_member_alone": (sel_member(0, -1), cond_lead_gone),
}
