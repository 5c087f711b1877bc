"""Windows that pass from one launch to another, against the C oracle.  A tile launch leaves at the first pass boundary at
or beyond tile_end, or earlier when fewer than tile_min_lanes windows are left in the tile, and hands its survivors to that
pass's global queue (vj_kernels.hip, tile_pass_body: flush_wave turns tile-local offsets back into image offsets); a queue
pass finishes them.  For batches of q_band_min_frames or more that queue pass may be the band-major one, which reads only
the runs the grid pass recorded in run_table; scale groups (VJ_TILE_GROUP) hand over from the group's pitch and origin.

tile_sp_begin 64 keeps a tile from finishing early, so every window that survives to the boundary is handed over.  Every
run compares rectangles, per-stage counts and windows with the oracle frame by frame, and the timed (uncounted) kernels'
rectangles with the counted ones."""
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import pytest

from cases import check_against_oracle, tunables   # (check_against_oracle: shared with test_gpu_tunable_parity.py)
from clfacedetection_amd import Environment, synth

pytestmark = pytest.mark.gpu

KINDS = ("noise", "faces", "blocks")
N_SET = 16                                   # every batch is a prefix of one set of distinct frames per size
SEED0 = {(480, 640): 4001, (479, 641): 4101}
MAIN, ODD = (480, 640), (479, 641)
CASCADES = ("frontalface_alt", "frontalface_default", "frontalface_alt2")   # stumps {0,3,22}, stumps {0,3,25}, two-node trees


@dataclass(frozen=True)
class Row:
    id: str
    pass_split: str
    tile_end: int
    tile_min_lanes: int
    q_band_px: int
    tile_sp_begin: int
    concurrent: int
    batches: tuple                           # frame counts: q_band_min_frames is 8; 11 does not divide by the 8 queue parts

    def settings(self):
        return (("pass_split", self.pass_split), ("tile_end", self.tile_end), ("tile_min_lanes", self.tile_min_lanes),
                ("q_band_px", self.q_band_px), ("tile_sp_begin", self.tile_sp_begin), ("concurrent", self.concurrent))

    def label(self, casc, size, n):
        return (f"{casc} {size[0]}x{size[1]} n={n} pass_split={self.pass_split} tile_end={self.tile_end} "
                f"tile_min_lanes={self.tile_min_lanes} q_band_px={self.q_band_px} tile_sp_begin={self.tile_sp_begin} "
                f"concurrent={self.concurrent}")

    def handover(self):
        """The pass boundary at which the tiles leave (the first one at or beyond tile_end), or None: they run to the end."""
        return next((b for b in map(int, self.pass_split.split(",")) if b >= self.tile_end), None)


# Only the rows with tile_min_lanes 0, q_band_px > 0 and two passes take the band-major queue pass on batches of >= 8 frames.
ROWS = [
    Row("s3_end2", "3", 2, 0, 128, 64, 1, (1, 8, 16)),              # below the boundary: tiles still leave at 3
    Row("s3_end3", "3", 3, 0, 128, 64, 1, (1, 7, 8, 11, 16)),       # at the boundary
    Row("s3_end3_sp3", "3", 3, 0, 128, 3, 1, (7, 8, 11)),           # ... with the shipped early finish
    Row("s3_end4", "3", 4, 0, 128, 64, 1, (7, 8, 16)),              # beyond it: tiles run the whole cascade
    Row("s3_end64", "3", 64, 0, 128, 64, 1, (1, 11)),
    Row("s3_end3_lanes64", "3", 3, 64, 128, 64, 1, (7, 16)),
    Row("s3_end64_lanes64", "3", 64, 64, 128, 3, 1, (1, 8)),        # thin tiles leave at 3, the others finish
    Row("s3_end3_chunked", "3", 3, 0, 0, 64, 1, (7, 11)),
    Row("s3_end3_serial", "3", 3, 0, 128, 64, 0, (1, 8)),           # one stream instead of the tile / gather split
    Row("s39_end3", "3,9", 3, 0, 128, 64, 1, (1, 11)),              # three passes: tiles feed pass 1
    Row("s39_end6", "3,9", 6, 0, 128, 64, 1, (7, 8, 16)),           # ... pass 2, while pass 1 runs next to the tiles
    Row("s39_end9", "3,9", 9, 0, 128, 64, 1, (1, 16)),
    Row("s39_end9_lanes64", "3,9", 9, 64, 0, 3, 1, (7, 8)),
]
ODD_ROWS = ("s3_end3", "s3_end64_lanes64", "s39_end6")
ODD_BATCHES = (7, 8, 11)

CELLS = [pytest.param(casc, MAIN, row, n, id=f"{casc}-{MAIN[0]}x{MAIN[1]}-{row.id}-n{n}")
         for casc in CASCADES for row in ROWS for n in row.batches]
CELLS += [pytest.param(casc, ODD, row, n, id=f"{casc}-{ODD[0]}x{ODD[1]}-{row.id}-n{n}")
          for casc in CASCADES for row in ROWS if row.id in ODD_ROWS for n in ODD_BATCHES]

_FRAMES = {}
_ORACLE = {}


def frame_set(size):
    if size not in _FRAMES:
        _FRAMES[size] = synth.batch(N_SET, size[0], size[1], seed0=SEED0[size], kinds=KINDS)
    return _FRAMES[size]


def oracle_set(oracle, cascades, casc, size):
    """[(rects, stats)] of the oracle for every frame of the set, computed once per module (the C entry point releases
    the GIL, so the frames run side by side)."""
    key = (casc, size)
    if key not in _ORACLE:
        _, a = cascades(casc)
        f = frame_set(size)
        with ThreadPoolExecutor(8) as ex:
            _ORACLE[key] = list(ex.map(lambda i: oracle.detect(a, f[i]), range(N_SET)))
    return _ORACLE[key]


def tile_counts(r, n_st):
    tiles = [l for l in r.launches if l["kind"] == "tile"]
    return tiles, [sum(l["stage_entered"][s] for l in tiles) for s in range(n_st)]


@pytest.mark.parametrize("casc,size,row,n", CELLS)
def test_tile_handoff_matches_the_oracle(env, oracle, cascades, casc, size, row, n):
    c, _ = cascades(casc)
    want = oracle_set(oracle, cascades, casc, size)[:n]
    label = row.label(casc, size, n)
    with tunables(env, *row.settings()):
        r, entered = check_against_oracle(env, c, frame_set(size)[:n], want, label)
    hb = row.handover()
    if hb is None or row.tile_sp_begin <= hb:   # (at a re-pack point from tile_sp_begin on, the boundary included, a tile
        return                                  # with few windows finishes the cascade in place instead of handing over)
    # the tiles really handed their windows over at hb, and nothing of theirs went past it
    tiles, t = tile_counts(r, c.info.n_stages)
    assert tiles, f"{label}: no tile launch, so no hand-off at stage {hb} was exercised"
    if row.tile_sp_begin >= 64 and row.tile_min_lanes == 0:
        assert t[hb - 1] > 0, f"{label}: the tiles entered no window at stage {hb - 1}, just before the boundary"
    assert not any(t[hb:]), f"{label}: the tiles entered stages at or beyond the boundary {hb}: {t[hb:]}"
    assert r.stage_entered[hb] == entered[hb], f"{label}: {r.stage_entered[hb]} windows entered stage {hb}, the oracle {entered[hb]}"


GROUP_ROWS = [  # (id, settings, hand-off boundary)
    ("end3_lanes0_sp64", (("tile_end", 3), ("tile_min_lanes", 0), ("tile_sp_begin", 64)), 3),
    ("end64_lanes64", (("tile_end", 64), ("tile_min_lanes", 64)), None),
]


@pytest.mark.parametrize("gid,settings,hb", GROUP_ROWS, ids=[g[0] for g in GROUP_ROWS])
def test_scale_group_members_hand_over(monkeypatch, oracle, cascades, gid, settings, hb):
    """Scales 0..3 share one staged tile with VJ_TILE_GROUP=4: every member hands its windows over from the group's pitch
    and origin.  Eight frames against the oracle, and G = 4 against G = 1."""
    casc, n = "frontalface_alt", 8
    c, _ = cascades(casc)
    want = oracle_set(oracle, cascades, casc, MAIN)[:n]
    frames = frame_set(MAIN)[:n]
    out = {}
    for g in (1, 4):
        label = f"{casc} {MAIN[0]}x{MAIN[1]} n={n} VJ_TILE_GROUP={g} " + " ".join(f"{k}={v}" for k, v in settings)
        monkeypatch.setenv("VJ_TILE_GROUP", str(g))
        e = Environment(0)
        try:
            with tunables(e, *settings):
                out[g], entered = check_against_oracle(e, c, frames, want, label)
        finally:
            e.close()
        tiles, t = tile_counts(out[g], c.info.n_stages)
        tile_scales = set().union(*(l["scales"] for l in tiles))
        assert set(range(4)) <= tile_scales, f"{label}: scales 0..3 are not all tile scales: {sorted(tile_scales)}"
        if hb is not None:
            assert t[hb - 1] > 0 and not any(t[hb:]), f"{label}: the tiles did not hand over at stage {hb}: {t}"
    monkeypatch.delenv("VJ_TILE_GROUP")
    assert np.array_equal(out[4].rects, out[1].rects), f"{gid}: VJ_TILE_GROUP 4 and 1 give different rectangles"
    assert (out[4].stage_entered, out[4].windows, out[4].stump_evals) == (out[1].stage_entered, out[1].windows, out[1].stump_evals), \
        f"{gid}: VJ_TILE_GROUP 4 and 1 give different counters"
