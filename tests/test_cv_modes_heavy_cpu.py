"""The premises of tests/test_gpu_cv_modes_heavy.py, on the restatements alone (tests/find_biggest_oracle.c, scale_image_oracle.c,
canny_oracle.c and the oracle): every cell of tests/heavy_cases.py is in the regime it stands for — the band of its before-hit
count, the tie at the first grouping, the scanROI's overflow of a frame's segment, the limit cases' counts after whole scales,
accept_all's rectangles above the detection buffer's initial capacity, a prune that bites while the prefix still passes."""
import numpy as np
import pytest

import canny_oracle as co
import heavy_cases as hc
import scale_image_oracle as so


@pytest.mark.parametrize("cid", list(hc.FB_CELLS))
def test_find_biggest_cells_are_in_their_bands(cid):
    form, spec, mn, kw, band = hc.FB_CELLS[cid]
    res, st = hc.biggest(form, spec, mn, **kw)
    n = hc.before_hit(st)
    print(f"{cid}: {n} before the hit, {st['roi_candidates']} in the ROI (clamped: {st['roi_clamped']}), result {res}")
    assert res is not None and st["first_hit_scale"] >= 0
    assert max(hc.counts_after_each_scale(st)) == n <= hc.GROUP_MAX       # the device groups it: no count after a scale is over the limit
    if band is not None:
        assert band in hc.BANDS and band[0] <= n <= band[1]


def test_find_biggest_cells_cover_every_band_and_form():
    for band in hc.BANDS:
        assert any(band[0] <= hc.before_hit(hc.biggest(f, s, mn, **kw)[1]) <= band[1] for f, s, mn, kw, _ in hc.FB_CELLS.values()), band
    assert {c[0] for c in hc.FB_CELLS.values()} == set(hc.SURVIVOR_FORMS)
    near = [hc.before_hit(hc.biggest(f, s, mn, **kw)[1]) for f, s, mn, kw, b in hc.FB_CELLS.values() if b == (1900, 2048)]
    assert near and all(n > 1024 for n in near)                             # the sort runs at P = 2048, block_rank takes two rounds
    assert sum(1 for c in hc.FB_CELLS.values() if c[3].get("rough")) >= 2 and any("scale_factor" in c[3] for c in hc.FB_CELLS.values())
    rough, plain = hc.biggest(*hc.FB_CELLS["chain_2032_rough"][:3], rough=True), hc.biggest(*hc.FB_CELLS["chain_2032"][:3])
    assert rough[0] != plain[0] and rough[1]["windows"] < plain[1]["windows"]


@pytest.mark.parametrize("cid", list(hc.TIE_CELLS))
def test_first_grouping_is_a_tie(oracle, cid):
    """At the hit, two groups share the greatest area: the pick takes the first of them in class order, and `>=` in place of `>`
    (or another class order) would take the other, whose scanROI lies elsewhere."""
    form, spec, mn = hc.TIE_CELLS[cid]
    res, st = hc.biggest(form, spec, mn)
    cand, n = st["candidates"], hc.before_hit(st)
    assert res is not None and 64 <= n <= hc.GROUP_MAX and n < len(cand)
    xywh = np.stack([cand[k][:n] for k in ("x", "y", "w", "h")], 1).astype(np.int32)      # already in the walk's order
    groups, _ = oracle.group_rectangles(xywh, max(mn, 1))
    areas = [int(g[2]) * int(g[3]) for g in groups]
    tied = [tuple(int(v) for v in g) for g, a in zip(groups, areas) if a == max(areas)]
    print(f"{cid}: {n} before the hit, groups {[tuple(int(v) for v in g) for g in groups]}, result {res}")
    assert len(tied) >= 2 and len(set(tied)) == len(tied)
    pushed = tuple(int(cand[n][k]) for k in ("x", "y", "w", "h"))
    assert pushed == tied[0]
    far = [t for t in tied[1:] if abs(t[0] - pushed[0]) > pushed[2] or abs(t[1] - pushed[1]) > pushed[3]]
    assert far                                               # the other tied group lies outside the first one's scanROI
    if cid.endswith("_anti"):                                # the walk's order (y, x) and the order (x, y) disagree on which is first
        assert all(t[1] > pushed[1] and t[0] < pushed[0] for t in tied[1:])


@pytest.mark.parametrize("cid", hc.ROI_OVERFLOW_CELLS)
def test_scan_roi_overflows_a_default_segment(cid):
    form, spec, mn, kw, _ = hc.FB_CELLS[cid]
    res, st = hc.biggest(form, spec, mn, **kw)
    assert hc.before_hit(st) <= hc.GROUP_MAX and st["roi_candidates"] > hc.FB_SEGMENT
    assert res is not None and res[4] > hc.FB_SEGMENT          # a neighbors count of several thousand
    clamped = {hc.biggest(*hc.FB_CELLS[c][:3])[1]["roi_clamped"] for c in hc.ROI_OVERFLOW_CELLS}
    assert clamped == {True, False}


@pytest.mark.parametrize("cid", list(hc.LIMIT_CELLS))
def test_limit_cells_exceed_group_max_after_a_whole_scale(cid):
    """The device groups after every scale, so what decides is the cumulative count after a whole scale while no group has
    formed: it passes GROUP_MAX before the reference's hit (or the reference never groups), and the ordinary frame of the
    batch stays far below."""
    form, spec, mn, other = hc.LIMIT_CELLS[cid]
    res, st = hc.biggest(form, spec, mn)
    ends = hc.counts_after_each_scale(st)
    print(f"{cid}: result {res}, counts after each scale {ends}")
    assert (res is None) == (cid == "never_groups")
    over = [n for n in ends[:-1] if n > hc.GROUP_MAX] if res is not None else [n for n in ends if n > hc.GROUP_MAX]
    assert over, "no grouping step before the hit sees more than GROUP_MAX candidates"
    res2, st2 = hc.biggest(form, other, mn)
    assert res2 is not None and hc.before_hit(st2) < hc.GROUP_MAX // 4
    assert hc.frame_of(other).shape == hc.frame_of(spec).shape


def test_mixed_batch_holds_every_regime():
    st = [hc.biggest(hc.MIXED_FORM, s, hc.MIXED_NEIGHBORS) for s in hc.MIXED_FRAMES]
    before = [hc.before_hit(s) for _, s in st]
    print("mixed batch: before the hit", before, "in the ROI", [s["roi_candidates"] for _, s in st], "results", [r for r, _ in st])
    assert len({hc.frame_of(s).shape for s in hc.MIXED_FRAMES}) == 1
    assert all(max(hc.counts_after_each_scale(s) or [0]) <= hc.GROUP_MAX for _, s in st)
    assert any(r is not None and n <= 512 and s["roi_candidates"] < 256 for (r, s), n in zip(st, before))       # a few candidates
    assert any(r is not None and 1900 <= n <= hc.GROUP_MAX for (r, _), n in zip(st, before))                       # about 2000 before the hit
    assert any(r is not None and s["roi_candidates"] > hc.FB_SEGMENT for r, s in st)                               # ROI overflow
    assert any(r is None and 0 < len(s["candidates"]) <= 256 for r, s in st)                                       # never groups, few candidates
    assert any(r is None and len(s["candidates"]) == 0 for r, s in st)                                             # no candidate at all
    assert hc.MIXED_FRAMES[4][:2] == ("synth", "smooth")
    assert sum(n > 64 for n in before) >= 3 and max(before) > 1024             # det_cap 64 regrows several times, det_cap 5000 once
    assert len({st[i][1]["first_hit_scale"] for i in range(len(st))}) >= 4    # the frames leave the search at different rounds


@pytest.mark.parametrize("form", hc.SURVIVOR_FORMS)
def test_scale_image_every_window_enters_the_prefix(form):
    for h, w in hc.SIZES:
        for ro, st in hc.cached_many(so.detect_scale_image, form, hc.survivor_specs(h, w)):
            assert st["windows"] > 100000 and st["stage_entered"][:3] == [st["windows"]] * 3
            if form == "accept_all":
                assert len(ro) == st["windows"]
            else:
                assert 1000 < len(ro) < st["windows"] // 20
    assert len({hc.frame_of(s).tobytes() for s in hc.survivor_specs(480, 640)}) == hc.N_DISTINCT


def test_scale_image_accept_all_exceeds_the_initial_detection_buffer():
    for ro, st in hc.cached_many(so.detect_scale_image, "accept_all", hc.survivor_specs(480, 640)):
        assert len(ro) == st["windows"] == 602348 > hc.DET_CAP_INIT


@pytest.mark.parametrize("form", hc.SURVIVOR_FORMS)
def test_canny_prune_bites_and_the_prefix_still_passes(form):
    for h, w in hc.CANNY_SIZES:
        specs = hc.canny_specs(h, w)
        assert len({hc.frame_of(s).tobytes() for s in specs}) == len(specs)
        for (ro, st), spec in zip(hc.cached_many(co.detect_opencvlike, form, specs), specs):
            e = st["stage_entered"]
            print(f"{form} {spec}: {st['windows']} windows, entered {e[:3]}, {len(ro)} rectangles")
            assert 0 < e[0] < st["windows"] * 3 // 4, spec
            assert e[1] == e[0] and len(ro) > 0, spec
            _, off = hc.cached(co.detect_opencvlike, form, spec, prune=False)
            assert off["stage_entered"][0] > e[0], spec


def test_plain_dot_frames_are_barely_pruned():
    """Why the frames above are needed: on dot_frame content the prune drops next to nothing of the linear forms."""
    spec = hc.survivor_specs(240, 320)[0]
    _, st = hc.cached(co.detect_opencvlike, "stumps", spec)
    assert st["stage_entered"][0] > st["windows"] * 9 // 10
