"""Survivor- and candidate-heavy inputs for the three OpenCV-profile modes (find-biggest, scale image, canny pruning): the frames,
cascades and parameter cells that tests/test_cv_modes_heavy_cpu.py (the premises, on the restatements alone) and
tests/test_gpu_cv_modes_heavy.py (the comparisons on the device) share.  Every count in a comment below was measured on the
restatements; the CPU file asserts the condition each cell stands for (a band, an overflow, a tie), so a change to synth, dot_frame
or a restatement that moves a cell out of its regime fails there."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import canny_oracle as co
import find_biggest_oracle as fo
import scale_image_oracle as so
from cases import SURVIVOR_FORMS, cascade_to_product, dot_frame, survivor_cascade

VJ_ERR_LIMIT = 8                     # include/vj.h
GROUP_MAX = 2048                     # vj_internal.hpp: candidates one workgroup groups in LDS
FB_SEGMENT = 2 * GROUP_MAX           # a frame's segment of the candidate buffer at the default det_cap
DET_CAP_INIT = 65536
LINEAR_FORMS = ("stumps", "trees", "accept_all")
TREE_FORMS = ("chain_tree", "branch_tree")
N_DISTINCT = 4
_ARR, _PROD, _FRAMES, _CACHE = {}, {}, {}, {}


def arrays(form):
    if form not in _ARR:
        _ARR[form] = survivor_cascade(form)
    return _ARR[form]


def product(form):
    """(product Cascade, oracle CascadeArrays); loads the library."""
    if form not in _PROD:
        _PROD[form] = (cascade_to_product(arrays(form)), arrays(form))
    return _PROD[form]


# ----------------------------------------------------------------------------- frames
def block_frame(seed, h, w, n_dots, block):
    """dot_frame with one constant square (y, x, side, value): inside it the variance norm factor is 0, so the selective nodes
    (threshold 0.05 x 0) let every window of every scale through — a region as dense as accept_all's inside a frame that is
    otherwise as sparse as the dots."""
    f = dot_frame(seed, h, w, n_dots)
    y, x, side, value = block
    f[y:y + side, x:x + side] = value
    return f


TIE_PATCH_SEED, TIE_PATCH_DOTS, TIE_PATCH_SIDE = 1, 6, 30


def tie_frame(seed, h, w, at, offset):
    """The same patch of dots pasted at `at` and at `at + offset` on a dark noise frame: two clusters of candidates whose classes
    average to the same w x h."""
    f = dot_frame(seed, h, w, 0)
    rng = np.random.default_rng(TIE_PATCH_SEED)
    patch = list(zip(rng.integers(0, TIE_PATCH_SIDE, TIE_PATCH_DOTS), rng.integers(0, TIE_PATCH_SIDE, TIE_PATCH_DOTS)))
    for y0, x0 in (at, (at[0] + offset[0], at[1] + offset[1])):
        for y, x in patch:
            f[y0 + int(y):y0 + int(y) + 4, x0 + int(x):x0 + int(x) + 4] = 255
    return f


def half_flat_frame(seed, h, w):
    """The survivor frames' content on the right, a constant left half: Canny finds no edge there, so the pruning test drops
    the windows of the left half (and the windows it keeps still pass the all-pass prefix)."""
    f = dot_frame(seed, h, w, (h * w) // 4000)
    f[:, :w // 2] = 24
    return f


def dark_patches_frame(seed, h, w):
    """canny_oracle.patches_frame (flat with a few textured patches and crude faces) darkened into dot_frame's range."""
    return (16 + co.patches_frame(seed, h, w) // 8).astype(np.uint8)


def frame_of(spec):
    """A frame from its spec: ("dots", seed, h, w, n_dots) | ("block", seed, h, w, n_dots, (y, x, side, value)) |
    ("tie", seed, h, w, (y, x), (dy, dx)) | ("synth", kind, seed, h, w) | ("half_flat", seed, h, w) | ("patches", seed, h, w)."""
    if spec not in _FRAMES:
        kind = spec[0]
        if kind == "dots":
            f = dot_frame(*spec[1:])
        elif kind == "block":
            f = block_frame(*spec[1:])
        elif kind == "tie":
            f = tie_frame(*spec[1:])
        elif kind == "synth":
            from clfacedetection_amd import synth
            f = synth.frame(spec[1], spec[2], spec[3], spec[4])
        elif kind == "half_flat":
            f = half_flat_frame(*spec[1:])
        elif kind == "patches":
            f = dark_patches_frame(*spec[1:])
        else:
            raise KeyError(spec)
        _FRAMES[spec] = np.ascontiguousarray(f)
    return _FRAMES[spec]


def survivor_specs(h, w):
    """The four distinct frames of tests/test_gpu_survivors.py at a size."""
    return [("dots", 7000 + i, h, w, (h * w) // 4000) for i in range(N_DISTINCT)]


def repeat(specs, n):
    return [specs[i % len(specs)] for i in range(n)]


# ----------------------------------------------------------------------------- the restatements, once per distinct input
def cached(fn, form, spec, **kw):
    key = (fn.__name__, form, spec, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = fn(arrays(form), frame_of(spec), **kw)
    return _CACHE[key]


def cached_many(fn, form, specs, **kw):
    """cached() for several frames at once (the C entry points release the GIL)."""
    todo = [s for s in dict.fromkeys(specs) if (fn.__name__, form, s, tuple(sorted(kw.items()))) not in _CACHE]
    if len(todo) > 1:
        with ThreadPoolExecutor(min(len(todo), 8)) as ex:
            list(ex.map(lambda s: cached(fn, form, s, **kw), todo))
    return [cached(fn, form, s, **kw) for s in specs]


def biggest(form, spec, min_neighbors, rough=False, scale_factor=1.1):
    return cached(fo.detect_biggest, form, spec, min_neighbors=min_neighbors, rough=rough, scale_factor=scale_factor)


# ----------------------------------------------------------------------------- 1. find-biggest
def before_hit(st) -> int:
    """Candidates in the list when the first group forms: the index of the pushed maxRect (scale_idx -2) in the restatement's
    candidate list, or the whole length when the frame never groups."""
    idx = np.flatnonzero(st["candidates"]["scale_idx"] == -2)
    return int(idx[0]) if len(idx) else len(st["candidates"])


def counts_after_each_scale(st) -> list:
    """The cumulative candidate count after every whole scale of the search phase that yielded any: what the grouping step
    after a scale sees, and what the device compares with GROUP_MAX (grouping runs once per scale)."""
    si = st["candidates"]["scale_idx"][:before_hit(st)]
    return [int((si >= k).sum()) for k in sorted(set(si.tolist()), reverse=True)]


D40 = ("dots", 3, 180, 240, 40)
BANDS = ((64, 256), (257, 1024), (1025, 2048), (1900, 2048))
# id: (form, frame, min_neighbors, keyword arguments, band of the before-hit count or None)
#                                                                                          measured: before hit | in the ROI | result
FB_CELLS = {
    "stumps_94": ("stumps", D40, 40, {}, (64, 256)),                                     # 94 | 91 | (144, 31, 47, 47) x 138
    "trees_615": ("trees", D40, 100, {}, (257, 1024)),                                   # 615 | 165 | (128, 74, 52, 52) x 105
    "stumps_1003": ("stumps", D40, 100, {}, (257, 1024)),                                # 1003 | 48 | (146, 32, 44, 44) x 158
    "trees_1573": ("trees", D40, 200, {}, (1025, 2048)),                                 # 1573 | 224 | (91, 55, 44, 44) x 304
    "chain_1305": ("chain_tree", D40, 150, {}, (1025, 2048)),                            # 1305 | 92 | (100, 122, 45, 45) x 152
    "chain_2032": ("chain_tree", D40, 200, {}, (1900, 2048)),                            # 2032 | 137 | (77, 73, 39, 39) x 221
    "branch_2032": ("branch_tree", D40, 200, {}, (1900, 2048)),                          # 2032 | 137 | (77, 73, 39, 39) x 221
    "branch_503": ("branch_tree", D40, 100, {}, (257, 1024)),                            # 503 | 133 | (150, 28, 44, 44) x 240
    "accept_1059": ("accept_all", ("dots", 3, 240, 320, 40), 1000, {}, (1025, 2048)),    # 1059 | 7717 | (109, 70, 86, 86) x 8777
    "accept_18": ("accept_all", D40, 3, {}, None),                                       # 18 | 4849, ROI clamped | (69, 45, 84, 84) x 4868
    "chain_2032_rough": ("chain_tree", D40, 200, {"rough": True}, (1900, 2048)),         # 2032 | 55 | (101, 126, 39, 39) x 278
    "accept_18_rough": ("accept_all", D40, 3, {"rough": True}, None),                    # 18 | 922, ROI clamped | (53, 28, 114, 114) x 941
    "trees_sf125": ("trees", D40, 150, {"scale_factor": 1.25}, (1025, 2048)),            # 1733 | 38 | (99, 130, 34, 34) x 228
}
ROI_OVERFLOW_CELLS = ("accept_18", "accept_1059")         # roi_candidates > FB_SEGMENT; roi_clamped True and False
# Ties: two classes of equal greatest area at the first grouping; (id: form, frame, min_neighbors)
TIE_CELLS = {
    "stumps_tie": ("stumps", ("tie", 9, 180, 240, (30, 30), (60, 100)), 80),     # 445 before hit; four groups, 39 x 39 twice, a 36 x 36 between them
    "trees_tie": ("trees", ("tie", 9, 180, 240, (30, 30), (0, 120)), 150),       # 431 before hit; two groups of 47 x 47
    # 443 before hit; (138, 26, 39, 39) and (38, 86, 39, 39): the first in the walk's order (y, then x) is the LAST by x, so a sort
    # key that orders a scale's candidates by x first picks the other one
    "stumps_tie_anti": ("stumps", ("tie", 9, 180, 240, (30, 130), (60, -100)), 80),
}
# The limit: more than GROUP_MAX candidates after a whole scale, and still no group
LIMIT_CELLS = {
    # 2239 candidates and no group in the reference; after the scales ... 1928, 2075: over the limit two scales before the end
    "never_groups": ("stumps", D40, 200, ("block", 5, 180, 240, 0, (30, 40, 100, 24))),
    # 6121 before the reference's hit; after the scales ... 1478, 2211: over the limit six scales before the reference groups
    "groups_late": ("stumps", ("dots", 3, 240, 320, 200), 200, ("block", 5, 240, 320, 0, (30, 40, 100, 24))),
}                                                   # (.., an ordinary frame of the same size and call: 244 before its hit)
# One batch of every regime: chain_tree, min_neighbors 200, 180 x 240
MIXED_FORM, MIXED_NEIGHBORS = "chain_tree", 200
MIXED_FRAMES = (
    ("dots", 11, 180, 240, 2),                        # a few: 320 before the hit, 63 in the ROI
    D40,                                              # 2032 before the hit
    ("block", 5, 180, 240, 0, (30, 40, 120, 24)),     # 241 before the hit, 4313 in the ROI: its segment overflows there
    ("dots", 11, 180, 240, 1),                        # 179 candidates, never groups
    ("synth", "smooth", 41, 180, 240),                # a smooth frame: 390 before the hit, 1842 in the ROI
    ("synth", "noise", 41, 180, 240),                 # no candidate at all
    ("dots", 11, 180, 240, 3),                        # 490 before the hit
)
MIXED_SETTINGS = ((("max_subbatch", "3"),), (("concurrent", "0"),), (("det_cap", "64"),), (("det_cap", "5000"),))

# ----------------------------------------------------------------------------- 2. scale image, 3. canny pruning, 4. the plain path
SIZES = ((240, 320), (480, 640), (479, 641))
BATCHES = (1, 7, 11)
SI_BIG = (1080, 1920, 8, ("stumps", "trees"))
SI_ACCEPT_ALL_BATCHES = (1, 3)                           # accept_all: every grid position is a rectangle; 480 x 640 only in a fresh environment
CANNY_SIZES = ((240, 320), (480, 640))
CANNY_BATCHES = (1, 8)
PLAIN_SIZES = ((480, 640), (479, 641))
PLAIN_BATCHES = (1, 8, 11)


def canny_specs(h, w):
    """Four distinct frames on which the prune bites: two half-flat survivor frames, two darkened patches frames."""
    return [("half_flat", 7000, h, w), ("patches", 4, h, w), ("half_flat", 7001, h, w), ("patches", 5, h, w)]


def nodes_per_stage(a):
    return [int(sum(a.tree_n_nodes[a.stage_first_tree[s]:a.stage_first_tree[s] + a.stage_n_trees[s]])) for s in range(a.n_stages)]


assert set(LINEAR_FORMS + TREE_FORMS) == set(SURVIVOR_FORMS)
