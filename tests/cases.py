"""Seeded parity cases shared by the golden generator (tools/make_golden.py), the CPU
tests (oracle vs fixtures) and the GPU tests (HIP path vs oracle and vs fixtures)."""
from __future__ import annotations

import contextlib
import hashlib
import lzma
import os

import numpy as np

from clfacedetection_amd import synth

# (id, cascade, generator, seed, height, width, min_size, max_size, signed_mean)
DETECT_CASES = [
    ("alt_xs12345_480", "frontalface_alt", "xorshift", 12345, 480, 640, (0, 0), (0, 0), False),
    ("default_xs12345_480", "frontalface_default", "xorshift", 12345, 480, 640, (0, 0), (0, 0), False),
    ("alt_noise_240", "frontalface_alt", "noise", 7, 240, 320, (0, 0), (0, 0), False),
    ("alt_smooth_480", "frontalface_alt", "smooth", 11, 480, 640, (0, 0), (0, 0), False),
    ("alt_blocks_odd", "frontalface_alt", "blocks", 5, 251, 333, (0, 0), (0, 0), False),
    ("default_min40", "frontalface_default", "noise", 21, 480, 640, (40, 40), (0, 0), False),
    ("default_minmax", "frontalface_default", "smooth", 22, 360, 480, (30, 30), (120, 120), False),
    ("eye_noise_300", "eye", "noise", 31, 300, 400, (0, 0), (0, 0), False),
    ("eye_blocks_200", "eye", "blocks", 32, 200, 200, (0, 0), (0, 0), False),
    ("alt_signed_mean", "frontalface_alt", "noise", 41, 240, 320, (0, 0), (0, 0), True),
    ("alt_tiny", "frontalface_alt", "noise", 51, 31, 31, (0, 0), (0, 0), False),
    ("alt_wide", "frontalface_alt", "noise", 52, 40, 700, (0, 0), (0, 0), False),
    ("alt2_noise_240", "frontalface_alt2", "noise", 61, 240, 320, (0, 0), (0, 0), False),
    ("alt2_smooth_300", "frontalface_alt2", "smooth", 62, 300, 400, (0, 0), (0, 0), False),
    ("alt_tree_noise_240", "frontalface_alt_tree", "noise", 71, 240, 320, (0, 0), (0, 0), False),
    ("alt_tree_blocks_300", "frontalface_alt_tree", "blocks", 72, 300, 400, (0, 0), (0, 0), False),
    # cascades the reference ships that the configs do not name: non-square base windows, and tilted features, which the clod
    # path reads as upright rectangles (clod.cpp:448-492; the GPU test calls at the reference's signature, which passes the flag)
    ("eyepair_small_noise", "mcs_eyepair_small", "noise", 91, 200, 320, (0, 0), (0, 0), False),     # 22 x 5
    ("eyepair_big_blocks", "mcs_eyepair_big", "blocks", 92, 240, 400, (0, 0), (0, 0), False),       # 45 x 11
    ("lowerbody_blocks", "lowerbody", "blocks", 93, 240, 320, (0, 0), (0, 0), False),               # 19 x 23
    ("profileface_noise", "profileface", "noise", 94, 240, 320, (0, 0), (0, 0), False),
    ("righteye_2splits_smooth", "righteye_2splits", "smooth", 95, 240, 320, (0, 0), (0, 0), False), # two-node trees with tilted nodes
    ("mcs_mouth_minmax", "mcs_mouth", "blocks", 96, 300, 400, (30, 18), (150, 90), False),          # 25 x 15, size limits
]
# the headline pin: the survey's recorded reference run
HEADLINE_CASE = ("alt_xs12345_1080", "frontalface_alt", "xorshift", 12345, 1080, 1920, (0, 0), (0, 0), False)

# the other evaluation modes (tests/golden/modes.json): P2 skip variants and the OpenCV arithmetic profile
MODE_CASES = [  # (id, cascade, generator, seed, height, width)
    ("m_alt_xs_480", "frontalface_alt", "xorshift", 12345, 480, 640),
    ("m_alt_smooth", "frontalface_alt", "smooth", 11, 300, 420),
    ("m_default_blocks", "frontalface_default", "blocks", 6, 360, 480),
    ("m_alt2_noise", "frontalface_alt2", "noise", 61, 240, 320),
    ("m_eye_noise", "eye", "noise", 31, 200, 260),
    ("m_alt_tree_blocks", "frontalface_alt_tree", "blocks", 72, 300, 400),
    ("m_fullbody_noise", "fullbody", "noise", 81, 240, 320),
    ("m_eyeglasses_smooth", "eye_tree_eyeglasses", "smooth", 84, 240, 320),
    ("m_mcs_nose_noise", "mcs_nose", "noise", 85, 200, 260),                 # 18 x 15, 990 tilted nodes
    ("m_upperbody_blocks", "upperbody", "blocks", 86, 240, 320),             # 22 x 18
    ("m_profileface_smooth", "profileface", "smooth", 87, 240, 320),         # upright stumps: skip modes too
    ("m_lefteye_2splits_noise", "lefteye_2splits", "noise", 88, 240, 320),
    ("m_eyepair_big_blocks", "mcs_eyepair_big", "blocks", 89, 200, 400),     # 45 x 11
]

GROUP_CASES = [  # (id, first cascade, second cascade, seed, height, width, min_neighbors): drawn faces (synth kind "faces")
    ("g_alt2_eye_3", "frontalface_alt2", "eye", 1, 360, 640, 3),
    ("g_alt_eye_1", "frontalface_alt", "eye", 2, 300, 480, 1),
    ("g_default_eye_3", "frontalface_default", "eye", 3, 360, 640, 3),
]

INTEGRAL_CASES = [  # (id, generator, seed, height, width)
    ("i_1x1", "noise", 1, 1, 1), ("i_3x5", "noise", 2, 3, 5), ("i_8x256", "noise", 3, 8, 256),
    ("i_9x257", "noise", 4, 9, 257), ("i_odd", "smooth", 5, 251, 333), ("i_vga", "noise", 6, 480, 640),
    ("i_white", "white", 0, 64, 300), ("i_1080p", "noise", 7, 1080, 1920),
]


# BASELINE.json's configs at their full sizes (tests/golden/fullsize.json, tools/make_fullsize_golden.py): the oracle
# runs once in the build container, the GPU suite compares whole results through rows_sha()
FULLSIZE = {
    "config3": {"cascade": "frontalface_alt", "frames": 64, "height": 1080, "width": 1920, "seed0": 1,
                "kinds": ["noise", "smooth", "blocks"]},
    "config4": {"cascade": "frontalface_alt_tree", "kind": "noise", "seed": 4096, "height": 4096, "width": 4096},
    "config5_raw": {"cascade": "frontalface_alt2", "second": "eye", "frames": 256, "height": 720, "width": 1280,
                    "seed0": 5001, "kinds": ["noise", "smooth", "blocks"]},
    "config5_grouped": {"cascade": "frontalface_alt2", "second": "eye", "frames": 256, "height": 720, "width": 1280,
                        "seed0": 5001, "kinds": ["faces", "noise", "smooth", "blocks"], "min_neighbors": 3},
    # (id, cascade, generator, seed, height, width)
    "opencv": [("cv_alt_pin_1080", "frontalface_alt", "xorshift", 12345, 1080, 1920),
               ("cv_alt_smooth_1080", "frontalface_alt", "smooth", 2, 1080, 1920),
               ("cv_alt_blocks_1080", "frontalface_alt", "blocks", 3, 1080, 1920),
               ("cv_alt_faces_1080", "frontalface_alt", "faces", 4, 1080, 1920),
               ("cv_alt_tree_noise_1080", "frontalface_alt_tree", "noise", 5, 1080, 1920),
               ("cv_alt_tree_faces_1080", "frontalface_alt_tree", "faces", 6, 1080, 1920),
               ("cv_alt2_faces_1080", "frontalface_alt2", "faces", 7, 1080, 1920),
               ("cv_fullbody_smooth_1080", "fullbody", "smooth", 8, 1080, 1920)],
    # (id, cascade, generator, seed, height, width): cascades the configs do not name, at 1080p in BOTH profiles (the clod profile reads
    # tilted rectangles as upright ones, like the reference)
    "shipped": [("s_upperbody_blocks_1080", "upperbody", "blocks", 11, 1080, 1920),
                ("s_mcs_mouth_faces_1080", "mcs_mouth", "faces", 12, 1080, 1920),
                ("s_eyepair_small_noise_1080", "mcs_eyepair_small", "noise", 13, 1080, 1920),
                ("s_lowerbody_smooth_1080", "lowerbody", "smooth", 14, 1080, 1920),
                ("s_righteye_2splits_faces_1080", "righteye_2splits", "faces", 15, 1080, 1920),
                ("s_profileface_faces_1080", "profileface", "faces", 16, 1080, 1920)],
    # (id, cascade, generator, seed, height, width, oracle mode): the CPU variants' window sets at 1080p
    "modes": [(f"m{mode}_{kind}_1080", "frontalface_alt", kind, seed, 1080, 1920, mode)
              for mode in (2, 3, 4, 5) for kind, seed in (("noise", 1), ("smooth", 2), ("faces", 4))],
}


def rows_sha(rects, keys=("scale_idx", "x", "y", "w", "h")) -> str:
    """SHA-256 of the rows of a rectangle list as little-endian int32, in the order given (results are sorted by
    (scale, y, x) on both sides).  `rects`: a structured array (fields `keys`) or a list of int tuples."""
    if isinstance(rects, np.ndarray) and rects.dtype.names:
        a = np.stack([rects[k].astype("<i4") for k in keys], 1) if len(rects) else np.zeros((0, len(keys)), "<i4")
    else:
        a = np.asarray(list(rects), "<i4").reshape(len(rects), -1) if len(rects) else np.zeros((0, 0), "<i4")
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_frame(generator: str, seed: int, h: int, w: int, oracle=None) -> np.ndarray:
    if generator == "xorshift":   # the survey's sequential generator lives in the oracle
        return oracle.xorshift_noise(seed, h, w)
    if generator == "white":
        return np.full((h, w), 255, np.uint8)
    return synth.frame(generator, seed, h, w)


def block_grid_frame(transposed: bool = False) -> np.ndarray:
    """A 900 x 300 (or 300 x 900) frame with a drawn face of 238 pixels at column (row) 650.  Scale 26 of a 20 x 20
    cascade (s = 11.918..., window 238) puts grid index 55 on pixel 656 when the product index * step is the f32 one
    (656.50 after rounding to 24 bits) and on 655 when it is the f64 one (655.4999...): the reference's block variant
    (double step, clod.cpp:862) and its other loops then evaluate different windows over the face, and with
    frontalface_alt they return different rectangles (x = 655 vs 656)."""
    face = np.clip(synth.crude_face(238), 0, 255).astype(np.uint8)
    if transposed:
        img = synth.frame("smooth", 26, 900, 300).copy()
        img[650:888, 20:258] = face
    else:
        img = synth.frame("smooth", 26, 300, 900).copy()
        img[20:258, 650:888] = face
    return img


BLOCK_GRID_LIMITS = {"min_size": (230, 230), "max_size": (270, 270)}     # scales 26 and 27 only


# the 19 stock OpenCV XMLs the cascades in clfacedetection_amd/data/ were converted from, verbatim and xz-compressed
# (tools/make_xml_golden.py): the loader tests read the XML text itself without the reference checkout
XML_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xml")
STOCK_XMLS = sorted(f[:-len(".xz")] for f in os.listdir(XML_DIR) if f.endswith(".xml.xz"))


def stock_xml(xml: str, dest_dir) -> str:
    """tests/golden/xml/<xml>.xz unpacked into dest_dir; returns the XML's path."""
    path = os.path.join(str(dest_dir), xml)
    with open(path, "wb") as f:
        f.write(lzma.decompress(open(os.path.join(XML_DIR, xml + ".xz"), "rb").read()))
    return path


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ----------------------------------------------------------------------------- OpenCV-profile arithmetic probes
def crafted_stump_cascade(three_rects: bool, threshold: float):
    """One stage, one stump, 20x20 window; leaves 0 / 1 and stage threshold 0.5: the window is a detection exactly
    when the node sum is >= threshold * vnf.  The rectangles nearly cancel (like real Haar features), so the rounding
    of each product shows in the sum."""
    from oracle.oracle import CascadeArrays
    c = CascadeArrays()
    c.win_w = c.win_h = 20
    c.name = "crafted"
    c.stage_first_tree = np.array([0], np.int32)
    c.stage_n_trees = np.array([1], np.int32)
    c.stage_threshold = np.array([0.5], np.float32)
    c.stage_parent = np.array([-1], np.int32)
    c.stage_next = np.array([-1], np.int32)
    c.stage_child = np.array([-1], np.int32)
    c.tree_first_node = np.array([0], np.int32)
    c.tree_n_nodes = np.array([1], np.int32)
    c.tree_first_alpha = np.array([0], np.int32)
    rects = [[2, 2, 16, 16], [2, 2, 8, 16], [10, 4, 4, 8] if three_rects else [0, 0, 0, 0]]
    c.node_rect = np.array(rects, np.int32).reshape(-1)
    c.node_weight = np.array([-1.0, 2.0, 0.5 if three_rects else 0.0], np.float32)
    c.node_threshold = np.array([threshold], np.float32)
    c.node_left = np.array([0], np.int32)
    c.node_right = np.array([-1], np.int32)
    c.node_tilted = np.array([0], np.int32)
    c.alpha = np.array([0.0, 1.0], np.float32)
    return c


def single_window_frame(seed: int, size: int = 600):
    """(bright noisy frame, factor): at the largest factor of cvHaarDetectObjects' loop for a 20x20 cascade the frame
    holds exactly one window, at (0, 0), whose rectangle sums are far above 2^24."""
    rng = np.random.default_rng(seed)
    img = (180 + rng.integers(0, 76, (size, size))).astype(np.uint8)
    factor, n = 1.0, 0
    while factor * 20 < size - 10:
        last = factor
        factor *= 1.1
    return img, last


def cascade_to_product(c):
    """oracle CascadeArrays -> product Cascade through vj_cascade_from_arrays."""
    from clfacedetection_amd import Cascade
    from clfacedetection_amd.api import NODE_DTYPE, STAGE_DTYPE, TREE_DTYPE
    st = np.zeros(c.n_stages, STAGE_DTYPE)
    st["first_tree"], st["n_trees"], st["threshold"] = c.stage_first_tree, c.stage_n_trees, c.stage_threshold
    st["parent"], st["next"], st["child"] = c.stage_parent, c.stage_next, c.stage_child
    tr = np.zeros(c.n_trees, TREE_DTYPE)
    tr["first_node"], tr["n_nodes"], tr["first_alpha"] = c.tree_first_node, c.tree_n_nodes, c.tree_first_alpha
    nd = np.zeros(c.n_nodes, NODE_DTYPE)
    r = c.node_rect.reshape(-1, 3, 4)
    w = c.node_weight.reshape(-1, 3)
    for k, f in enumerate(("x", "y", "w", "h")):
        nd["rect"][f] = r[:, :, k]
    nd["rect"]["weight"] = w
    nd["n_rects"] = (w != 0).sum(1)
    nd["tilted"] = c.node_tilted if len(c.node_tilted) == c.n_nodes else 0
    nd["threshold"], nd["left"], nd["right"] = c.node_threshold, c.node_left, c.node_right
    return Cascade.from_arrays(c.win_w, c.win_h, st, tr, nd, c.alpha)


def as_stage_tree(c, split_at: int = 4):
    """A copy of a linear cascade re-linked like frontalface_alt_tree: stages 0..split_at form a chain, then two
    chains alternate (split_at+1, +3, +5, ... and split_at+2, +4, ...), the second one taking over when the first rejects
    (parent / next / child as icvReadHaarClassifier would have set them)."""
    import copy
    t = copy.deepcopy(c)
    n = t.n_stages
    parent = np.full(n, -1, np.int32)
    nxt = np.full(n, -1, np.int32)
    for i in range(1, n):
        parent[i] = i - 1 if i <= split_at + 1 else i - 2
    parent[split_at + 2] = split_at
    nxt[split_at + 1] = split_at + 2
    child = np.full(n, -1, np.int32)
    for i in range(n):
        if parent[i] != -1 and child[parent[i]] == -1:
            child[parent[i]] = i
    t.stage_parent, t.stage_next, t.stage_child = parent, nxt, child
    return t


# vj_env_configure keys, read from the rows of the key table in vj_env.cpp (each row begins with its maker and the key name)
CONFIGURE_ACTIONS = ("defaults", "balance_export", "balance_import")   # keys that do something rather than hold a value


def configure_keys() -> list[str]:
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "clfacedetection_amd", "csrc", "vj_env.cpp")).read()
    return re.findall(r'^\s+(?:flag|int_flag|clamped|bounded|with_auto|int_list|special)\("([a-z0-9_]+)"', src, re.M)


@contextlib.contextmanager
def tunables(env, *settings):
    """with tunables(env, ("tile_split", "1"), ...): apply the settings in order; on exit every tunable goes back to its
    default (configure("defaults", "")), whatever the body did."""
    try:
        for k, v in settings:
            env.configure(k, v)
        yield env
    finally:
        env.configure("defaults", "")


# ----------------------------------------------------------------------------- feature geometry at the window's edges
GEOMETRY_WINDOWS = ((20, 20), (24, 24), (45, 11), (14, 28), (7, 5))   # (win_w, win_h)
GEOMETRY_KINDS = ("upright", "tilted", "tree")


def _geometry_nodes(ww: int, wh: int, kind: str):
    """The nodes of one geometry cascade, as stages of [(tilted, [(x, y, w, h, weight), ...])].  Every rectangle lies
    inside the window by the loader's rule, most of them on one of its bounds; rect 0 always has an area (the evaluators
    scale its weight by the others' areas over its own)."""
    a = max(1, min(ww, wh) // 4)                       # side of the small tilted rectangles
    hh = min(wh // 2, ww // 2)
    dia = (hh, 0, min(ww - hh, wh - hh), hh)           # the largest tilted rectangle: x - h == 0, y == 0, on x + w or y + w + h
    t_low = (a, wh - 2 * a, a, a)                      # x - h == 0, y + w + h == win_h
    t_right = (ww - a, 0, a, a)                        # x + w == win_w, y == 0
    t_min = (1, 0, 1, 1)                               # the smallest one, on x - h == 0 and y == 0
    t_min_br = (ww - 1, wh - 2, 1, 1)                  # ... on x + w == win_w and y + w + h == win_h
    half_w, half_h = max(1, ww // 2), max(1, wh // 2)
    full = (0, 0, ww, wh)
    upright = [
        [(0, 0, ww, wh, -1.0), (ww // 3, wh // 3, max(1, ww // 3), max(1, wh // 3), 3.0)],           # the full window
        [(ww - half_w, 0, half_w, wh, -1.0), (ww - 1, 0, 1, wh, 2.0)],                             # flush right, 1-px strip
        [(0, wh - half_h, ww, half_h, -1.0), (0, wh - 1, ww, 1, 2.0)],                             # flush bottom, 1-px strip
        [(0, 0, 1, wh, 1.0), (0, 0, ww, 1, -2.0)],                                                 # left / top strips, negative
        [(ww - 2, wh - 2, 2, 2, -1.0), (0, 0, 2, 2, 1.0), (ww - 2, 0, 2, 2, 1.0)],                 # three corners
        [(0, wh - 2, 2, 2, -1.0), (ww - 2, wh - 2, 2, 2, 2.0), (0, 0, ww, wh, 0.0)],               # w[2] == 0: rect 2 unused
        [(1, 1, ww - 2, wh - 2, -1.0), (ww, 0, 0, wh, 2.0), (0, wh // 2, ww, half_h, -1.0)],       # w == 0 on the right bound
        [(0, 0, half_w, half_h, -1.0), (0, wh, ww, 0, 1.0), (ww - half_w, wh - half_h, half_w, half_h, 2.0)],  # h == 0 at the bottom
        [(0, 0, ww, wh, 1.0), (ww // 2, 0, ww - ww // 2, wh, -3.0), (0, 0, ww, wh // 2, -1.0)],    # negative weights, three rects
    ]
    tilted = [
        [dia, (hh, 0, 1, 1, 2.0)],
        [t_low, t_right],
        [t_min, t_min_br],
        [(dia[0], dia[1], dia[2], dia[3]), (a, wh - 2 * a, 0, a, 1.0), t_right],   # w == 0 inside, three rects
        [(t_right[0], t_right[1], t_right[2], t_right[3]), (hh, 0, hh, 0, 1.0)],  # h == 0
    ]
    tilted = [[r if len(r) == 5 else (*r, (-1.0, 2.0, 1.5)[i]) for i, r in enumerate(n)] for n in tilted]
    if kind == "upright":
        return [[(0, n) for n in upright[:5]], [(0, n) for n in upright[5:]]]
    if kind == "tilted":
        return [[(1, n) for n in tilted], [(0, upright[0]), (1, tilted[0]), (0, upright[4]), (1, tilted[2])]]
    # two-node trees: (root, child), the child hangs off the root's left branch
    return [[((0, upright[1]), (1, tilted[1])), ((1, tilted[0]), (0, upright[2])), ((0, upright[6]), (0, upright[4]))],
            [((1, tilted[2]), (1, tilted[3])), ((0, upright[0]), (1, tilted[4])), ((1, tilted[4]), (0, upright[8]))]]


def geometry_cascade(ww: int, wh: int, kind: str):
    """oracle CascadeArrays of a two-stage cascade whose features sit on the edges of a ww x wh window: kind "upright"
    (stumps), "tilted" (stumps, tilted ones on each of the four tilted bounds) or "tree" (two-node trees mixing upright and
    tilted nodes).  Node thresholds are 0, leaves 0 / 1 (0.5 on a tree root's right), and a stage passes when its trees' sum
    reaches three quarters of their number: on noise, blocks and smooth frames some windows pass each stage, most do not."""
    from oracle.oracle import CascadeArrays
    c = CascadeArrays()
    c.win_w, c.win_h = ww, wh
    c.name = f"geometry_{kind}_{ww}x{wh}"
    st_first, st_n, st_thr, tr_first, tr_n, tr_alpha = [], [], [], [], [], []
    rects, weights, thr, left, right, tilted, alpha = [], [], [], [], [], [], []
    for stage in _geometry_nodes(ww, wh, kind):
        st_first.append(len(tr_first))
        st_n.append(len(stage))
        st_thr.append(0.75 * len(stage) - 0.125)
        for tree in stage:
            nodes = [tree] if kind != "tree" else list(tree)
            tr_first.append(len(thr))
            tr_n.append(len(nodes))
            tr_alpha.append(len(alpha))
            for k, (t, rr) in enumerate(nodes):
                rr = list(rr) + [(0, 0, 0, 0, 0.0)] * (3 - len(rr))
                rects += [r[:4] for r in rr]
                weights += [r[4] for r in rr]
                thr.append(0.0)
                tilted.append(t)
                if len(nodes) == 1:
                    left.append(0); right.append(-1)
                elif k == 0:
                    left.append(1); right.append(0)            # left -> the child node, right -> alpha[0]
                else:
                    left.append(-1); right.append(-2)          # alpha[1], alpha[2]
            alpha += [0.0, 1.0] if len(nodes) == 1 else [0.5, 0.0, 1.0]
    c.stage_first_tree = np.array(st_first, np.int32)
    c.stage_n_trees = np.array(st_n, np.int32)
    c.stage_threshold = np.array(st_thr, np.float32)
    c.stage_parent = np.arange(-1, len(st_first) - 1, dtype=np.int32)
    c.stage_next = np.full(len(st_first), -1, np.int32)
    c.stage_child = np.array(list(range(1, len(st_first))) + [-1], np.int32)
    c.tree_first_node = np.array(tr_first, np.int32)
    c.tree_n_nodes = np.array(tr_n, np.int32)
    c.tree_first_alpha = np.array(tr_alpha, np.int32)
    c.node_rect = np.array(rects, np.int32).reshape(-1)
    c.node_weight = np.array(weights, np.float32)
    c.node_threshold = np.array(thr, np.float32)
    c.node_left = np.array(left, np.int32)
    c.node_right = np.array(right, np.int32)
    c.node_tilted = np.array(tilted, np.int32)
    c.alpha = np.array(alpha, np.float32)
    return c


def rect_inside_window(x: int, y: int, w: int, h: int, tilted: bool, ww: int, wh: int) -> bool:
    """The loader's rule (icvCreateHidHaarClassifierCascade's)."""
    if min(x, y, w, h) < 0:
        return False
    if tilted:
        return x - h >= 0 and x + w <= ww and y + w + h <= wh
    return x + w <= ww and y + h <= wh


def round_f32(v) -> int:
    """round() of a positive binary32 value, half away from zero, as the plan rounds int * float (vj_plan.cpp)."""
    return int(np.floor(np.float64(np.float32(v)) + 0.5))


def overhangs(c, scales) -> dict:
    """{"x": [...], "y": [...]}: (scale index, node, rect) of every weighted rectangle whose rounded far edge passes the
    rounded window by one pixel at one of `scales` (ScaleInfo rows of the clod plan), in the plan's f32 arithmetic:
    round(x s) + round(w s) == round(win_w s) + 1 (and in y)."""
    out = {"x": [], "y": []}
    r = c.node_rect.reshape(-1, 3, 4)
    wt = c.node_weight.reshape(-1, 3)
    for si in scales:
        s = np.float32(si.scale)
        ex, ey = round_f32(np.float32(c.win_w) * s), round_f32(np.float32(c.win_h) * s)
        for n in range(c.n_nodes):
            for q in range(3):
                if wt[n, q] == 0:
                    continue
                x, y, w, h = (round_f32(np.float32(v) * s) for v in r[n, q])
                if x + w == ex + 1:
                    out["x"].append((si.scale_idx, n, q))
                if y + h == ey + 1:
                    out["y"].append((si.scale_idx, n, q))
    return out


# ----------------------------------------------------------------------------- survivor-heavy cascades
SURVIVOR_SPOTS = ((8, 8, 4, 4), (4, 12, 4, 4))   # (x, y, w, h) in the 20 x 20 window: the selective stages look here
SURVIVOR_SPOT_THRESHOLD = 0.05                    # node threshold of a selective node (times the variance norm factor)
SURVIVOR_FORMS = ("stumps", "trees", "chain_tree", "branch_tree", "accept_all")


def _spot_node(spot: int, thr: float):
    """(rects, weights, threshold) of a node that compares the mean under SURVIVOR_SPOTS[spot] with the window's: rect 0 is
    the whole window (the evaluators set its weight from rect 1's area), rect 1 the spot."""
    return [(0, 0, 20, 20), SURVIVOR_SPOTS[spot], (0, 0, 0, 0)], [-1.0, 1.0, 0.0], thr


def survivor_cascade(form: str = "stumps", n_pass: int = 2):
    """oracle CascadeArrays of a 20 x 20 cascade whose first n_pass stages accept every window (leaves 0 / 1, stage
    threshold -1: far below any sum they reach in either profile), followed by stages that pass a window only when a bright
    pixel lies under a small spot of it (a node threshold that dot_frame()'s dark noise never reaches).  On dot_frame()
    content every window reaches the selective stages; detections follow the dots.

    form: "stumps" (one selective stump stage), "trees" (every stage one two-node tree: the root tests spot 0, its left
    branch spot 1), "chain_tree" (stumps re-linked by as_stage_tree after the prefix: two chains, made of chains),
    "branch_tree" (stumps, a stage tree whose part after the prefix is NOT made of chains: one stage's rejects go to its
    sibling, its parent's to another), "accept_all" (every stage, the last one too, accepts every window)."""
    from oracle.oracle import CascadeArrays
    assert form in SURVIVOR_FORMS and n_pass >= 1
    # stages: [trees], a tree: [(rects, weights, threshold, left, right)] with left / right as in the node arrays
    # (> 0: node index inside the tree, <= 0: -alpha index inside the tree), alphas per tree
    def stump(spot, thr, lo=0.0, hi=1.0):
        rr, ww, t = _spot_node(spot, thr)
        return [(rr, ww, t, 0, -1)], [lo, hi]
    pass_stage = ([stump(0, 0.0)], -1.0)
    if form == "trees":
        r0, w0, t0 = _spot_node(0, SURVIVOR_SPOT_THRESHOLD)
        r1, w1, t1 = _spot_node(1, SURVIVOR_SPOT_THRESHOLD)
        pass_tree = ([(r0, w0, 0.0, 1, 0), (r1, w1, 0.0, -1, -2)], [0.5, 0.0, 1.0])
        sel_tree = ([(r0, w0, t0, 1, 0), (r1, w1, t1, -1, -2)], [1.0, 0.0, 1.0])   # spot 0 bright: 1; else spot 1 decides
        stages = [([pass_tree], -1.0)] * n_pass + [([sel_tree], 0.5)]
    elif form == "accept_all":
        stages = [pass_stage] * (n_pass + 1)
    else:
        sel = [([stump(0, SURVIVOR_SPOT_THRESHOLD)], 0.5), ([stump(1, SURVIVOR_SPOT_THRESHOLD)], 0.5)]
        if form == "stumps":
            stages = [pass_stage] * n_pass + [sel[0]]
        elif form == "chain_tree":           # chains {P, P+2} and {P+1, P+3}: spot 0 then all-pass, or spot 1 then all-pass
            stages = [pass_stage] * n_pass + [sel[0], sel[1], pass_stage, pass_stage]
        else:                                # X = P (spot 0), its children Y1 = P+1 (spot 1), Y2 = P+2 (all-pass); X.next = Z = P+3 (spot 1)
            stages = [pass_stage] * n_pass + [sel[0], sel[1], pass_stage, sel[1]]
    c = CascadeArrays()
    c.win_w = c.win_h = 20
    c.name = f"survivor_{form}_{n_pass}"
    st_first, st_n, st_thr, tr_first, tr_n, tr_alpha = [], [], [], [], [], []
    rects, weights, thr, left, right, alpha = [], [], [], [], [], []
    for trees, sthr in stages:
        st_first.append(len(tr_first))
        st_n.append(len(trees))
        st_thr.append(sthr)
        for nodes, al in trees:
            tr_first.append(len(thr))
            tr_n.append(len(nodes))
            tr_alpha.append(len(alpha))
            for rr, ww, t, lf, rt in nodes:
                rects += [list(r) for r in rr]
                weights += ww
                thr.append(t)
                left.append(lf)
                right.append(rt)
            alpha += al
    n = len(stages)
    c.stage_first_tree = np.array(st_first, np.int32)
    c.stage_n_trees = np.array(st_n, np.int32)
    c.stage_threshold = np.array(st_thr, np.float32)
    c.stage_parent = np.arange(-1, n - 1, dtype=np.int32)
    c.stage_next = np.full(n, -1, np.int32)
    c.stage_child = np.array(list(range(1, n)) + [-1], np.int32)
    c.tree_first_node = np.array(tr_first, np.int32)
    c.tree_n_nodes = np.array(tr_n, np.int32)
    c.tree_first_alpha = np.array(tr_alpha, np.int32)
    c.node_rect = np.array(rects, np.int32).reshape(-1)
    c.node_weight = np.array(weights, np.float32)
    c.node_threshold = np.array(thr, np.float32)
    c.node_left = np.array(left, np.int32)
    c.node_right = np.array(right, np.int32)
    c.node_tilted = np.zeros(len(thr), np.int32)
    c.alpha = np.array(alpha, np.float32)
    if form == "chain_tree":
        c = as_stage_tree(c, split_at=n_pass - 1)
    elif form == "branch_tree":
        p = n_pass
        parent = np.arange(-1, n - 1, dtype=np.int32)
        parent[p + 1] = parent[p + 2] = p
        parent[p + 3] = p - 1
        nxt = np.full(n, -1, np.int32)
        nxt[p], nxt[p + 1] = p + 3, p + 2
        child = np.full(n, -1, np.int32)
        for i in range(n):
            if parent[i] != -1 and child[parent[i]] == -1:
                child[parent[i]] = i
        c.stage_parent, c.stage_next, c.stage_child = parent, nxt, child
    return c


def dot_frame(seed: int, h: int, w: int, n_dots: int, dot: int = 4) -> np.ndarray:
    """A dark frame (16 + uniform noise of 0..16: the variance norm factor stays well above 0) with n_dots bright (255)
    squares of dot x dot pixels at seeded positions.  survivor_cascade()'s selective stages pass only windows with a dot under
    their spot, so the detections follow the dots and the small scales, not the number of windows."""
    rng = np.random.default_rng(seed)
    img = (16 + rng.integers(0, 17, (h, w))).astype(np.uint8)
    for y, x in zip(rng.integers(0, h - dot, n_dots), rng.integers(0, w - dot, n_dots)):
        img[y:y + dot, x:x + dot] = 255
    return img


# ----------------------------------------------------------------------------- a call against the oracle, frame by frame
def rows_of(rects):
    return [tuple(int(r[k]) for k in ("scale_idx", "x", "y", "w", "h")) for r in rects]


def first_difference(got, want):
    s = next(s for s, (x, y) in enumerate(zip(got, want)) if x != y)
    return f"stage {s}: {got[s]} entered, the oracle {want[s]}"


def check_against_oracle(env, c, frames, want, label):
    """One counted and one timed detect of `frames` against the oracle's per-frame results `want`; returns the counted
    result and the oracle's per-stage totals."""
    from clfacedetection_amd import VJ_FLAG_COUNTERS, default_params
    r = env.detect(c, frames, default_params(flags=VJ_FLAG_COUNTERS))
    n_st = c.info.n_stages
    entered, windows = [0] * n_st, 0
    for i, (ro, st) in enumerate(want):
        mine = rows_of(r.rects[r.rects["frame"] == i])
        assert mine == rows_of(ro), f"{label}: frame {i}: {len(mine)} rectangles, the oracle {len(ro)}"
        entered = [x + y for x, y in zip(entered, st["stage_entered"])]
        windows += st["windows"]
    assert r.stage_entered == entered, f"{label}: {first_difference(r.stage_entered, entered)}"
    assert r.windows == windows, f"{label}: {r.windows} windows, the oracle {windows}"
    per_launch = [sum(l["stage_entered"][s] for l in r.launches) for s in range(n_st)]
    assert per_launch == r.stage_entered, f"{label}: per-launch counters do not add up ({first_difference(per_launch, r.stage_entered)})"
    r2 = env.detect(c, frames)
    assert np.array_equal(r2.rects, r.rects), f"{label}: the timed kernels' rectangles differ from the counted ones"
    return r, entered


# ----------------------------------------------------------------------------- every configure key against the oracle
# tests/test_gpu_tunable_parity.py runs the table below cell by cell; tests/soak_gpu.py draws its settings from it.
TUNABLE_KINDS = ("noise", "faces", "blocks")      # every batch is a prefix of one set of DISTINCT frames of these kinds
# name -> (api, cascades, sizes (h, w), batch prefixes, first seed).  api: "clod" vj_detect, "cv" vj_detect_opencv,
# "chain" vj_detect_chain (the cascade's faces grouped with min_neighbors 3, haarcascade_eye inside each) + vj_detect_rois
TUNABLE_WORKLOADS = {
    # >= 800000 px, the second size a multiple of nothing: what one_pass_max_frames applies to
    "lin_few": ("clod", ("frontalface_alt",), ((720, 1280), (750, 1100)), (1, 3), 6000),
    # stumps and two-node trees; 8 and 11 frames take the band-major queue pass, 11 does not divide by the eight queue parts
    "lin_batch": ("clod", ("frontalface_alt", "frontalface_alt2"), ((479, 641),), (1, 8, 11), 6100),
    # the one shipped stage tree: prefix 0..4, then two chains of about twenty stages each
    "tree": ("clod", ("frontalface_alt_tree",), ((480, 640),), (1, 3, 9), 6200),
    "cv_tree": ("cv", ("frontalface_alt_tree",), ((480, 640),), (1, 5), 6300),   # (tree_queue == 1 at the defaults: asserted)
    "cv_lin": ("cv", ("frontalface_alt",), ((480, 640),), (1, 5), 6400),
    "cv_lin2": ("cv", ("frontalface_alt2",), ((300, 420),), (1, 5), 6500),       # two-node trees (cv_tree2)
    "cv_tilted": ("cv", ("fullbody",), ((300, 420),), (1, 5), 6600),             # tilted features (cv_tiles_tilted)
    "regions": ("chain", ("frontalface_alt2",), ((360, 640),), (2, 4), 6700),    # (frame 1 is the first drawn-faces frame)
}


class Sweep:
    """Values of one key (all different from its default, in configure's syntax), the workloads that reach the code the key
    steers, and settings applied before it when the key only acts next to them."""
    def __init__(self, values, *workloads, also=()):
        self.values, self.workloads, self.also = tuple(values), tuple(workloads), tuple(also)


TUNABLE_SWEEPS = {
    # ---- launch structure
    "pass_split": [Sweep(("3", "3,9", "2,5,12"), "lin_batch")],
    # asserted: r.passes are the rule's (cumulative nodes) for the value and differ from the default's
    "pass_cut_nodes": [Sweep(("150", "7", "35,150", "-1"), "lin_batch")],
    "blocks_per_cu": [Sweep(("1", "3"), "lin_batch", "tree")],
    "concurrent": [Sweep(("0",), "lin_batch", "tree", "cv_lin", "cv_tree")],
    # asserted: a tile, a grid and a queue launch exist and the queue launch entered windows (the grid's size is not reported)
    "concurrent_blocks_per_cu": [Sweep(("2", "8"), "lin_batch")],
    "max_subbatch": [Sweep(("2", "3"), "lin_batch", "cv_lin")],
    "det_cap": [Sweep(("1", "7"), "lin_batch", "tree", "regions")],                 # the regrow path
    # ---- LDS tiles
    "tile_classes_kb": [Sweep(("0,0,0", "24,40,60"), "lin_batch", "tree")],
    "tile_lds_reserve_kb": [Sweep(("0", "48"), "lin_batch")],
    "tile_min_windows": [Sweep(("64", "2048"), "lin_batch")],
    # asserted: the scales of the tile launches differ from the default's
    "tile_accept_windows": [Sweep(("0", "65536"), "lin_batch")],
    "tile_max_dwords_per_window": [Sweep(("100", "8000"), "lin_batch")],
    "tile_end": [Sweep(("2", "3", "5"), "lin_batch")],
    "tile_min_lanes": [Sweep(("64", "512"), "lin_batch")],
    "tile_repack": [Sweep(("3,5", ""), "lin_batch")],
    "tile_sp_begin": [Sweep(("64", "5"), "lin_batch")],
    "tile_ws_min": [Sweep(("0", "256"), "lin_batch")],
    "tile_ws_max": [Sweep(("0", "100"), "lin_batch")],
    # ---- chain balance
    "tile_split": [Sweep(("0", "0.5", "0,1.5,2"), "lin_batch")],                    # a static split
    "auto_balance": [Sweep(("0",), "lin_batch")],
    # ---- global-gather chain
    "grid_block_w": [Sweep(("0", "16"), "lin_batch", "tree")],
    # 3 on 8 and 11 frames and 4 on one frame are the pairings the default never makes; the kernels take 1 and 2 as well (every
    # index is per wave, blockDim gives the waves per workgroup).  asserted: a queue launch entered windows
    "gather_waves": [Sweep(("1", "2", "3", "4"), "lin_batch")],
    "gather_pairs": [Sweep(("0", "1", "2"), "lin_batch")],
    "sp_tail_max": [Sweep(("0", "16"), "lin_batch", "tree")],
    "wide_tail": [Sweep(("0", "1"), "lin_batch")],
    "min_chunk": [Sweep(("64", "5"), "lin_batch", "tree")],
    # the slices belong to the chunk-by-chunk queue pass: one frame at the defaults, every batch with q_band_px 0.
    # asserted: a queue launch entered windows (which walk it took is not reported)
    "q_slices": [Sweep(("1", "5"), "lin_batch"), Sweep(("1", "5"), "lin_batch", also=(("q_band_px", "0"),))],
    "q_band_px": [Sweep(("0", "32", "700"), "lin_batch")],
    "q_group_units": [Sweep(("1", "16"), "lin_batch")],
    "q_band_min_frames": [Sweep(("1", "2"), "lin_batch")],
    # ---- stage trees
    "general_prefix": [Sweep(("0",), "tree")],
    "tile_segments": [Sweep(("0",), "tree")],
    # asserted: r.passes are the planner's rule — every chain longer than value + 4 stages gets a boundary at its start + value
    # (8, 4); 3 (not > 3) and 40 (no chain that long) leave the passes alone.  tile_segments and tree_split_queues choose who
    # feeds the new pass
    "seg_cut2": [Sweep(("8", "4", "3", "40"), "tree"), Sweep(("8",), "tree", also=(("tile_segments", "0"),)),
                 Sweep(("8",), "tree", also=(("tree_split_queues", "0"),))],
    "tree_split_queues": [Sweep(("0",), "tree")],
    # ---- regions / chain (which route a call took is not visible in its result)
    "rois_on_device": [Sweep(("0",), "regions")],
    "roi_tiles": [Sweep(("64", "0"), "regions")],
    "group_max": [Sweep(("30", "50"), "regions")],
    # ---- OpenCV profile
    "cv_tiles": [Sweep(("0",), "cv_lin", "cv_tree")],
    "cv_row_blocks": [Sweep(("1", "3"), "cv_lin", "cv_lin2")],
    "cv_tile_min_windows": [Sweep(("64", "256"), "cv_lin", "cv_lin2")],
    "cv_tile_min_windows0": [Sweep(("64", "512"), "cv_lin", "cv_tree")],
    "cv_tile_ws_max": [Sweep(("0", "100"), "cv_lin")],
    # asserted for the three tree-queue keys: the plan has tile scales and takes the chain pass over the tree queue
    # (tree_queue == 1), or the flat queue (2) next to cv_tree_chains 0
    "cv_row_blocks_tree": [Sweep(("1", "4"), "cv_tree")],
    # asserted: the plan's number of tile scales differs from the default's
    "cv_tile_min_windows_tree": [Sweep(("64", "2048"), "cv_tree")],
    "cv_tree_chains": [Sweep(("0",), "cv_tree")],
    # (64 is the default and runs as the default call of every cell; 100 is not a multiple of the wave; 256 is the most the chain
    # pass takes)
    "cv_tree_chunk": [Sweep(("100", "256"), "cv_tree"), Sweep(("100",), "cv_tree", also=(("cv_tree_chains", "0"),))],
    "cv_tree_chain_blocks": [Sweep(("1", "4"), "cv_tree")],
    "cv_tail_max": [Sweep(("0", "20"), "cv_lin", "cv_tree")],
    "cv_row_band_px": [Sweep(("0", "37"), "cv_lin", "cv_tree")],
    "cv_tree2": [Sweep(("0",), "cv_lin2")],
    "cv_tiles_tilted": [Sweep(("0",), "cv_tilted")],
    "cv_tree_queue_cap": [Sweep(("16", "100000"), "cv_tree")],                      # 16 overflows: the call falls back to the rows
    # ---- single frames, integral, housekeeping
    # asserted: for n_frames <= value the gather chain is ONE grid pass over [0, n_stages) and no queue launch; with more
    # frames the default passes (the other refusals: test_one_pass_refusals_keep_the_default_passes)
    "one_pass_max_frames": [Sweep(("1", "4"), "lin_few")],
    "integral_rows": [Sweep(("0", "1"), "lin_batch", "cv_lin")],
    "plan_cache_max": [Sweep(("2",), "lin_batch", "regions")],                      # the chain holds two plans at once
}


# ----------------------------------------------------------------------------- arithmetic edges: stage sums, variances, sums
# tests/test_arithmetic_cases_cpu.py proves on the CPU that these inputs are decisive; tests/test_gpu_arithmetic_edges.py runs
# them through every path.  Both walk ORDER_CELLS / TIE_CELLS.
ORDER_FORMS = ("stumps", "trees", "two_stage", "huge")
ORDER_PREFIX = 3            # stages in front of the decisive one(s): accept-all, thinning, accept-all
THIN_STUMPS = 4             # the thinning stage passes a window when all of its stumps say yes: 1 in 16 on noise


def _small_spot(k: int):
    """The k-th 3 x 3 spot of the 20 x 20 window (18 x 18 positions, visited with a stride coprime to 324)."""
    p = (k * 89 + 7) % 324
    return (p % 18, p // 18, 3, 3)


def _mean_node(spot, left, right):
    """A node that compares the mean under `spot` with the window's at node threshold 0 (rect 0 is the whole window: the
    evaluators set its weight from rect 1's area)."""
    return ([(0, 0, 20, 20), spot, (0, 0, 0, 0)], [-1.0, 1.0, 0.0], 0.0, left, right)


def _linear_cascade(name: str, stages):
    """oracle CascadeArrays of a linear 20 x 20 cascade.  stages: [(trees, stage threshold)], a tree: (nodes, leaf values),
    a node: (rects, weights, threshold, left, right) with left / right as in the node arrays."""
    from oracle.oracle import CascadeArrays
    c = CascadeArrays()
    c.win_w = c.win_h = 20
    c.name = name
    st_first, st_n, st_thr, tr_first, tr_n, tr_alpha = [], [], [], [], [], []
    rects, weights, thr, left, right, alpha = [], [], [], [], [], []
    for trees, sthr in stages:
        st_first.append(len(tr_first))
        st_n.append(len(trees))
        st_thr.append(sthr)
        for nodes, al in trees:
            tr_first.append(len(thr))
            tr_n.append(len(nodes))
            tr_alpha.append(len(alpha))
            for rr, ww, t, lf, rt in nodes:
                rects += [list(r) for r in rr]
                weights += ww
                thr.append(t)
                left.append(lf)
                right.append(rt)
            alpha += list(al)
    n = len(stages)
    c.stage_first_tree = np.array(st_first, np.int32)
    c.stage_n_trees = np.array(st_n, np.int32)
    c.stage_threshold = np.array(st_thr, np.float32)
    c.stage_parent = np.arange(-1, n - 1, dtype=np.int32)
    c.stage_next = np.full(n, -1, np.int32)
    c.stage_child = np.array(list(range(1, n)) + [-1], np.int32)
    c.tree_first_node = np.array(tr_first, np.int32)
    c.tree_n_nodes = np.array(tr_n, np.int32)
    c.tree_first_alpha = np.array(tr_alpha, np.int32)
    c.node_rect = np.array(rects, np.int32).reshape(-1)
    c.node_weight = np.array(weights, np.float32)
    c.node_threshold = np.array(thr, np.float32)
    c.node_left = np.array(left, np.int32)
    c.node_right = np.array(right, np.int32)
    c.node_tilted = np.zeros(len(thr), np.int32)
    c.alpha = np.array(alpha, np.float32)
    return c


def _thinning_prefix(trees: bool = False):
    """Stage 0 accepts every window (the decisive stage is not stage 0, and the OpenCV profile's walk never skips a
    window), stage 1 passes one window in sixteen on noise (all THIN_STUMPS spots brighter than the window's mean), stage 2
    accepts every window again.  The tile kernel's wave-split finish and wave-independent tail — where a stage's leaves are
    added in another order than the reference's — take a tile over at a re-pack point at or after tile_sp_begin (3) once at
    most tile_ws_max (512) of its up to 2048 windows are left: the thinning stage is what gets the decisive stage there.
    trees: the same verdicts from two-node trees (the root decides; both leaves of its child are 0), because the kernels'
    two-node forms (TREE2, cv_tree2) are only taken by cascades made of such trees throughout."""
    def item(k):
        if trees:
            return ([_mean_node(_small_spot(k), 1, 0), _mean_node(_small_spot(k + 7), -1, -2)], [1.0, 0.0, 0.0])
        return ([_mean_node(_small_spot(k), 0, -1)], [0.0, 1.0])
    all_pass = ([item(300)], -1.0)
    thin = ([item(310 + k) for k in range(THIN_STUMPS)], THIN_STUMPS - 0.5)
    return [all_pass, thin, all_pass]


def _median_in_order(values, dtype):
    """Median attained running sum (dtype additions, column order) of the rows of `values`."""
    from oracle.np_oracle import in_order_sum
    s = in_order_sum(values, dtype)
    return np.sort(s)[len(s) // 2]


def _order_stage(rng, form: str, n: int, spot0: int):
    """One decisive stage of order_cascade: ([trees], threshold)."""
    f32 = np.float32
    if form == "huge":
        # three classes: around 2^100 (both leaves equal: the part every window shares, which takes the running f64 sum to
        # where one ulp is 2^48 and more), around 2^60 (right = left + j 2^48: the lattice of attained sums, whose low bits
        # the large partial sums round away in an order-dependent way) and around 1 (lost in every order)
        cls = rng.choice(3, n, p=[0.3, 0.55, 0.15])
        left = (np.array([2.0 ** 100, 2.0 ** 60, 1.0])[cls] * rng.uniform(1, 2, n) * rng.choice([-1, 1], n)).astype(f32)
        top = np.nonzero(cls == 0)[0]
        left[top[1::2]] = -left[top[0:2 * (len(top) // 2):2]]      # the large leaves cancel in pairs: the sum ends near 2^63,
        if len(top) % 2:                                           # where a float threshold is fine enough
            left[top[-1]], cls[top[-1]] = f32(2.0 ** 60), 1
        step = np.array([0.0, 2.0 ** 48, 1.0])[cls]
        extra = [(left + rng.integers(1, 64, n) * step).astype(f32) for _ in range(2)]
    else:
        left = (rng.choice([3000.0, 700.0, 90.0, 11.0], n) * rng.choice([-1, 1], n) + rng.uniform(-1, 1, n)).astype(f32)
        coarse = rng.choice(n, min(14, n), replace=False)
        extra = []
        for _ in range(2):
            if n < 16:   # a handful of items: the band is a few ulps of the sum, so the leaves differ by 1..3 of them
                r = (left + rng.integers(1, 4, n) * np.spacing(f32(np.abs(left).sum()))).astype(f32)
            else:
                r = (left + rng.integers(1, 64, n) * f32(2.0 ** -12)).astype(f32)
                r[coarse] = (left[coarse] + rng.integers(1, 64, len(coarse)) * f32(2.0 ** -9)).astype(f32)
            extra.append(r)
    # the threshold: the median attained in-order sum under independent fair bits (what the nodes give on noise), in the
    # arithmetic of the profile the form is for (f64 for "huge", else f32)
    sim = 20000
    if form == "trees":      # root right: leaf 0; root left -> child: leaves 1 / 2
        code = rng.choice(3, (sim, n), p=[0.5, 0.25, 0.25])
        leaves = np.stack([left, extra[0], extra[1]], 1)                 # (n, 3)
        vals = leaves[np.arange(n)[None, :], code]
        trees = [([_mean_node(_small_spot(spot0 + 2 * k), 1, 0), _mean_node(_small_spot(spot0 + 2 * k + 1), -1, -2)],
                  [float(v) for v in leaves[k]]) for k in range(n)]
    else:
        vals = np.where(rng.integers(0, 2, (sim, n)).astype(bool), extra[0][None, :], left[None, :])
        trees = [([_mean_node(_small_spot(spot0 + k), 0, -1)], [float(left[k]), float(extra[0][k])]) for k in range(n)]
    thr = _median_in_order(vals, np.float64 if form == "huge" else f32)
    return trees, float(f32(thr))


def order_cascade(form: str, n: int, seed: int = 0):
    """oracle CascadeArrays of a 20 x 20 cascade whose decisive stage (index ORDER_PREFIX) has n stumps — n two-node trees
    for "trees" — whose running sum depends on the order of addition, behind _thinning_prefix().  Every item compares its
    own 3 x 3 spot with the window's mean at node threshold 0, so on noise the verdict bits are close to independent and
    every window takes its own rounding path.  Leaves: a magnitude from {3000, 700, 90, 11} +- 1 with a random sign on the
    left, the left one plus a small multiple of 2^-12 (for up to 14 items 2^-9) on the right; the stage threshold is the
    median attained in-order sum, so the attained sums form a fine lattice around it and every window lies within sp_delta
    of it.  "two_stage": two such stages in a row (the survivors of a replayed stage enter another one).  "huge": leaves
    around +-2^100, +-2^60 and +-1, for which the f64 sum of the OpenCV profile depends on the order too; sp_delta is
    about 2^90 there, still a finite float."""
    assert form in ORDER_FORMS and 1 <= n <= 256
    rng = np.random.default_rng([seed, n, ORDER_FORMS.index(form)])
    stages = _thinning_prefix(form == "trees") + [_order_stage(rng, form, n, 0)]
    if form == "two_stage":
        stages.append(_order_stage(rng, form, n, 150))
    return _linear_cascade(f"order_{form}_{n}_{seed}", stages)


TIE_STUMPS = 70


def tie_cascade(strict: bool = False, seed: int = 0):
    """Like order_cascade("stumps", 70), with leaves that are multiples of 2^-6 of magnitude <= 2: every order of addition
    gives the same exact sum, the attained sums lie 2^-6 apart and sp_delta (about 8e-4) is far below that, so a window is
    inside the band only when its sum EQUALS the threshold.  strict=False: the stage threshold is an attained sum (those
    windows pass: sum >= thr); strict=True: the next float above it (the same windows fail)."""
    rng = np.random.default_rng([seed, 4242])
    n = TIE_STUMPS
    left = rng.integers(-96, 97, n) / 64.0
    right = np.clip(left + rng.integers(1, 9, n) * rng.choice([-1, 1], n) / 64.0, -2.0, 2.0)
    vals = np.where(rng.integers(0, 2, (20000, n)).astype(bool), right[None, :], left[None, :])
    thr = np.float32(_median_in_order(vals, np.float32))
    if strict:
        thr = np.nextafter(thr, np.float32(np.inf))
    trees = [([_mean_node(_small_spot(k), 0, -1)], [float(left[k]), float(right[k])]) for k in range(n)]
    return _linear_cascade(f"tie_{'gt' if strict else 'ge'}_{seed}", _thinning_prefix() + [(trees, float(thr))])


def sp_delta(c, stage: int) -> np.float32:
    """The documented band of a stage: 4 n 2^-24 sum over trees of max|leaf| * 1.001 + 1e-30 (n: the stage's nodes), as a float."""
    t0, nt = int(c.stage_first_tree[stage]), int(c.stage_n_trees[stage])
    amax = sum(float(np.abs(c.alpha[int(c.tree_first_alpha[t]):int(c.tree_first_alpha[t]) + int(c.tree_n_nodes[t]) + 1].astype(np.float64)).max())
               for t in range(t0, t0 + nt))
    n = sum(int(c.tree_n_nodes[t]) for t in range(t0, t0 + nt))
    return np.float32(4.0 * n * 2.0 ** -24 * amax * 1.001 + 1e-30)


def alternative_orders(n: int):
    """{name: function(leaves (windows, n), dtype) -> sums}: the orders in which the kernels add a stage's n leaf values
    when they do not follow the reference — reversed; a butterfly inside balanced blocks of up to 64, the blocks in order
    (tile_wave_tail); K even ranges, each in order, for K in 2, 4, 8 (tile_wave_split) — leaving out those whose sequence of
    additions IS the reference's for this n (K ranges of one range, or whose second range is empty)."""
    from oracle.np_oracle import in_order_sum as in_order

    def butterfly(v, dt):
        nb = (n + 63) // 64
        out, jb = np.zeros(len(v), dt), 0
        for b in range(nb):
            jn = n // nb + (1 if b < n % nb else 0)
            x = np.zeros((len(v), 64), dt)
            x[:, :jn] = v[:, jb:jb + jn]
            jb += jn
            w = 64
            while w > 1:
                x = (x[:, :w // 2] + x[:, w // 2:w]).astype(dt)
                w //= 2
            out = (out + x[:, 0]).astype(dt)
        return out

    def ranges(K):
        rs = ((n + K - 1) // K + 1) & ~1
        def f(v, dt):
            out = np.zeros(len(v), dt)
            for j0 in range(0, n, rs):
                out = (out + in_order(v[:, j0:j0 + rs], dt)).astype(dt)
            return out
        return rs, f
    orders = {"reversed": lambda v, dt: in_order(v[:, ::-1], dt), "butterfly": butterfly}
    for K in (2, 4, 8):
        rs, f = ranges(K)
        if n - rs >= 2:   # a second range of one value adds it last, as the running sum does
            orders[f"ranges{K}"] = f
    return orders


def near_flat_frame(seed: int, h: int, w: int, level: int, n_off: int) -> np.ndarray:
    """A constant frame of grey `level` with n_off pixels one level off (below at 255, above otherwise): in most windows
    the f32 expression Q / area - mean * mean cancels to a small negative, zero or positive value."""
    rng = np.random.default_rng([seed, level])
    img = np.full((h, w), level, np.uint8)
    flat = rng.choice(h * w, n_off, replace=False)
    img.reshape(-1)[flat] = level - 1 if level == 255 else level + 1
    return img


BRIGHT_SIDE = 4608


def bright_frame(seed: int, side: int = BRIGHT_SIDE) -> np.ndarray:
    """side x side pixels of 230..255 (noise of 230..235 under three large drawn faces): the sum integral passes 2^32 (side^2 * 242.5 = 5.1e9 at 4608) and the largest windows
    hold more than 2^31, where VJ_FLAG_SIGNED_MEAN reads the sum as negative.  The profiles accept about 32 k a side
    ((W + 1)(H + 3) < 2^30); such a frame is 1 GiB and its integrals 12 GiB in the oracle, so the side is the smallest round
    one that meets both premises with room to spare (tests/test_arithmetic_cases_cpu.py asserts them)."""
    img = np.random.default_rng([seed, side]).integers(230, 236, (side, side), dtype=np.uint8)
    # drawn faces as large as the largest windows, their contrast pressed into 236..255: on plain noise every large window
    # fails stage 0 with or without the flag; a face takes windows deep into the cascade, where the norm factor decides
    for size, at in ((3437, 300), (3781, 500), (4159, 200)):
        face = np.clip(synth.crude_face(size), 0, 255) * (19.0 / 255.0)
        img[at:at + size, at:at + size] = np.maximum(img[at:at + size, at:at + size], (236 + face).astype(np.uint8))
    return img


# (id, form, n, cascade seed, (h, w), first frame seed): batches are the first 1 and all ARITH_FRAMES noise frames
ARITH_FRAMES = 8
ORDER_CELLS = [
    ("stumps3", "stumps", 3, 5, (240, 320), 100),
    ("stumps64", "stumps", 64, 0, (240, 320), 110),
    ("stumps65", "stumps", 65, 0, (240, 320), 120),
    ("stumps130", "stumps", 130, 0, (240, 320), 130),
    ("stumps200", "stumps", 200, 0, (240, 320), 140),
    ("trees65", "trees", 65, 0, (240, 320), 150),
    ("trees130", "trees", 130, 0, (240, 320), 160),
    ("two_stage130", "two_stage", 130, 0, (240, 320), 170),
    ("huge130", "huge", 130, 7, (240, 320), 180),
]
TIE_CELLS = [("tie_ge", False, 0, (240, 320), 190), ("tie_gt", True, 0, (240, 320), 190)]


def arith_frames(size, seed0: int, n: int = ARITH_FRAMES) -> np.ndarray:
    return np.stack([synth.frame("noise", seed0 + k, size[0], size[1]) for k in range(n)])


# (id, cascade — a shipped one or ("geometry", win, kind) —, (h, w), pixels off): a cell's frames are near_flat_frame at each
# of NEAR_FLAT_LEVELS (seed = the level's index), one batch of distinct frames
NEAR_FLAT_LEVELS = (255, 128, 1)
NEAR_FLAT_CELLS = [
    ("alt", "frontalface_alt", (150, 200), 60),
    ("alt2", "frontalface_alt2", (150, 200), 60),
    ("alt_tree", "frontalface_alt_tree", (150, 200), 60),
    ("geometry", ("geometry", (24, 24), "upright"), (150, 200), 60),
    ("alt_sparse", "frontalface_alt", (131, 177), 25),
]


def near_flat_frames(size, n_off: int) -> np.ndarray:
    return np.stack([near_flat_frame(k, size[0], size[1], level, n_off) for k, level in enumerate(NEAR_FLAT_LEVELS)])


BRIGHT_MIN = 3000           # min_w / min_h of the bright-frame calls: the five largest scales (windows of 3125 .. 4575 pixels)
BRIGHT_CASCADES = ("frontalface_alt", "frontalface_alt_tree")


# ----------------------------------------------------------------------------- cascade topologies
# Cascade SHAPES on each side of the planners' and kernels' fixed-size assumptions ("Fixed-size assumptions"):
# stage counts around VJ_MAX_STAGES, stage widths around the two stump-parallel tails, node trees beyond {root, child}, stage
# trees around CvChainDev::begin[4] / CascadeArgs::seg_end[4] and VJ_MAX_PASSES.  tests/test_topology_cases_cpu.py proves the
# premises on the oracle alone and keeps the table on both sides of every limit; tests/test_gpu_topologies.py runs every case
# through every entry point that takes a cascade.  These are structure tests, not rounding tests: every leaf is a multiple of
# 2^-6 of magnitude <= 2 (as in tie_cascade), so every order of addition gives the same exact sum, and every stage threshold
# lies halfway between two attained sums.
TOPOLOGY_SIZE = (240, 320)
# (stumps, how many must say yes): 1/2, 1/2, 5/16 and 11/16 of the windows on noise; the fifth form, 1/16, is for the cascades
# too short to get below a tenth of the windows with the others (lin1, lin2)
TOPOLOGY_SEL_FORMS = ((1, 1), (3, 2), (4, 3), (4, 2), (4, 4))
TOPOLOGY_WIDE_STAGE = ORDER_PREFIX                      # index of the decisive stage of the w* cases
_TOPOLOGY, _TOPOLOGY_CHAINS = {}, {}


class _Spots:
    """Hands every node a 3 x 3 spot of its own (_small_spot visits the 324 positions before it repeats)."""
    def __init__(self, first: int = 0):
        self.k = first

    def take(self):
        self.k += 1
        return _small_spot(self.k - 1)


def _stump(sp, lo=0.0, hi=1.0):
    return ([_mean_node(sp.take(), 0, -1)], [lo, hi])


def _all_stage(sp):
    """Accepts every window: one stump with leaves 0 / 1 under a stage threshold of -1."""
    return ([_stump(sp)], -1.0)


def _sel_stage(sp, form: int = 0):
    """`n` mean-vs-spot stumps with leaves 0 / 1, `need` of which must say yes: the threshold need - 0.5 lies halfway between
    two attained sums."""
    n, need = TOPOLOGY_SEL_FORMS[form]
    return ([_stump(sp) for _ in range(n)], need - 0.5)


def _sel_stage_tree2(sp):
    """A selective stage of two {root, child at index 1} trees: a tree says yes when its root's spot is
    dark and its child's is bright (1 in 4 on noise); one of the two is enough (7 in 16)."""
    def tree():
        return ([_mean_node(sp.take(), 1, 0), _mean_node(sp.take(), -1, -2)], [0.0, 0.0, 1.0])
    return ([tree(), tree()], 0.5)


# node trees: (left, right) per node, > 0 a node of the tree, <= 0 minus a leaf index; leaves are numbered in the order in
# which a reader of the XML meets them (icvReadHaarClassifier), node by node, left before right
def _shape_links(shape: str):
    if shape == "stump":
        return [(0, -1)]
    if shape == "tree2":                       # the child hangs on the root's left branch
        return [(1, 0), (-1, -2)]
    if shape == "tree2r":                      # ... on its right branch
        return [(0, 1), (-1, -2)]
    if shape == "tree3y":                      # a root with two internal children
        return [(1, 2), (0, -1), (-2, -3)]
    if shape == "tree7":                       # the full binary tree of 7 nodes and 8 leaves
        return [(1, 2), (3, 4), (5, 6), (0, -1), (-2, -3), (-4, -5), (-6, -7)]
    if shape == "spine15":                     # each node's left branch is the next node
        return [(k + 1, -k) for k in range(14)] + [(-14, -15)]
    raise ValueError(shape)


def _tree_values(links, leaves, bits):
    """The leaf value every row of `bits` (rows x nodes; 1: the node's sum reaches its threshold, the walk goes right) ends on."""
    left = np.array([l for l, _ in links])
    right = np.array([r for _, r in links])
    rows = np.arange(len(bits))
    cur = np.zeros(len(bits), np.int64)
    leaf = np.zeros(len(bits), np.int64)
    active = np.ones(len(bits), bool)
    for _ in links:
        nxt = np.where(bits[rows, cur] != 0, right[cur], left[cur])
        done = active & (nxt <= 0)
        leaf[done] = -nxt[done]
        active &= nxt > 0
        cur = np.where(active, nxt, cur)
    return np.asarray(leaves)[leaf]


def _midpoint_threshold(sums) -> float:
    """Halfway between the median attained sum and the attained sum below it."""
    u = np.unique(sums)
    m = int(np.searchsorted(u, np.sort(sums)[len(sums) // 2]))
    m = max(m, 1)
    return float(np.float32((u[m] + u[m - 1]) / 2.0))


def _tree_stage(rng, sp, shapes):
    """A stage of node trees of the given shapes, leaves seeded multiples of 2^-6 in [-1.5, 1.5]; the stage threshold is the
    midpoint below the median sum under independent fair node bits (what the spots give on noise)."""
    trees, total = [], np.zeros(4000)
    for shape in shapes:
        links = _shape_links(shape)
        leaves = rng.permutation(np.arange(-96, 97))[:len(links) + 1] / 64.0      # distinct: every leaf can be told from the others
        trees.append(([_mean_node(sp.take(), l, r) for l, r in links], [float(v) for v in leaves]))
        total = total + _tree_values(links, leaves, rng.integers(0, 2, (4000, len(links))))
    return trees, _midpoint_threshold(total)


def _wide_stage(rng, sp, n: int):
    """One decisive stage of n stumps with tie_cascade's leaves (no limit on n: the 324 spots repeat)."""
    left = rng.integers(-96, 97, n) / 64.0
    right = np.clip(left + rng.integers(1, 9, n) * rng.choice([-1, 1], n) / 64.0, -2.0, 2.0)
    spots = [sp.take() for _ in range(n)]
    first = {}
    bits = rng.integers(0, 2, (4000, n))
    for k, s in enumerate(spots):            # a repeated spot gives the same verdict
        bits[:, k] = bits[:, first.setdefault(s, k)]
    sums = np.where(bits != 0, right[None, :], left[None, :]).sum(1)
    trees = [([_mean_node(spots[k], 0, -1)], [float(left[k]), float(right[k])]) for k in range(n)]
    return trees, _midpoint_threshold(sums)


def _link_stages(c, parent, nxt):
    """Sets parent / next and the child links icvReadHaarClassifier would have set (a stage's first child by index)."""
    n = c.n_stages
    child = np.full(n, -1, np.int32)
    for i in range(n):
        if parent[i] != -1 and child[parent[i]] == -1:
            child[parent[i]] = i
    c.stage_parent, c.stage_next, c.stage_child = np.array(parent, np.int32), np.array(nxt, np.int32), child
    return c


def _stage_tree(name: str, n_prefix: int, chain_lens, stage=_sel_stage, forms=None):
    """A prefix of n_prefix stages and chains of the given lengths, all children of the prefix's last stage (of nothing
    without a prefix); each chain's first stage has the next chain's first stage as its `next`, so a reject anywhere in a
    chain starts the next chain.  A chain's last stage has no child.  Returns (CascadeArrays, [(first, end) of every chain])."""
    sp = _Spots()
    n = n_prefix + sum(chain_lens)
    if forms:                         # (None: a stage that accepts every window)
        stages = [_all_stage(sp) if forms[i] is None else _sel_stage(sp, forms[i]) for i in range(n)]
    else:
        stages = [stage(sp, i % 4) if stage is _sel_stage else stage(sp) for i in range(n)]
    c = _linear_cascade(name, stages)
    parent, nxt = [-1] * n, [-1] * n
    for i in range(1, n_prefix):
        parent[i] = i - 1
    chains, b = [], n_prefix
    for ln in chain_lens:
        chains.append((b, b + ln))
        parent[b] = n_prefix - 1
        for i in range(b + 1, b + ln):
            parent[i] = i - 1
        b += ln
    for (b0, _), (b1, _) in zip(chains, chains[1:]):
        nxt[b0] = b1
    return _link_stages(c, parent, nxt), chains


def _build_topology(case_id: str):
    sp = _Spots()
    rng = np.random.default_rng([9000, sum(case_id.encode())])
    name = "topology_" + case_id
    if case_id.startswith("lin"):
        n = int(case_id[3:])
        sel = {0: 0, 1: 1, n // 2 - 1: 2, n - 2: 3, n - 1: 0} if n >= 64 else dict(enumerate({1: [4], 2: [1, 4], 3: [0, 1, 2]}[n]))
        return _linear_cascade(name, [_sel_stage(sp, sel[i]) if i in sel else _all_stage(sp) for i in range(n)]), []
    if case_id.startswith("w"):
        widths = [int(v) for v in case_id[1:].split("x")]
        widths = widths[:1] * (widths[1] if len(widths) > 1 else 1)
        sp.k = 20                         # (the thinning prefix has spots of its own, 300 and up)
        return _linear_cascade(name, _thinning_prefix() + [_wide_stage(rng, sp, w) for w in widths]), []
    node_trees = {"tree3y": [["tree3y"] * 3] * 5, "tree7": [["tree7"] * 3] * 5, "spine15": [["spine15"] * 3] * 5,
                  "tree2r": [["tree2r"] * 4] * 5,
                  "mixed": [["stump", "tree2", "tree7"], ["tree7", "stump", "stump", "tree2"], ["tree2", "tree7", "stump"],
                            ["stump", "tree7", "tree2", "stump"], ["tree7", "tree2", "stump"]]}
    if case_id in node_trees:
        return _linear_cascade(name, [_tree_stage(rng, sp, shapes) for shapes in node_trees[case_id]]), []
    stage_trees = {"st_root": (0, (3, 3)), "st_p1": (1, (3, 3)), "st_c3": (3, (2, 2, 2)), "st_c4": (3, (2, 2, 2, 2)),
                   "st_c5": (3, (2, 2, 2, 2, 2)), "st_c3long": (3, (6, 6, 6)), "st_c4long": (3, (6, 6, 6, 6)),
                   "st_c1": (3, (1, 6, 1))}
    if case_id == "st_root":              # (5 in 16 a stage: two chains of three loose stages accept more than a tenth of the windows)
        return _stage_tree(name, *stage_trees[case_id], forms=[2] * 6)
    if case_id in stage_trees:
        return _stage_tree(name, *stage_trees[case_id])
    if case_id == "st_64":                # VJ_MAX_STAGES stages in a stage tree: the 64-bit "entered" masks of the OpenCV-profile kernels carry
        # bits 32 .. 63 only there.  Prefix 0 1 2, chains 3 .. 32 and 33 .. 63; selective: the prefix, each chain's first and last two stages
        forms = [0, 1, 2] + [0] + [None] * 27 + [1, 0] + [0] + [None] * 28 + [1, 0]
        return _stage_tree(name, 3, (30, 31), forms=forms)
    if case_id == "st_tree2":
        return _stage_tree(name, *stage_trees["st_c4"], stage=_sel_stage_tree2)
    if case_id == "st_dead":              # st_c3 and a tenth stage that nothing points to (a second root without a `next` leading to it)
        c, chains = _stage_tree(name, *stage_trees["st_c3"])
        d = _linear_cascade(name, [_sel_stage(sp, i % 4) for i in range(10)])   # (the first nine: st_c3's own stages)
        return _link_stages(d, list(c.stage_parent) + [-1], list(c.stage_next) + [-1]), chains
    if case_id == "st_cycle":             # st_c3 whose last chain's rejects go back to the first chain
        c, chains = _stage_tree(name, *stage_trees["st_c3"])
        c.stage_next[chains[-1][0]] = chains[0][0]
        return c, chains
    if case_id == "st_nested":
        # prefix 0 1 2; the first chain 3 4 5; stage 4 has a sibling list of its own, 6 7 (children of 3): a reject at 4 or 5
        # goes to 6, one at 3, 6 or 7 to the second chain 8 9 (a child of 2, the `next` of 3)
        c = _linear_cascade(name, [_sel_stage(sp, i % 4) for i in range(10)])
        parent = [-1, 0, 1, 2, 3, 4, 3, 6, 2, 8]
        nxt = [-1, -1, -1, 8, 6, -1, -1, -1, -1, -1]
        return _link_stages(c, parent, nxt), [(3, 6), (6, 8), (8, 10)]
    raise KeyError(case_id)


def topology_cascade(case_id: str):
    """oracle CascadeArrays of one topology case (built once; callers copy before they change anything)."""
    if case_id not in _TOPOLOGY:
        _TOPOLOGY[case_id], _TOPOLOGY_CHAINS[case_id] = _build_topology(case_id)
    return _TOPOLOGY[case_id]


def topology_chains(case_id: str):
    """[(first stage, end stage)] of a stage-tree case's chains ([] for the others)."""
    topology_cascade(case_id)
    return list(_TOPOLOGY_CHAINS[case_id])


# (id, family, (h, w), first frame seed, runnable): frames are arith_frames(size, seed) — a batch of ARITH_FRAMES distinct
# 240 x 320 noise frames, and its first frame alone.  Not runnable: lin65 (more than VJ_MAX_STAGES stages) and st_cycle are
# refused by every entry point.  No case needed another frame set or size.
TOPOLOGY_CELLS = [
    ("lin1", "linear", TOPOLOGY_SIZE, 300, True), ("lin2", "linear", TOPOLOGY_SIZE, 301, True),
    ("lin3", "linear", TOPOLOGY_SIZE, 302, True), ("lin64", "linear", TOPOLOGY_SIZE, 303, True),
    ("lin65", "linear", TOPOLOGY_SIZE, 304, False),
    ("w256", "wide", TOPOLOGY_SIZE, 310, True), ("w257", "wide", TOPOLOGY_SIZE, 311, True),
    ("w512", "wide", TOPOLOGY_SIZE, 312, True), ("w513", "wide", TOPOLOGY_SIZE, 313, True),
    ("w257x2", "wide", TOPOLOGY_SIZE, 314, True),
    ("tree3y", "trees", TOPOLOGY_SIZE, 320, True), ("tree7", "trees", TOPOLOGY_SIZE, 321, True),
    ("spine15", "trees", TOPOLOGY_SIZE, 322, True), ("mixed", "trees", TOPOLOGY_SIZE, 323, True),
    ("tree2r", "trees", TOPOLOGY_SIZE, 324, True),
    ("st_root", "stage_tree", TOPOLOGY_SIZE, 330, True), ("st_p1", "stage_tree", TOPOLOGY_SIZE, 331, True),
    ("st_c3", "stage_tree", TOPOLOGY_SIZE, 332, True), ("st_c4", "stage_tree", TOPOLOGY_SIZE, 333, True),
    ("st_c5", "stage_tree", TOPOLOGY_SIZE, 334, True), ("st_c3long", "stage_tree", TOPOLOGY_SIZE, 335, True),
    ("st_c4long", "stage_tree", TOPOLOGY_SIZE, 336, True), ("st_c1", "stage_tree", TOPOLOGY_SIZE, 337, True),
    ("st_nested", "stage_tree", TOPOLOGY_SIZE, 338, True), ("st_dead", "stage_tree", TOPOLOGY_SIZE, 339, True),
    ("st_cycle", "stage_tree", TOPOLOGY_SIZE, 340, False), ("st_tree2", "stage_tree", TOPOLOGY_SIZE, 341, True),
    ("st_64", "stage_tree", TOPOLOGY_SIZE, 342, True),
]
TOPOLOGY_RUNNABLE = [cell for cell in TOPOLOGY_CELLS if cell[4]]


def topology_cell(case_id: str):
    return next(cell for cell in TOPOLOGY_CELLS if cell[0] == case_id)


def topology_frames(cell) -> np.ndarray:
    return arith_frames(cell[2], cell[3])


def stage_links(c):
    """(on_pass, on_fail) of every stage as the walk of tempcv.cpp:834-861 gives them: a stage index, -1 accept, -2 reject."""
    on_pass = [int(v) for v in c.stage_child]
    on_fail = []
    for s in range(c.n_stages):
        ptr = s
        while ptr != -1 and c.stage_next[ptr] == -1:
            ptr = int(c.stage_parent[ptr])
        on_fail.append(-2 if ptr == -1 else int(c.stage_next[ptr]))
    return on_pass, on_fail


def reachable_stages(c) -> set:
    """Stages the pass / fail graph reaches from stage 0."""
    on_pass, on_fail = stage_links(c)
    seen, todo = set(), [0]
    while todo:
        s = todo.pop()
        if s < 0 or s in seen:
            continue
        seen.add(s)
        todo += [on_pass[s], on_fail[s]]
    return seen


def linked_linearly(c):
    """A copy with the same stages in one chain."""
    import copy
    t = copy.deepcopy(c)
    n = t.n_stages
    t.stage_parent = np.arange(-1, n - 1, dtype=np.int32)
    t.stage_next = np.full(n, -1, np.int32)
    t.stage_child = np.array(list(range(1, n)) + [-1], np.int32)
    return t


def without_chain(c, chains, k: int):
    """A copy without chain k: the `next` that leads to it is cut and joined to the chain after it (the prefix's child link
    for the first chain), so the other chains stay as they are."""
    import copy
    t = copy.deepcopy(c)
    head = chains[k][0]
    after = int(t.stage_next[head])
    for s in range(t.n_stages):
        if t.stage_next[s] == head:
            t.stage_next[s] = after
        if t.stage_child[s] == head:
            t.stage_child[s] = after
    return t


def topology_passes(n_prefix: int, chain_lens) -> int:
    """The passes the planner's segment plan (segment_stage_tree) needs with seg_cut2 at its default: one for the prefix, two per chain of more than
    4 stages, else one."""
    return 1 + sum(2 if ln > 4 else 1 for ln in chain_lens)
