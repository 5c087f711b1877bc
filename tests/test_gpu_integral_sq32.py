"""The u32 layout of the squared integral (IntegralArgs::sq_u32: the squares kept in 32 bits end to end, values mod 2^32), read
back through vj_integral_batch_sq32, against numpy's cumulative sums mod 2^32 — every element, and the sum image with it.

Shapes are the smallest that reach each kernel: single frames run band_scan2 + band_rows_par (37 x 45, 300 x 300, the widths
around one 256-column chunk and 1023, the heights around one 8-row band), 2048 bands or more in a call run band_scan2 +
band_rows_w3 (260 frames of 64 x 64; 1024 frames of 257 x 9: a partial chunk and a partial band), and integral_rows 0 sends
single frames through band_rows.  Contents: all 255 (the largest squares: 300 x 300 wraps 2^32) and random {0, 255}."""
import numpy as np
import pytest

from cases import tunables

pytestmark = pytest.mark.gpu


def content(kind, shape, seed):
    if kind == "all255":
        return np.full(shape, 255, np.uint8)
    return np.random.default_rng(seed).integers(0, 2, shape, dtype=np.uint8) * np.uint8(255)


def integrals_mod32(gray):
    """(sum, squared sum) of (n, h, w) uint8 frames, both (n, h + 1, w + 1) uint32: the exact integrals reduced mod 2^32."""
    a = gray.astype(np.uint64)
    out = []
    for v in (a, a * a):
        full = np.zeros((gray.shape[0], gray.shape[1] + 1, gray.shape[2] + 1), np.uint64)
        np.cumsum(np.cumsum(v, axis=1), axis=2, out=full[:, 1:, 1:])
        out.append((full & np.uint64(0xffffffff)).astype(np.uint32))
    return out


def check(env, frames, label, gray=None, color=False):
    s, q = env.integral_sq32(frames, color=color)
    ws, wq = integrals_mod32(frames if gray is None else gray)
    assert s.shape == ws.shape and q.shape == wq.shape, label
    assert np.array_equal(s, ws), f"{label}: sum differs in {int((s != ws).sum())} elements"
    bad = np.argwhere(q != wq)
    assert len(bad) == 0, f"{label}: squared sum differs in {len(bad)} elements, first at (frame, y, x) = {tuple(bad[0])}"


SINGLE = [(45, 37), (300, 300)] + [(h, w) for h in (7, 8, 9) for w in (255, 256, 257, 1023)]


@pytest.mark.parametrize("kind", ["all255", "random"])
@pytest.mark.parametrize("rows", [0, 1, 2], ids=lambda m: f"rows{m}")
def test_single_frames(env, kind, rows):
    """One frame per call: the two-level band prefix and the side-by-side row kernel (integral_rows 1, and 2 for a call that is
    no batch), or one wave per band (0)."""
    with tunables(env, ("integral_rows", rows)):
        for h, w in SINGLE:
            check(env, content(kind, (1, h, w), h * 1000 + w), f"{kind} {w} x {h} integral_rows={rows}")
    white = integrals_mod32(np.full((1, 300, 300), 255, np.uint8))[1]
    assert 65025 * 300 * 300 >= 2**32 and int(white[0, -1, -1]) == 65025 * 300 * 300 - 2**32    # (the case does wrap)


@pytest.mark.parametrize("kind", ["all255", "random"])
@pytest.mark.parametrize("n,h,w", [(260, 64, 64), (1024, 9, 257)])
def test_batches_of_2048_bands(env, kind, n, h, w):
    """n frames x ceil(h / 8) bands >= 2048: the batch form of the row kernel (three waves per SIMD, non-temporal stores),
    whatever integral_rows' default (2) would choose for a smaller call; frames differ, so a frame read at another's offset
    shows."""
    assert n * ((h + 7) // 8) >= 2048
    frames = content(kind, (n, h, w), n + h + w)
    if kind == "all255":
        frames[1::2, ::3, ::5] = 0          # (distinct neighbours)
    check(env, frames, f"{kind} {n} x {w} x {h}")
    with tunables(env, ("integral_rows", 1)):   # the same batch through the side-by-side kernel
        check(env, frames, f"{kind} {n} x {w} x {h} integral_rows=1")


def test_bgr_input(env, oracle):
    """BGR frames are converted inside the integral kernels: the reference is the oracle's gray image."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 2, (2, 45, 261, 3), dtype=np.uint8) * np.uint8(255)
    img[1] = 255
    gray = np.stack([oracle.bgr2gray(f) for f in img])
    check(env, img, "BGR 261 x 45", gray=gray, color=True)


def test_u64_call_is_unchanged_after_a_u32_one(env, oracle):
    """vj_integral keeps returning the exact u64 image, also right after a call that left the u32 layout in the same buffers."""
    img = np.full((300, 300), 255, np.uint8)
    img[::7, ::11] = 0
    env.integral_sq32(img[None])
    s, q = env.integral(img)
    so, qo = oracle.integral(img)
    assert int(qo[-1, -1]) >= 2**32 and np.array_equal(s, so) and np.array_equal(q, qo)
    check(env, img[None], "u32 after u64")
