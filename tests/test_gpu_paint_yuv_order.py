"""vj_paint_yuv and torch work pending on its frames ("In-place calls"), on the helpers of
tests/test_gpu_stream_order.py.  paint_yuv() writes the planes it is given: it must run after work queued on them on torch's current
stream, and what torch queues right after the call must see the painted planes.  A and B are two random stacked 38 x 30 NV12 frames;
painting either changes it, and the two painted frames differ (asserted here: a test whose premise does not hold fails)."""
import numpy as np
import pytest

import paint_yuv_cases as pyc
import yuv_cases as yc
from test_gpu_stream_order import PREMISE, cycles_per_ms, queue_delay, ready_wall_ms, record_done  # noqa: F401 (cycles_per_ms: a fixture)

pytestmark = pytest.mark.gpu
RECTS = [(0, 5, 3, 21, 15), (0, 15, 10, 30, 30)]
KW = dict(size=5, ellipse=True)


def frames_and_restatements():
    out = []
    for seed in (31, 32):
        f = pyc.frame(pyc.W, pyc.H, yc.NV12, seed)
        out.append((yc.stacked(f, yc.NV12)[None], yc.stacked(pyc.restate([f], yc.NV12, RECTS, "blur", **KW)[0], yc.NV12)[None]))
    (a, wa), (b, wb) = out
    assert not np.array_equal(wa, a) and not np.array_equal(wb, b) and not np.array_equal(wa, wb)
    assert not np.array_equal(wa[0, pyc.H:], a[0, pyc.H:]) and not np.array_equal(wb[0, pyc.H:], b[0, pyc.H:])     # the chroma too
    return a, b, [wa, wb]


def test_a_pending_producer_is_painted_not_what_it_overwrites(env, cycles_per_ms):
    """The tensor holds A; a delay and then the copy of B are queued on torch's current stream; paint_yuv() is called at once.
    Without the ordering the regions of A are painted and the copy then overwrites them: the tensor ends as B, unpainted."""
    import torch
    a, b, want = frames_and_restatements()
    t = torch.from_numpy(a.copy()).cuda()
    b_dev = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    wall, _ = ready_wall_ms(lambda: env.paint_yuv(t.clone(), RECTS, "blur", **KW))
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, "paint_yuv", wall)
    t.copy_(b_dev, non_blocking=True)
    done = record_done()
    assert not done.query(), PREMISE
    assert env.paint_yuv(t, RECTS, "blur", **KW) is t                        # at once: no synchronize in the test
    torch.cuda.synchronize()
    got = t.cpu().numpy()
    print("the tensor holds", "B painted" if np.array_equal(got, want[1]) else "B unpainted" if np.array_equal(got, b) else "something else")
    assert not np.array_equal(got, b), "paint_yuv() ran before torch's pending copy: the copy overwrote what it painted"
    assert np.array_equal(got, want[1])


def test_a_torch_read_right_after_the_call_sees_the_painted_planes(env):
    """The call returns after its work is complete: any stream of torch's may read the planes at once."""
    import torch
    a, b, want = frames_and_restatements()
    side = torch.cuda.Stream()
    for src, w in ((a, want[0]), (b, want[1])):
        t = torch.from_numpy(src.copy()).cuda()
        torch.cuda.synchronize()
        env.paint_yuv(t, RECTS, "blur", **KW)
        copy = t.clone()                                                       # on the current stream ...
        with torch.cuda.stream(side):
            total = t.to(torch.int32).sum()                                    # ... and on a side stream, both right after the call
        assert int(total.item()) == int(w.astype(np.int64).sum())
        torch.cuda.synchronize()
        assert np.array_equal(copy.cpu().numpy(), w)
