"""vj_extract_yuv / vj_extract_affine_yuv and torch work pending on their frames, on the helpers of
tests/test_gpu_stream_order.py.  Both calls read device planes torch may still be writing: they must run after work queued on torch's
current stream, and what torch queues right after a call must see the crops.  A and B are two random stacked 38 x 30 NV12 frames whose
crops differ (asserted here: a test whose premise does not hold fails)."""
import numpy as np
import pytest

import affine_cases as ac
import extract_yuv_cases as eyc
import yuv_cases as yc
from clfacedetection_amd import YuvFrames
from test_gpu_stream_order import PREMISE, cycles_per_ms, queue_delay, ready_wall_ms, record_done  # noqa: F401 (cycles_per_ms: a fixture)

pytestmark = pytest.mark.gpu
RECTS = [(0, 5, 3, 21, 15), (0, -2, 10, 30, 30)]
ROWS = ac.rows_for(0, [eyc.REPRESENTATIVE, ac.identity()])
SIZE = (21, 17)
CALLS = {"extract_yuv": lambda env, y: env.extract_yuv(y, RECTS, SIZE, alpha=True),
         "extract_affine_yuv": lambda env, y: env.extract_affine_yuv(y, ROWS, SIZE, rgb=True)}


def frames_and_restatements(oracle, name):
    out = []
    for seed in (31, 32):
        f = yc.random_frame(38, 30, yc.NV12, seed)
        want = (eyc.restate(oracle, [f], yc.NV12, RECTS, SIZE, alpha=True) if name == "extract_yuv"
                else eyc.restate_affine(oracle, [f], yc.NV12, ROWS, SIZE, rgb=True))
        out.append((yc.stacked(f, yc.NV12)[None], want))
    (a, wa), (b, wb) = out
    assert not np.array_equal(wa, wb)
    return a, b, [wa, wb]


@pytest.mark.parametrize("name", list(CALLS))
def test_a_pending_producer_is_cropped_not_what_it_overwrites(env, oracle, cycles_per_ms, name):
    """The tensor holds A; a delay and then the copy of B are queued on torch's current stream; the call is made at once.  Without the
    ordering it crops frame A."""
    import torch
    a, b, want = frames_and_restatements(oracle, name)
    t = torch.from_numpy(a.copy()).cuda()
    b_dev = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    wall, _ = ready_wall_ms(lambda: CALLS[name](env, YuvFrames.from_torch(t)))
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, name, wall)
    t.copy_(b_dev, non_blocking=True)
    done = record_done()
    assert not done.query(), PREMISE
    got = CALLS[name](env, YuvFrames.from_torch(t)).cpu().numpy()             # at once: no synchronize in the test
    print("the crops are of", "B" if np.array_equal(got, want[1]) else "A" if np.array_equal(got, want[0]) else "something else")
    assert not np.array_equal(got, want[0]), f"{name}() ran before torch's pending copy: it cropped the frame the copy overwrote"
    assert np.array_equal(got, want[1])


@pytest.mark.parametrize("name", list(CALLS))
def test_a_torch_read_right_after_the_call_sees_the_crops(env, oracle, name):
    """The call returns after its work is complete: any stream of torch's may read the crops at once."""
    import torch
    a, b, want = frames_and_restatements(oracle, name)
    side = torch.cuda.Stream()
    for src, w in ((a, want[0]), (b, want[1])):
        t = torch.from_numpy(src.copy()).cuda()
        out = torch.zeros(w.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = (env.extract_yuv(YuvFrames.from_torch(t), RECTS, SIZE, alpha=True, out=out) if name == "extract_yuv"
               else env.extract_affine_yuv(YuvFrames.from_torch(t), ROWS, SIZE, rgb=True, out=out))
        copy = res.clone()                                                       # on the current stream ...
        with torch.cuda.stream(side):
            total = res.to(torch.int32).sum()                                    # ... and on a side stream, both right after the call
        assert int(total.item()) == int(w.astype(np.int64).sum())
        torch.cuda.synchronize()
        assert np.array_equal(copy.cpu().numpy(), w)
