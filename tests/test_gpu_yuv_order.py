"""vj_yuv_to_bgr / vj_bgr_to_yuv and torch work pending on their frames ("Sharing a process with PyTorch"), on the
helpers of tests/test_gpu_stream_order.py.  Both calls read device memory a decoder or a paint() may still be writing: they must run
after work queued on it on torch's current stream, and what torch queues right after the call must see the converted frames.  A and
B are two random 66 x 38 frames whose conversions differ (asserted here: a test whose premise does not hold fails)."""
import numpy as np
import pytest

import yuv_cases as yc
from clfacedetection_amd import DeviceFrames, YuvFrames
from test_gpu_stream_order import PREMISE, cycles_per_ms, queue_delay, ready_wall_ms, record_done  # noqa: F401 (cycles_per_ms: a fixture)

pytestmark = pytest.mark.gpu
W, H = 66, 38


def download(d, nbytes):
    off = d.ptr - d.owner.data_ptr() if isinstance(d, DeviceFrames) else d.ptr_y - d.owner.data_ptr()
    return d.owner.cpu().numpy()[off:off + nbytes]


def cases():
    """direction -> (A, B as host arrays of what the tensor holds, the call on the tensor, the restatement of A and B as flat bytes)"""
    ya, yb = (yc.stacked(yc.random_frame(W, H, yc.NV12, s), yc.NV12)[None] for s in (41, 42))
    ba, bb = (yc.random_image(W, H, 3, s)[None] for s in (43, 44))
    dec_bytes, enc_bytes = H * yc.align(W * 3, 4), yc.align(W, 4) * (H + H // 2)
    dec_want = [yc.decode_buffer([yc.unstack(y[0], yc.NV12)], yc.NV12, 3, False, dec_bytes, 0)[0] for y in (ya, yb)]
    enc_want = [yc.encode_buffer([b[0]], yc.NV12, False, enc_bytes, 0)[0] for b in (ba, bb)]
    assert not np.array_equal(dec_want[0], dec_want[1]) and not np.array_equal(enc_want[0], enc_want[1])
    return {"yuv_to_bgr": (ya, yb, lambda env, t: env.yuv_to_bgr(YuvFrames.from_torch(t))[0], dec_want),
            "bgr_to_yuv": (ba, bb, lambda env, t: env.bgr_to_yuv(DeviceFrames.from_torch(t)), enc_want)}


@pytest.mark.parametrize("direction", ["yuv_to_bgr", "bgr_to_yuv"])
def test_a_pending_producer_is_converted_not_what_it_overwrites(env, cycles_per_ms, direction):
    """The tensor holds A; a delay and then the copy of B are queued on torch's current stream; the call is made at once.  Without
    the ordering it converts A."""
    import torch
    a, b, call, want = cases()[direction]
    t = torch.from_numpy(a.copy()).cuda()
    b_dev = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()
    wall, r = ready_wall_ms(lambda: call(env, t))
    assert np.array_equal(download(r, len(want[0])), want[0])                     # on ready input: A's conversion
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, direction, wall)
    t.copy_(b_dev, non_blocking=True)
    done = record_done()
    assert not done.query(), PREMISE
    r = call(env, t)                                                              # at once: no synchronize in the test
    torch.cuda.synchronize()
    got = download(r, len(want[1]))
    print("the call converted", "B" if np.array_equal(got, want[1]) else "A" if np.array_equal(got, want[0]) else "something else")
    assert not np.array_equal(got, want[0]), "the call ran before torch's pending copy: it converted what the copy overwrote"
    assert np.array_equal(got, want[1])


@pytest.mark.parametrize("direction", ["yuv_to_bgr", "bgr_to_yuv"])
def test_a_torch_read_right_after_the_call_sees_the_converted_frames(env, direction):
    """The call returns after its work is complete: any stream of torch's may read its output at once."""
    import torch
    a, b, call, want = cases()[direction]
    side = torch.cuda.Stream()
    for src, w in ((a, want[0]), (b, want[1])):
        t = torch.from_numpy(src.copy()).cuda()
        torch.cuda.synchronize()
        r = call(env, t)
        off = (r.ptr if isinstance(r, DeviceFrames) else r.ptr_y) - r.owner.data_ptr()
        view = r.owner[off:off + len(w)]
        copy = view.clone()                                                       # on the current stream ...
        with torch.cuda.stream(side):
            total = view.to(torch.int32).sum()                                    # ... and on a side stream, both right after the call
        assert int(total.item()) == int(w.astype(np.int64).sum())
        torch.cuda.synchronize()
        assert np.array_equal(copy.cpu().numpy(), w)
