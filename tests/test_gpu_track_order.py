"""Environment.track with torch work still pending on its device memory: the cases of tests/test_gpu_stream_order.py for the new
entry point, built on that file's helpers.  The call gets two frames: a ready device copy of frame A, and memory that holds A before
the queued copy and B after it; its rows look for boxes of the first in the second, so on A every sum is 0 at (0, 0) and on B it is
not.  That A's and B's results differ is asserted here on the restatement before anything runs."""
import numpy as np
import pytest

import extract_cases as ec
import prep_cases as pc
import stream_order_cases as sc
import track_cases as tc
from clfacedetection_amd import DeviceFrames
from test_gpu_stream_order import PREMISE, canon, cs, cycles_per_ms, device_pair, queue_delay, ready_wall_ms, record_done  # noqa: F401

pytestmark = pytest.mark.gpu
A, B = sc.A, sc.B
TR = (32, 8)
ROWS = [(0, 1, 36, 54, 96, 96), (0, 1, 200, 150, 64, 64), (0, 1, -10, 280, 80, 60), (0, 1, 300, 20, 32, 32)]


def restated(oracle, which):
    return pc.once(("so_track", which), lambda: tc.restate(oracle, [ec.e2e_bgr()[A], ec.e2e_bgr()[which]], ROWS, *TR))


def test_pending_producer(cs, cycles_per_ms):
    import torch
    s = cs
    want = [canon(restated(s.oracle, k)) for k in (A, B)]
    assert want[A] != want[B], "premise: A's and B's results differ"
    fixed = torch.from_numpy(np.ascontiguousarray(ec.e2e_bgr()[A])[None].copy()).cuda()
    t, d, b_dev = device_pair(s, "bgr")
    call = lambda: s.env.track([DeviceFrames.from_torch(fixed), d], ROWS, tmpl=TR[0], radius=TR[1])   # noqa: E731
    wall, ready = ready_wall_ms(call)
    assert canon(ready) == want[A], "on ready memory that holds A the call returns A's result"
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, "track", wall)
    t.copy_(b_dev, non_blocking=True)
    done = record_done()
    assert not done.query(), PREMISE
    got = canon(call())                                                      # at once: no synchronize in the test
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), b_dev.cpu().numpy())
    assert got != want[A], "the call read the memory before torch's pending copy had written it: it returned A's result"
    assert got == want[B], "the call returned neither A's nor B's result"


def test_results_are_finished_when_the_call_returns(cs):
    """The call returns after its work is complete: a torch read of the results at once sees them, and torch may overwrite the
    frames on any stream right after it."""
    import torch
    s = cs
    want = restated(s.oracle, B)
    fixed = torch.from_numpy(np.ascontiguousarray(ec.e2e_bgr()[A])[None].copy()).cuda()
    t = torch.from_numpy(np.ascontiguousarray(ec.e2e_bgr()[B])[None].copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = s.env.track([fixed, t], ROWS, tmpl=TR[0], radius=TR[1])
    with torch.cuda.stream(side):
        t.zero_()
        sums = torch.from_numpy(got["sad"].astype(np.int64)).cuda().sum()
    assert int(sums.item()) == int(want["sad"].astype(np.int64).sum())
    torch.cuda.synchronize()
    assert tc.equal(got, want)
