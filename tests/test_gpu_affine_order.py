"""Environment.extract_affine with torch work still pending on its device memory: the cases of tests/test_gpu_stream_order.py (a
producer queued behind a delay on torch's current stream; a fill of out= queued behind a delay) for the new entry point, built on
that file's helpers.  The memory holds frame A before the queued copy and frame B after it; the call must return the restatement's
bytes for B (tests/affine_cases.py).  That A's and B's results differ is asserted here on the restatement before anything runs."""
import numpy as np
import pytest

import affine_cases as ac
import extract_cases as ec
import prep_cases as pc
import stream_order_cases as sc
from test_gpu_stream_order import (PREMISE, canon, cs, cycles_per_ms, device_pair, queue_delay, ready_wall_ms, record_done,  # noqa: F401
                                   tensor_bytes)

pytestmark = pytest.mark.gpu
A, B = sc.A, sc.B
SIZE = (32, 32)
ROWS = ac.rows_for(0, [ac.rotation(20.0, 2.0, (200.0, 150.0), SIZE), ac.from_rect(36, 54, 108, 108, SIZE), ac.rotation(-35.0, 3.0, (10.0, 300.0), SIZE),
                       ac.from_rect(0, 0, pc.E2E_SRC_W, pc.E2E_SRC_H, SIZE)])


def restated(oracle, which):
    return pc.once(("so_affine", which), lambda: ac.restate(oracle, [ec.e2e_bgr()[which]], ROWS, SIZE))


def test_pending_producer(cs, cycles_per_ms):
    import torch
    s = cs
    want = [canon(restated(s.oracle, k)) for k in (A, B)]
    assert want[A] != want[B], "premise: A's and B's results differ"
    t, d, b_dev = device_pair(s, "bgr")
    wall, ready = ready_wall_ms(lambda: s.env.extract_affine([d], ROWS, SIZE))
    assert tensor_bytes(ready) == want[A], "on ready memory that holds A the call returns A's result"
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, "extract_affine", wall)
    t.copy_(b_dev, non_blocking=True)
    done = record_done()
    assert not done.query(), PREMISE
    got = tensor_bytes(s.env.extract_affine([d], ROWS, SIZE))                # at once: no synchronize in the test
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), b_dev.cpu().numpy())
    assert got != want[A], "the call read the memory before torch's pending copy had written it: it returned A's result"
    assert got == want[B], "the call returned neither A's nor B's result"


def test_out_tensor_with_pending_work_on_it(cs, cycles_per_ms):
    """A fill of the destination is queued behind the delay: it must not land after the library's write."""
    import torch
    s = cs
    want = canon(restated(s.oracle, B))
    call = lambda out: s.env.extract_affine([s.src["bgr"][B]], ROWS, SIZE, out=out)   # noqa: E731
    out = torch.zeros(restated(s.oracle, B).size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    wall, ready = ready_wall_ms(lambda: call(out))
    assert tensor_bytes(ready) == want
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, "extract_affine out=", wall)
    out.fill_(0xAB)
    done = record_done()
    assert not done.query(), PREMISE
    got = tensor_bytes(call(out))
    torch.cuda.synchronize()
    assert got == want, "the pending fill of out= landed after the library's write"
