"""Device-resident inputs and outputs with torch work still pending on them ("Sharing a process with PyTorch").

The library's streams are non-blocking, so the Python wrapper orders every call that passes device memory after torch's current
stream on the environment's device.  Each test queues a delay and then the work on that stream, checks that the work is still
pending (`done.query()` is False: the premise — a test whose premise does not hold fails, it never passes vacuously) and calls the
library at once, with no synchronize of its own.  The memory holds A before the work and B after it (tests/stream_order_cases.py):
the call must return B's result — the oracle's or the restatement's where one exists, else what the same entry point returns for
the host copy of B, whose equality with the oracle is its own test file's matter — and not A's.  That the two differ is asserted on
the CPU in tests/test_stream_order_cpu.py.

The delay is the larger of 50 ms and ten times the wall time of the same call on ready input, at most 500 ms; both are printed.
Nothing here can fault: without the ordering the library reads or writes valid memory too early, which is a wrong answer.

Against a wrapper without the ordering (the one before this file existed), on an MI355X: every row of test_pending_producer
returned A's result — detect, detect_opencv, detect_chain, detect_opencv_chain with and without the device hand-off, detect_rois,
detect_opencv_rois, detect_opencv_roc, run_windows, run_windows_opencv, detect_mixed, detect_opencv_mixed, pack_frames, preprocess,
extract, canny, equalize_hist, resize_linear, integral_sq32, FrameStream.submit / collect —, so did the three side-stream cases; the
two out= cases came back filled with 0xAB; in the two allocator-reuse cases the clone held the call's output instead of 0x5A.  The
two after-call cases and the host-frames case passed, as they must."""
import contextlib
import time
from types import SimpleNamespace

import numpy as np
import pytest

import clod_window_oracle as cw
import cv_rois_cases as cc
import extract_cases as ec
import mixed_cases as mc
import prep_cases as pc
import run_window_oracle as rw
import stream_order_cases as sc
from clfacedetection_amd import (VJ_FLAG_COUNTERS, VJ_FLAG_CV_CHAIN_DEVICE, VJ_FLAG_CV_SCALE_IMAGE, DeviceFrames, Environment,
                                 default_params, run_windows, run_windows_opencv)
from clfacedetection_amd.api import DetectResult
from test_gpu_prep import download

pytestmark = pytest.mark.gpu
CNT = VJ_FLAG_COUNTERS
A, B = sc.A, sc.B
PREMISE = ("premise: the producer queued on torch's stream must still be pending when the library is called (done.query() was "
           "already True) — nothing was tested; the delay is too short for this machine")


# ------------------------------------------------------------------------------------------------------------------- the delay
@pytest.fixture(scope="session")
def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond, measured once with two torch events."""
    import torch
    torch.cuda._sleep(1000)                                          # loads the kernel
    torch.cuda.synchronize()
    n = 1_000_000
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 10.0:
            break
        n *= 10
    print(f"torch.cuda._sleep: {n} cycles took {ms:.2f} ms")
    assert ms >= 10.0, "torch.cuda._sleep does not delay the stream"
    return n / ms


def ready_wall_ms(call):
    """Wall time of `call` on ready input: the second of two runs (the first builds plans and buffers).  Returns (ms, result)."""
    call()
    t0 = time.perf_counter()
    r = call()
    return (time.perf_counter() - t0) * 1e3, r


def delay_ms(wall_ms):
    return min(max(50.0, 10.0 * wall_ms), 500.0)


def queue_delay(cycles_per_ms, label, wall_ms):
    import torch
    ms = delay_ms(wall_ms)
    print(f"{label}: {wall_ms:.2f} ms on ready input, delay {ms:.0f} ms")
    torch.cuda._sleep(int(ms * cycles_per_ms))


def record_done():
    import torch
    done = torch.cuda.Event()
    done.record()
    return done


# ------------------------------------------------------------------------------------------------------------------ comparing
def canon(r):
    """A result as something == compares: arrays by shape, type and bytes; a DetectResult by its rectangles, counters and levels."""
    if isinstance(r, DetectResult):
        return ("result", canon(r.rects), r.windows, r.stump_evals, tuple(r.stage_entered), canon(r.reject_levels), canon(r.level_weights))
    if isinstance(r, np.ndarray):
        return (r.shape, r.dtype.str, np.ascontiguousarray(r).tobytes())
    if isinstance(r, (tuple, list)):
        return tuple(canon(x) for x in r)
    assert r is None or isinstance(r, (int, float)), type(r)
    return r


def counted(r):
    return (mc.rows(r.rects), r.windows, [int(v) for v in r.stage_entered])


def oracle_counted(lists, which):
    want, st = lists[which]
    return (mc.rows(want), int(st["windows"]), [int(v) for v in st["stage_entered"]])


def prep_images(outs):
    return canon([img[:, :w] for img, w in download(outs)])


def tensor_bytes(t):
    return canon(t.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------------- the cases
@pytest.fixture(scope="module")
def cs(env, oracle, cascades):
    c, a = cascades(pc.CASC)
    c2, a2 = cascades("eye")
    prepared = pc.e2e_prepared(oracle)
    s = SimpleNamespace(env=env, oracle=oracle, c=c, a=a, c2=c2,
                        src={"prepared": [np.ascontiguousarray(prepared[k]) for k in (A, B)],
                             "gray": [np.ascontiguousarray(pc.e2e_frames()[k]) for k in (A, B)],
                             "bgr": [np.ascontiguousarray(ec.e2e_bgr()[k]) for k in (A, B)]},
                        small=prepared[2][:97, :131],                      # a host frame of another size: the two are packed into an atlas
                        rois=np.array([(0, *r) for r in cc.REGIONS], np.int32),
                        cv_windows=sc.cv_windows(a), clod_windows=sc.clod_windows(a), streams=[])
    assert (rw.FRAME_W, rw.FRAME_H) == pc.E2E_SIZE == (cw.FRAME_W, cw.FRAME_H)
    yield s
    for fs in s.streams:
        fs.close()


def frame_stream(s):
    if not s.streams:
        s.streams.append(s.env.stream(s.c, pc.E2E_SIZE[0], pc.E2E_SIZE[1], 1, default_params(flags=CNT)))
    return s.streams[0]


def submit_collect(s, x):
    fs = frame_stream(s)
    fs.submit(x)
    return fs.collect()


# id -> (which A / B pair the memory holds, call(s, x) with x a DeviceFrames or the host array, view of the result, the oracle's or
# restatement's view for A / B — None: the same call on the host array)
TABLE = {
    "detect": ("prepared", lambda s, x: s.env.detect(s.c, x, default_params(flags=CNT)), counted,
               lambda s, k: oracle_counted(sc.detect_lists(s.oracle, s.a, "clod"), k)),
    "detect_opencv": ("prepared", lambda s, x: s.env.detect_opencv(s.c, x, flags=CNT), counted,
                      lambda s, k: oracle_counted(sc.detect_lists(s.oracle, s.a, "cv"), k)),
    "detect_chain": ("prepared", lambda s, x: s.env.detect_chain(s.c, s.c2, x, default_params(min_neighbors=3), default_params(flags=CNT)),
                     canon, None),
    "detect_opencv_chain": ("prepared", lambda s, x: s.env.detect_opencv_chain(s.c, s.c2, x, min_neighbors=3, flags=CNT, flags_second=CNT),
                            canon, None),
    "detect_opencv_chain_device": ("prepared", lambda s, x: s.env.detect_opencv_chain(s.c, s.c2, x, min_neighbors=3, flags=CNT | VJ_FLAG_CV_CHAIN_DEVICE,
                                                                                       flags_second=CNT), canon, None),
    "detect_rois": ("prepared", lambda s, x: s.env.detect_rois(s.c, x, s.rois, default_params(flags=CNT)), canon, None),
    "detect_opencv_rois": ("prepared", lambda s, x: s.env.detect_opencv_rois(s.c, x, s.rois, flags=CNT), canon, None),
    "detect_opencv_roc": ("prepared", lambda s, x: s.env.detect_opencv_roc(s.c, x, flags=VJ_FLAG_CV_SCALE_IMAGE | CNT), canon, None),
    "run_windows": ("prepared", lambda s, x: run_windows(x, s.c, s.env, s.clod_windows, cw.case_scales()), canon, None),
    "run_windows_opencv": ("prepared", lambda s, x: run_windows_opencv(x, s.c, s.env, s.cv_windows, rw.case_scales()), canon, None),
    "detect_mixed": ("prepared", lambda s, x: s.env.detect_mixed(s.c, [x, s.small], default_params(flags=CNT)), canon, None),
    "detect_opencv_mixed": ("prepared", lambda s, x: s.env.detect_opencv_mixed(s.c, [x, s.small], flags=CNT), canon, None),
    "pack_frames": ("prepared", lambda s, x: s.env.pack_frames([x, s.small]), canon, None),
    "preprocess": ("gray", lambda s, x: s.env.preprocess([x], **sc.PREP_KW), prep_images,
                   lambda s, k: canon([sc.prepared(s.oracle, k)])),
    "extract": ("bgr", lambda s, x: s.env.extract([x], sc.EXTRACT_RECTS, sc.EXTRACT_SIZE, scale=sc.EXTRACT_SCALE), tensor_bytes,
                lambda s, k: canon(sc.extracted(s.oracle, k))),
    "canny": ("prepared", lambda s, x: s.env.canny(x), canon, lambda s, k: canon(sc.canny(s.oracle, k))),
    "equalize_hist": ("prepared", lambda s, x: s.env.equalize_hist(x), canon, lambda s, k: canon(sc.equalized(s.oracle, k))),
    "resize_linear": ("prepared", lambda s, x: s.env.resize_linear(x, *sc.RESIZE_TO), canon, lambda s, k: canon(sc.resized(s.oracle, k))),
    "integral_sq32": ("prepared", lambda s, x: s.env.integral_sq32(x), canon, None),
    "frame_stream": ("prepared", submit_collect, counted, None),
}


def expected(s, name):
    """(A's view, B's view) of a row: from the oracle or the restatement, else from the entry point itself on the host arrays."""
    src, call, view, reference = TABLE[name]
    if reference is not None:
        want = [reference(s, k) for k in (A, B)]
    else:
        want = [view(call(s, s.src[src][k])) for k in (A, B)]
    assert want[A] != want[B], "premise: A's and B's results differ"
    return want


def device_pair(s, src):
    """(tensor holding A, DeviceFrames of it, tensor holding B), ready."""
    import torch
    t = torch.from_numpy(s.src[src][A][None].copy()).cuda()
    b_dev = torch.from_numpy(s.src[src][B][None].copy()).cuda()
    torch.cuda.synchronize()
    return t, DeviceFrames.from_torch(t), b_dev


def pending_input(s, name, cycles_per_ms, stream=None):
    """The row's call on memory that holds A while a delay and then the copy of B are queued on torch's current stream (`stream`:
    a side stream that is made current for the producer and the call).  Returns the view of what the call returned."""
    import torch
    src, call, view, _ = TABLE[name]
    want = expected(s, name)
    t, d, b_dev = device_pair(s, src)
    wall, ready = ready_wall_ms(lambda: call(s, d))
    assert view(ready) == want[A], "on ready memory that holds A the call returns A's result"
    torch.cuda.synchronize()
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        queue_delay(cycles_per_ms, name, wall)
        t.copy_(b_dev, non_blocking=True)
        done = record_done()
        assert not done.query(), PREMISE
        got = view(call(s, d))                                            # at once: no synchronize in the test
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), b_dev.cpu().numpy())
    print(f"{name}: the call returned {'B' if got == want[B] else 'A' if got == want[A] else 'neither'}'s result")
    assert got != want[A], "the call read the memory before torch's pending copy had written it: it returned A's result"
    assert got == want[B], "the call returned neither A's nor B's result: it read the memory while torch's pending copy was writing it"
    return got


# ------------------------------------------------------------------------------------------ 1. a producer on the current stream
# The two window-list calls upload their scale records with a blocking hipMemcpy (csrc/vj_points_driver.hpp) before they touch a
# frame.  That copy runs on the null stream, and the null stream is torch's default stream: there the library happens to wait for the
# producer whatever the wrapper does, and the case could not fail.  Their producer therefore runs on side streams.
ORDERED_AFTER_THE_NULL_STREAM_BY_ACCIDENT = ("run_windows", "run_windows_opencv")


def on_two_side_streams(s, name, cycles_per_ms):
    """Two streams of torch's pool, one after the other.  The runtime maps its streams onto a few hardware queues (four by default),
    and a producer whose stream shares a queue with the library's is ordered before the library's work by the hardware alone:
    without any ordering in the wrapper, one in four consecutive pool streams gave B for detect_opencv, preprocess and extract on
    an MI355X, and every second one for the window lists — never two in a row, so one of the two streams here is a real test."""
    import torch
    for _ in range(2):
        pending_input(s, name, cycles_per_ms, stream=torch.cuda.Stream())


@pytest.mark.parametrize("name", list(TABLE))
def test_pending_producer(cs, cycles_per_ms, name):
    if name in ORDERED_AFTER_THE_NULL_STREAM_BY_ACCIDENT:
        on_two_side_streams(cs, name, cycles_per_ms)
    else:
        pending_input(cs, name, cycles_per_ms)


# ------------------------------------------------------------------------------------------------------------ 2. a side stream
@pytest.mark.parametrize("name", ["detect_opencv", "preprocess", "extract"])
def test_producer_on_a_side_stream_that_is_current_at_the_call(cs, cycles_per_ms, name):
    on_two_side_streams(cs, name, cycles_per_ms)


# --------------------------------------------------------------------------------------------- 3. a caller's out= with work on it
def _out_cases(s):
    """name -> (call(out) on the HOST copy of B, bytes of the output, view, B's restatement)"""
    recs, nbytes = s.env.preprocess_layout([s.src["gray"][B]], **sc.PREP_KW)
    assert nbytes == pc.E2E_SIZE[0] * pc.E2E_SIZE[1]                        # rows of 240 bytes: no pad columns
    return {"preprocess": (lambda out: s.env.preprocess([s.src["gray"][B]], out=out, **sc.PREP_KW), nbytes, prep_images,
                           canon([sc.prepared(s.oracle, B)])),
            "extract": (lambda out: s.env.extract([s.src["bgr"][B]], sc.EXTRACT_RECTS, sc.EXTRACT_SIZE, scale=sc.EXTRACT_SCALE, out=out),
                        sc.extracted(s.oracle, B).size, tensor_bytes, canon(sc.extracted(s.oracle, B)))}


@pytest.mark.parametrize("name", ["preprocess", "extract"])
def test_out_tensor_with_pending_work_on_it(cs, cycles_per_ms, name):
    """A fill of the destination is queued behind the delay: it must not land after the library's write."""
    import torch
    call, nbytes, view, want = _out_cases(cs)[name]
    out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    wall, ready = ready_wall_ms(lambda: call(out))
    assert view(ready) == want
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, name + " out=", wall)
    out.fill_(0xAB)
    done = record_done()
    assert not done.query(), PREMISE
    res = call(out)
    got = view(res)
    torch.cuda.synchronize()
    assert got == want, "the pending fill of out= landed after the library's write"


@pytest.mark.parametrize("name", ["preprocess", "extract"])
def test_allocator_reuse(cs, cycles_per_ms, name):
    """The block the call's own torch.empty gets is one whose last reader, a clone, is still queued on torch's stream."""
    import torch
    call, nbytes, view, want = _out_cases(cs)[name]
    wall, ready = ready_wall_ms(lambda: call(None))
    assert view(ready) == want
    del ready
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                                # the next block starts a segment: nothing to merge with
    x = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, name + " allocator reuse", wall)
    y = x.clone()
    done = record_done()
    p = x.data_ptr()
    del x
    assert not done.query(), PREMISE
    res = call(None)
    start = (res[0].owner if name == "preprocess" else res).data_ptr()
    got = view(res)
    torch.cuda.synchronize()
    assert start == p, "premise: torch's allocator must hand the call the block that was just freed — it did not, nothing was tested"
    assert bool((y == 0x5A).all()), "the library wrote the recycled block before its pending reader had run"
    assert got == want


# ---------------------------------------------------------------------------------------------------------- 4. after the call
@pytest.mark.parametrize("name", ["preprocess", "extract"])
def test_result_is_ready_for_any_stream(cs, name):
    """The call returns after its work is complete: a side stream may consume the result at once."""
    import torch
    call, nbytes, view, want = _out_cases(cs)[name]
    side = torch.cuda.Stream()
    res = call(None)
    t = res[0].owner if name == "preprocess" else res
    with torch.cuda.stream(side):
        total = t.to(torch.int32).sum()
    restated = sc.prepared(cs.oracle, B) if name == "preprocess" else sc.extracted(cs.oracle, B)
    assert int(total.item()) == int(restated.astype(np.int64).sum())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 5. no over-synchronizing
def test_a_call_on_host_frames_does_not_wait_for_torch(cs, cycles_per_ms):
    import torch
    s = cs
    frame = s.src["prepared"][B]
    want = oracle_counted(sc.detect_lists(s.oracle, s.a, "clod"), B)
    wall, ready = ready_wall_ms(lambda: s.env.detect(s.c, frame, default_params(flags=CNT)))
    assert counted(ready) == want
    torch.cuda.synchronize()
    queue_delay(cycles_per_ms, "detect on a host frame", wall)
    done = record_done()
    assert not done.query(), PREMISE
    r = s.env.detect(s.c, frame, default_params(flags=CNT))
    still_pending = not done.query()
    torch.cuda.synchronize()
    assert counted(r) == want
    assert still_pending, "a call that passes no device pointer waited for torch's stream"


# ---------------------------------------------------------------------------------------------------------- 6. a second device
def test_outputs_are_allocated_on_the_environments_device(cs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second visible GPU")
    assert torch.cuda.current_device() == 0
    e1 = Environment(1)
    try:
        outs = e1.preprocess([cs.src["gray"][B]], **sc.PREP_KW)
        assert outs[0].owner.device == torch.device("cuda", 1)
        assert prep_images(outs) == canon([sc.prepared(cs.oracle, B)])
        res = e1.extract([cs.src["bgr"][B]], sc.EXTRACT_RECTS, sc.EXTRACT_SIZE, scale=sc.EXTRACT_SCALE)
        assert res.device == torch.device("cuda", 1)
        assert tensor_bytes(res) == canon(sc.extracted(cs.oracle, B))
        assert torch.cuda.current_device() == 0
    finally:
        e1.close()
