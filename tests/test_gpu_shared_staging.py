"""What the frame-processing calls share: ONE environment with max_subbatch 1 runs paint, extract, paint_yuv,
preprocess, yuv_to_bgr, extract_affine, track and paint again on pageable host frames, so that the page-locked staging buffer and the
device blocks grow, are reused by a smaller call and are reused across entry points, and one pair of events times every call.  Every
result is compared exactly with the numpy restatement its own test uses (tests/*_cases.py), and after every call every byte of every
host buffer — row padding and the sentinels around the planes included — with what the paint calls so far must have left there.
These paths are bit-exact: no tolerance."""
import numpy as np
import pytest

import affine_cases as ac
import extract_cases as ec
import paint_cases as pcs
import paint_yuv_cases as pyc
import prep_cases as pc
import track_cases as tc
import yuv_cases as yc
from clfacedetection_amd import Environment
from test_gpu_paint import Frame
from test_gpu_paint_yuv import Frame as YuvFrame
from test_gpu_prep import download
from test_gpu_yuv import check_decode

pytestmark = pytest.mark.gpu


def test_one_environment_through_every_entry_point(oracle):
    rng = np.random.default_rng(424)
    small = [rng.integers(0, 256, (23, 37, 3), dtype=np.uint8) for _ in range(2)]              # two 37 x 23 BGR frames
    big = rng.integers(0, 256, (67, 130, 3), dtype=np.uint8)                                   # one 130 x 67 frame
    planes = pyc.frame(38, 22, yc.NV12, 7)                                                     # one 38 x 22 NV12 frame
    fs = [Frame(small[0], "host", 1, 3), Frame(small[1], "host", 2, 5)]                        # rows 3 and 5 bytes further apart
    fy = YuvFrame(planes, yc.NV12, "host", (1, 3, 0), 2)
    big_before = big.copy()
    env = Environment(0)
    try:
        env.configure("max_subbatch", "1")
        state = {"small": small, "planes": planes}

        def host_memory_is(what):
            for i, f in enumerate(fs):
                assert np.array_equal(f.now(), f.want(state["small"][i])), (what, "frame", i)
            assert np.array_equal(fy.now(), fy.want(state["planes"])), (what, "nv12")
            assert np.array_equal(big, big_before), what

        # 1. paint (blur) on the two small frames: two slices, regions that overlap and one that leaves the frame
        rects = [(0, 2, 3, 20, 12), (1, 10, 5, 30, 30), (0, 15, 8, 12, 9), (1, -4, 1, 9, 7), (1, 36, 22, 1, 1)]
        state["small"] = pcs.restate(state["small"], rects, "blur", size=5)
        assert any(not np.array_equal(a, b) for a, b in zip(state["small"], small))
        env.paint([f.item for f in fs], rects, "blur", size=5)
        assert env.paint_timing() > 0
        host_memory_is("paint")
        # 2. extract from the large frame: the staging buffer and d_extract grow
        crops = [(0, 5, 4, 60, 40), (0, -6, 50, 40, 30), (0, 100, 10, 30, 57)]
        got = env.extract([big], crops, (24, 18)).cpu().numpy()
        assert np.array_equal(got, ec.restate(oracle, [big], crops, (24, 18)))
        assert env.extract_timing() > 0
        host_memory_is("extract")
        # 3. paint_yuv (pixelate) on the NV12 frame: a smaller call in the grown buffers
        yrects = [(0, 3, 2, 17, 11), (0, 20, 9, 30, 30), (0, 11, 7, 6, 5)]
        state["planes"] = pyc.restate([state["planes"]], [yc.NV12], yrects, "pixelate", size=3)[0]
        assert any(not np.array_equal(a, b) for a, b in zip(state["planes"], planes))
        env.paint_yuv([fy.item], yrects, "pixelate", size=3, layout="nv12")
        assert env.paint_yuv_timing() > 0
        host_memory_is("paint_yuv")
        # 4. preprocess of the large frame
        img, w = download(env.preprocess([big], size=(65, 33), equalize=True))[0]
        want = pc.restate(oracle, big, size=(65, 33), equalize=True)
        assert w == want.shape[1] and np.array_equal(img[:, :w], want) and not img[:, w:].any()
        assert env.preprocess_timing() > 0
        host_memory_is("preprocess")
        # 5. yuv_to_bgr of the painted NV12 frame, every byte of the destination
        check_decode(env, [fy.item], [state["planes"]], [yc.NV12], False, False)
        assert env.yuv_timing() > 0
        host_memory_is("yuv_to_bgr")
        # 6. extract_affine from the painted small frames
        rows = np.concatenate([ac.rows_for(0, [ac.identity(), ac.ROT]), ac.rows_for(1, [ac.translation(-3.0, 4.0), ac.SHEAR])])
        got = env.extract_affine([f.item for f in fs], rows, ac.ROT_SIZE).cpu().numpy()
        assert np.array_equal(got, ac.restate(oracle, state["small"], rows, ac.ROT_SIZE))
        assert env.extract_affine_timing() > 0
        host_memory_is("extract_affine")
        # 7. track between the two small frames, both ways
        trows = [(0, 1, 8, 6, 12, 12), (1, 0, 20, 9, 10, 11), (0, 1, -3, 15, 12, 12)]
        got = env.track([f.item for f in fs], trows, tmpl=8, radius=3)
        assert tc.equal(got, tc.restate(oracle, state["small"], trows, 8, 3))
        assert env.track_timing()[0] > 0
        host_memory_is("track")
        # 8. paint again on the first frames, from what the first call left
        rects = [(1, 0, 0, 37, 23), (0, 30, 15, 20, 20), (0, 1, 1, 6, 21)]
        state["small"] = pcs.restate(state["small"], rects, "pixelate", size=4)
        env.paint([f.item for f in fs], rects, "pixelate", size=4)
        host_memory_is("paint again")
    finally:
        env.close()
