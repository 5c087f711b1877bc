"""Diagnostic build only (VJ_STAMPS=1 at build time, VJ_DEBUG_STAMPS=1 at run time): when the waves of the grid pass leave
their unit loop, on the bench workload (64 x 1080p, frontalface_alt) at the given tile_split values.  After every detect the
library prints, per grid launch: the launch's span in ticks of the constant 100 MHz counter (s_memrealtime: comparable across
CUs and XCDs), per workgroup the last wave's end minus the mean wave end (mean and max over workgroups, as a share of the
span), and the launch's end minus the mean over workgroups of the last wave's end.  With one workgroup per CU next to the
tiles (concurrent_blocks_per_cu 1) a workgroup is a CU's share of the pass.
Usage on the GPU box:  VJ_STAMPS=1 python -c "from clfacedetection_amd.build import build_lib; build_lib(force=True)"
                       VJ_DEBUG_STAMPS=1 python tools/grid_stamps.py 1/1.25 [frames]
"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from clfacedetection_amd import Cascade, Environment, DeviceFrames, synth
vals = (sys.argv[1] if len(sys.argv) > 1 else "1/1.25").split("/")
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
env = Environment(0); c = Cascade.load("frontalface_alt")
t = torch.from_numpy(synth.batch(B, 1080, 1920, seed0=1)).cuda(); torch.cuda.synchronize()
df = DeviceFrames.from_torch(t)
for v in vals:
    env.configure("tile_split", v)
    for rep in range(5):   # the first two are warm-up
        print(f"== tile_split {v} run {rep}", file=sys.stderr, flush=True)
        r = env.detect(c, df)
        print(f"== tile_split {v} run {rep}: cascade {r.cascade_ms:.2f} ms launches " +
              " ".join(f"{l['kind']}{l['lds_class']}:{l['ms']:.2f}" for l in r.launches), file=sys.stderr, flush=True)
