"""Build recipe of libvjhip.so (the C-ABI library declared in include/vj.h).

Everything is compiled in-tree with hipcc for gfx950 only; the resulting .so is
git-ignored but travels to the GPU box with the snapshot.  -ffp-contract=off is part
of the arithmetic contract: hipcc's default would fuse the reference's
separate multiply/add into FMAs and break bit-exact parity.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libvjhip.so")
SOURCES = ["vj_cascade.cpp", "vj_plan.cpp", "vj_clod_plan.cpp", "vj_group.cpp", "vj_env.cpp", "vj_detect.cpp", "vj_detect_regions.cpp", "vj_cv.cpp", "vj_cv_plan.cpp", "vj_cv_roi_host.cpp", "vj_cv_roi_levels_host.cpp", "vj_cv_points_host.cpp", "vj_points_host.cpp", "vj_points_driver.cpp", "vj_atlas_host.cpp", "vj_mixed.cpp", "vj_prep_host.cpp", "vj_preprocess.cpp", "vj_extract_host.cpp", "vj_extract.cpp", "vj_affine_host.cpp", "vj_extract_affine.cpp", "vj_paint_host.cpp", "vj_paint.cpp", "vj_yuv_host.cpp", "vj_yuv.cpp", "vj_paint_yuv_host.cpp", "vj_paint_yuv.cpp", "vj_extract_yuv_host.cpp", "vj_extract_yuv.cpp", "vj_track_host.cpp", "vj_track.cpp", "vj_kernels.hip",
           "vj_cv_profile.hip", "vj_cv_tile.hip", "vj_group_dev.hip", "vj_canny.hip", "vj_pyramid.hip", "vj_cv_biggest.hip", "vj_cv_roi.hip", "vj_cv_chain.hip", "vj_cv_points.hip", "vj_points.hip", "vj_atlas.hip", "vj_equalize.hip", "vj_prep.hip", "vj_extract.hip", "vj_affine.hip", "vj_paint.hip", "vj_yuv.hip", "vj_paint_yuv.hip", "vj_extract_yuv.hip", "vj_track.hip"]
HEADERS = ["vj_internal.hpp", "vj_device.hpp", "vj_env_internal.hpp", "vj_detect_host.hpp", "vj_tunables.hpp", "vj_clod_plan.hpp", "vj_cv_plan.hpp", "vj_devutil.hpp", "vj_cv_window.hpp", "vj_group_frame.hpp", "vj_cv_roi_units.hpp", "vj_cv_roi_host.hpp", "vj_cv_roi_levels_host.hpp", "vj_cv_tq_host.hpp", "vj_cv_points_units.hpp", "vj_cv_points_host.hpp", "vj_points_units.hpp", "vj_points_host.hpp", "vj_points_driver.hpp", "vj_clod_window.hpp", "vj_grid_parts.hpp", "vj_gather_queue.hpp", "vj_sq_strips.hpp", "vj_atlas_units.hpp", "vj_atlas_host.hpp", "vj_prep_units.hpp", "vj_prep_host.hpp", "vj_extract_units.hpp", "vj_extract_host.hpp", "vj_affine_units.hpp", "vj_affine_host.hpp", "vj_paint_units.hpp", "vj_paint_host.hpp", "vj_yuv_units.hpp", "vj_yuv_host.hpp", "vj_paint_yuv_units.hpp", "vj_paint_yuv_host.hpp", "vj_extract_yuv_units.hpp", "vj_extract_yuv_host.hpp", "vj_track_units.hpp", "vj_track_host.hpp", "vj_stage_host.hpp", "vj_slice.hpp", os.path.join("..", "..", "include", "vj.h")]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
         "-Wall", "-Wno-unused-function", "-fvisibility=hidden", "-DVJ_BUILDING"] + \
    (["-DVJ_STAMPS=1"] if os.environ.get("VJ_STAMPS") else []) + \
    [f"-D{k}={v}" for k, v in (kv.split("=", 1) for kv in os.environ.get("VJ_DEFINES", "").split(",") if "=" in kv)]   # experiment switches


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found; libvjhip.so cannot be built")


def _stale() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_lib(force: bool = False, verbose: bool = False) -> str:
    """Compile libvjhip.so if missing or older than its sources; returns its path."""
    if not force and not _stale():
        return LIB_PATH
    objs = []
    build_dir = os.path.join(PKG_DIR, "build")
    os.makedirs(build_dir, exist_ok=True)
    hipcc = _hipcc()
    for src in SOURCES:
        stem, ext = os.path.splitext(src)
        obj = os.path.join(build_dir, stem + ".o")
        if obj in objs:   # vj_extract.cpp and vj_extract.hip: the later one keeps its suffix in the object's name
            obj = os.path.join(build_dir, stem + "_" + ext[1:] + ".o")
        cmd = [hipcc, *FLAGS, "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stdout}\n{r.stderr}")
        objs.append(obj)
    tmp = LIB_PATH + ".tmp"
    cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", *objs, "-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
