#!/usr/bin/env python3
"""On the GPU box: cgpt_denoise_variance_guided against cgpt_denoise and cgpt_denoise_temporal of the same build, on the C3 scene (the
glass dragon stand-in, level 6, in the reference layout) at 1920x1080 after a 4-sample render, default parameters, the packed pixels as
the only output, the camera of the render (cached guides: the warm call).
  spatial:  without CGPT_VARIANCE_TEMPORAL -- denoise_prepare, variance_estimate over every pixel's 7x7 window, five variance passes;
  temporal: with the flag and the history's camera -- the merge with the moments; after min_history_frames calls every pixel has its
            var_t and variance_estimate skips the windows;
  moving:   with the flag and a camera that alternates between two views 0.05 apart (guides recomputed, the history reprojected, the
            revealed and the glass pixels take var_s), next to cgpt_denoise and cgpt_denoise_temporal with the same alternation.
Median and best of repeated calls after a warm-up; every call ends in a synchronise (the ABI's calls block).
usage: python scripts/gpu_variance_time.py [repeats [spatial|temporal|moving|all]]   (one mode alone: for a kernel trace of that mode)"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
which = sys.argv[2] if len(sys.argv) > 2 else "all"
W, H = 1920, 1080
s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
r = P.Renderer(0)
r.upload(s)
r.render(W, H, 4)
L, ctx = r.L, r._ctx
cam_a = s.camera()
s.set_camera((0.05, 0.0, 8.0), (0.0, 0.0, -1.0), 60.0, W / H)
cam_b = s.camera()
px = np.empty((H, W), np.uint32)
up = px.ctypes.data_as(C.POINTER(C.c_uint32))
with_flag = N.VarianceParams(4.0, 4, N.VARIANCE_TEMPORAL)


def denoise(cam):
    rc = L.cgpt_denoise(ctx, C.byref(cam), None, None, 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def temporal(cam):
    rc = L.cgpt_denoise_temporal(ctx, C.byref(cam), None, None, None, 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def guided(cam, v=None):
    rc = L.cgpt_denoise_variance_guided(ctx, C.byref(cam), None, None, C.byref(v) if v is not None else None, None, 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def median_ms(fn, warm=2):
    for k in range(warm):                                   # warm-up (allocations, code objects, the history's first frames)
        fn(k)
    t = []
    for k in range(reps):
        t0 = time.perf_counter(); fn(k); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t)


res = {}
if which in ("spatial", "temporal", "all"):
    res["cgpt_denoise, warm"] = median_ms(lambda k: denoise(cam_a))
if which in ("spatial", "all"):
    res["cgpt_denoise_variance_guided, warm, spatial estimate"] = median_ms(lambda k: guided(cam_a))
if which in ("temporal", "all"):
    res["cgpt_denoise_temporal, warm (same camera)"] = median_ms(lambda k: temporal(cam_a))
    r.temporal_reset()
    res["cgpt_denoise_variance_guided + TEMPORAL, warm (same camera)"] = median_ms(lambda k: guided(cam_a, with_flag), warm=4)
if which in ("moving", "all"):
    res["cgpt_denoise, cold (guides)"] = median_ms(lambda k: denoise(cam_b if k % 2 else cam_a))
    r.temporal_reset()
    res["cgpt_denoise_temporal, moving (guides + reprojection)"] = median_ms(lambda k: temporal(cam_b if k % 2 else cam_a))
    r.temporal_reset()
    res["cgpt_denoise_variance_guided + TEMPORAL, moving"] = median_ms(lambda k: guided(cam_b if k % 2 else cam_a, with_flag), warm=4)
print(f"C3 scene {W}x{H}, 4 spp accumulated, default parameters, pixels out; {reps} calls after a warm-up")
for name, (med, best) in res.items():
    print(f"  {name:62s} median {med:8.3f} ms   best {best:8.3f} ms")
r.close()
