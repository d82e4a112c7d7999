#!/usr/bin/env python3
"""On the GPU box: cgpt_denoise_temporal against cgpt_denoise of the same build, on the C3 scene (the glass dragon stand-in, level 6, in
the reference layout) at 1920x1080 after a 4-sample render, default parameters, the packed pixels as the only output.
  static: the camera of the history (cached guides; the temporal stage maps every pixel to itself) -- the warm call;
  moving: the camera alternates between two views 0.05 apart, so every call recomputes the guides and reprojects the history of the other
          view; cgpt_denoise with the same alternation is the cold call it is compared with.
Median and best of repeated calls after a warm-up; every call ends in a synchronise (the ABI's calls block).
usage: python scripts/gpu_temporal_time.py [repeats [static|moving|all]]   (one mode alone: for a kernel trace of that mode)"""
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


def denoise(cam):
    rc = L.cgpt_denoise(ctx, C.byref(cam), None, None, 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def temporal(cam):
    rc = L.cgpt_denoise_temporal(ctx, C.byref(cam), None, None, None, 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def median_ms(fn):
    fn(0); fn(1)                                            # warm-up (allocations, code objects)
    t = []
    for k in range(reps):
        t0 = time.perf_counter(); fn(k); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t)


res = {}
if which in ("static", "all"):
    res["cgpt_denoise, warm"] = median_ms(lambda k: denoise(cam_a))
    res["cgpt_denoise_temporal, warm (same camera)"] = median_ms(lambda k: temporal(cam_a))
if which in ("moving", "all"):
    res["cgpt_denoise, cold (guides)"] = median_ms(lambda k: denoise(cam_b if k % 2 else cam_a))
    res["cgpt_denoise_temporal, moving (guides + reprojection)"] = median_ms(lambda k: temporal(cam_b if k % 2 else cam_a))
    hist = r.temporal_history()[..., 3]
    print(f"  after the moving calls {float(np.mean(hist > 4)):.1%} of the pixels carry a reprojected history (the glass first hits drop theirs)")
print(f"C3 scene {W}x{H}, 4 spp accumulated, default parameters, pixels out; {reps} calls after a warm-up")
for name, (med, best) in res.items():
    print(f"  {name:56s} median {med:8.3f} ms   best {best:8.3f} ms")
r.close()
