#!/usr/bin/env python3
"""On the GPU box: cgpt_denoise on the C3 scene (the glass dragon stand-in, level 6, in the reference layout) at 1920x1080 after a
4-sample render, default parameters (5 passes, demodulation).  A warm call filters with the cached guides; a cold call also recomputes
them (the camera alternates between two positions 1e-4 apart, so every call sees a new camera).  Each with the packed pixels as the only
output, and with the float4 radiance as well; cgpt_read_pixels alone for the copy it shares.  Median and best of repeated calls after a
warm-up; every call ends in a synchronise (the ABI's calls block).
usage: python scripts/gpu_denoise_time.py [repeats]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
W, H = 1920, 1080
s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
r = P.Renderer(0)
r.upload(s)
r.render(W, H, 4)
L, ctx = r.L, r._ctx
cam_a = s.camera()
cam_b = N.Camera.from_buffer_copy(cam_a)
cam_b.pos[0] = cam_a.pos[0] + 1e-4
rgba = np.empty((H, W, 4), np.float32)
px = np.empty((H, W), np.uint32)
fp, up = rgba.ctypes.data_as(C.POINTER(C.c_float)), px.ctypes.data_as(C.POINTER(C.c_uint32))


def denoise(cam, with_rgba, iterations=5):
    p = N.DenoiseParams(iterations, N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    rc = L.cgpt_denoise(ctx, C.byref(cam), C.byref(p), fp if with_rgba else None, rgba.size if with_rgba else 0, up, px.size)
    assert rc == 0, L.cgpt_last_error(ctx)


def median_ms(fn):
    fn(0); fn(1)                                            # warm-up (allocations, code objects)
    t = []
    for k in range(reps):
        t0 = time.perf_counter(); fn(k); t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t)


res = {}
res["warm (5 passes), pixels"] = median_ms(lambda k: denoise(cam_a, False))
res["warm (5 passes), pixels + rgba"] = median_ms(lambda k: denoise(cam_a, True))
res["cold (guides + 5 passes), pixels"] = median_ms(lambda k: denoise(cam_b if k % 2 else cam_a, False))
res["cold (guides + 5 passes), pixels + rgba"] = median_ms(lambda k: denoise(cam_b if k % 2 else cam_a, True))
res["iterations 0, pixels"] = median_ms(lambda k: denoise(cam_a, False, 0))
res["cgpt_read_pixels"] = median_ms(lambda k: r.pixels())
print(f"C3 scene {W}x{H}, 4 spp accumulated, default parameters; {reps} calls after a warm-up")
for name, (med, best) in res.items():
    print(f"  {name:42s} median {med:8.3f} ms   best {best:8.3f} ms")
r.close()
