#!/usr/bin/env python3
"""On the GPU box: ms per cgpt_render call on the C3 scene (the glass dragon stand-in, level 6, in the reference layout) at 1920x1080 with
the dragon's glass (material 3) at transmission roughness 0 -- lobe level 0, the instantiations without a rough lobe -- and at 0.3 (lobe
level 2, the rough dielectric lobe), in each kernel and AUTO: a 256-sample call and a one-sample call.  Median and best of repeated calls
after a warm-up, from cgpt_stats.kernel_ms (device time of the call).  DESIGN.md 5.11.
usage: python scripts/gpu_rough_glass_time.py [repeats]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cpugpupathtracing_amd as P

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H = 1920, 1080
s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
KERNELS = (("megakernel", P.KERNEL_MEGAKERNEL), ("persistent", P.KERNEL_PERSISTENT), ("wavefront", P.KERNEL_WAVEFRONT), ("auto", P.KERNEL_AUTO))
print(f"C3 scene {W}x{H}, ADVANCED, dragon material 3; ms per call (median / best of {reps} after one warm-up)")
for rho in (0.0, 0.3):
    s.set_transmission_roughness(3, rho)
    what = f"dragon transmission roughness {rho}"
    r = P.Renderer(0)
    r.upload(s)
    for spp in (256, 1):
        for name, k in KERNELS:
            reps_k = max(1, reps // 2) if name == "megakernel" and spp == 256 else reps
            r.reset_accumulator(); r.render(W, H, spp, kernel=k)        # warm-up (allocations, occupancy queries)
            t = []
            for i in range(reps_k):
                r.reset_accumulator(); r.reset_stats()
                r.render(W, H, spp, kernel=k, seed=1000 + i)
                t.append(r.stats().kernel_ms)
            print(f"  {what:36s} spp {spp:3d}  {name:10s}  {np.median(t):8.3f} / {min(t):8.3f} ms", flush=True)
    r.close()
