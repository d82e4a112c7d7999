#!/usr/bin/env python3
"""On the GPU box: ms per cgpt_render call on the C3 scene (the glass dragon stand-in, level 6, in the reference layout) at 1920x1080 with
the ground (material 1) at roughness 0 -- the mirror-only instantiations -- and at specular 0.5 / roughness 0, 0.3 (the GLOSSY ones), in
each kernel: a 256-sample call and a one-sample call.  Median and best of repeated calls after a warm-up, from cgpt_stats.kernel_ms
(device time of the call).  DESIGN.md 5.9.
usage: python scripts/gpu_glossy_time.py [repeats]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cpugpupathtracing_amd as P

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
W, H = 1920, 1080
s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
n_mat = s.flatten().n_materials
KERNELS = (("megakernel", P.KERNEL_MEGAKERNEL), ("persistent", P.KERNEL_PERSISTENT), ("wavefront", P.KERNEL_WAVEFRONT), ("auto", P.KERNEL_AUTO))
print(f"C3 scene {W}x{H}, ADVANCED, ground material 1; ms per call (median / best of {reps} after one warm-up)")
for ground, rough in (("ground diffuse (shipped), roughness 0", 0.0), ("ground specular 0.5, roughness 0", 0.0), ("ground specular 0.5, roughness 0.3", 0.3)):
    if ground.startswith("ground specular"):
        s.set_material(1, P.Material(albedo=(1.0, 1.0, 1.0), specular=0.5, roughness=rough))
    r = P.Renderer(0)
    r.upload(s)
    for spp in (256, 1):
        for name, k in KERNELS:
            if name == "megakernel" and spp == 256:
                reps_k = max(1, reps // 2)
            else:
                reps_k = reps
            r.reset_accumulator(); r.render(W, H, spp, kernel=k)        # warm-up (allocations, occupancy queries)
            t = []
            for i in range(reps_k):
                r.reset_accumulator(); r.reset_stats()
                r.render(W, H, spp, kernel=k, seed=1000 + i)
                t.append(r.stats().kernel_ms)
            print(f"  {ground:40s} spp {spp:3d}  {name:10s}  {np.median(t):8.3f} / {min(t):8.3f} ms", flush=True)
    r.close()
