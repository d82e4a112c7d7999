#!/usr/bin/env python3
"""On the GPU box: the one-sample-per-call configuration (profiles/r03/one_sample.md: 1080p glass stand-in level 6, n_samples = 1) with the
host's share in view: wall time per cgpt_render call beside the device time cgpt_stats books.  A regression of the host plumbing shows in
the difference.  usage: python scripts/gpu_one_sample_wall.py [calls=200]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpugpupathtracing_amd as P

calls = int(sys.argv[1].split("=")[-1]) if len(sys.argv) > 1 else 200
W, H = 1920, 1080
r = P.Renderer(0)
r.upload(P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H, P.BUILD_SAH_INTERVALS))
for kernel, name in ((P.KERNEL_AUTO, "auto"), (P.KERNEL_PERSISTENT, "persistent"), (P.KERNEL_WAVEFRONT, "wavefront")):
    r.reset_accumulator()
    for _ in range(5):
        r.render(W, H, 1, kernel=kernel)
    r.reset_stats()
    t0 = time.perf_counter()
    for _ in range(calls):
        r.render(W, H, 1, kernel=kernel)
    wall = (time.perf_counter() - t0) * 1e3 / calls
    print(f"{W}x{H} 1 sample {name:10s} wall {wall:.4f} ms/call  device {r.stats().kernel_ms / calls:.4f} ms/call  ({calls} calls)", flush=True)
r.close()
