#!/usr/bin/env python3
"""On the GPU box: the C3 workload of bench.py (1080p, 256 spp, glass stand-in of 81 920 triangles, wavefront pipeline) with the mesh's
tree built by SAH split intervals and by the binned build: render time per frame, traversal counters per ray.  The
images differ in the last bits at most (another tree, another traversal order of equal hits); this script compares times, not pixels.
usage: python scripts/gpu_binned_render_ab.py [--steps N] [--warmup N] [--level L]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpugpupathtracing_amd as P

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--level", type=int, default=6)
args = ap.parse_args()
W, H, SPP = 1920, 1080, 256
mesh = P.Mesh.dragon_standin(args.level)
r = P.Renderer(0)
for rnd in range(2):                                       # both options twice, alternated: drift of the box shows as a difference between rounds
    for name, option in (("intervals", P.BUILD_SAH_INTERVALS), ("binned", P.BUILD_SAH_BINNED)):
        r.upload(P.Scene.reference_layout(mesh, 3, W / H, option))
        times = []
        for step in range(args.warmup + args.steps):
            r.reset_accumulator(); r.reset_stats()
            t0 = time.perf_counter()
            r.render(W, H, SPP, kernel=P.KERNEL_WAVEFRONT)
            r.synchronize()
            if step >= args.warmup:
                times.append(time.perf_counter() - t0)
        r.reset_accumulator(); r.reset_stats()
        r.render(W, H, 4, kernel=P.KERNEL_WAVEFRONT, counters=True)
        st = r.stats()
        print(f"round {rnd} {name:9s}: median {statistics.median(times) * 1e3:7.2f} ms, min {min(times) * 1e3:7.2f} ms per {SPP}-spp frame ({args.steps} frames); "
              f"inner steps per ray {st.inner_steps / st.traced_rays:.2f}, triangle tests per ray {st.tri_tests / st.traced_rays:.2f}", flush=True)
