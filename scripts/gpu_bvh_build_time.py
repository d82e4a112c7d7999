#!/usr/bin/env python3
"""On the GPU box: BVH::Build of the stand-in mesh on the host (csrc/host/mesh_bvh.cpp, one thread, as the reference) and on the GPU
(csrc/device/bvh_build.hip, same tree word for word: tests/test_gpu_bvh_build.py, tests/test_gpu_binned_build.py), for the reference's
SAH split intervals (ref: Source/BVH.cpp:11-45,204-366) and for the binned build.  Medians of --repeat timed calls
after one warm-up call each.
usage: python scripts/gpu_bvh_build_time.py [--option intervals|binned|both] [--repeat N] [--no-host] [levels ...]"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cpugpupathtracing_amd as P

ap = argparse.ArgumentParser()
ap.add_argument("--option", choices=("intervals", "binned", "both"), default="both")
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--no-host", action="store_true", help="skip the host builds (a profiler run wants the kernels only)")
ap.add_argument("levels", nargs="*", type=int, default=[5, 6, 7, 8])
args = ap.parse_args()
options = [("intervals", P.BUILD_SAH_INTERVALS), ("binned", P.BUILD_SAH_BINNED)]
options = [o for o in options if args.option in ("both", o[0])]


def timed(mesh, option, builder):
    s = P.Scene()
    s.add_material(P.Material())
    t0 = time.perf_counter()
    s.add_mesh(mesh, 0, option, device_builder=builder)
    return time.perf_counter() - t0, s.bvh_info(0)


r = P.Renderer(0)
for level in args.levels:
    mesh = P.Mesh.dragon_standin(level) if level < 8 else P.Mesh.bumpy_icosphere(8, (0.0, 6.0, -30.0), (24.0, 10.0, 16.0), 0.15)   # bench.py's 1.31 M-triangle scene
    n_tris = len(mesh.indices) // 3
    for name, option in options:
        first, info = timed(mesh, option, r)
        gpu = statistics.median(timed(mesh, option, r)[0] for _ in range(args.repeat))
        line = f"level {level}: {n_tris:8d} triangles, {name:9s}: depth {info.max_depth:3d}, {info.nodes_used:8d} nodes, gpu {gpu * 1e3:8.1f} ms (first call {first * 1e3:8.1f} ms)"
        if not args.no_host:
            host = statistics.median(timed(mesh, option, None)[0] for _ in range(3 if n_tris < 1000000 else 1))
            line += f", host {host * 1e3:9.1f} ms, {host / gpu:.1f}x"
        print(line, flush=True)
