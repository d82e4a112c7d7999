#!/usr/bin/env python3
"""On the GPU box: what rebuilding a mesh's tree in place costs (cgpt_scene_rebuild_mesh) against the only route the
parent commit has to the same end state, and what the rebuilt tree buys a render.

  call    the stand-in at --levels (6 is 81 920 triangles, 8 is 1.31 M), skinned to two joints and bent by --bend degrees.  One side is
          Renderer.rebuild_mesh (binned and intervals) with a synchronise; the other is the old route: the pose on the host
          (Scene.skin_mesh), Scene.rebuild_bvh(device_builder), Renderer.upload and the skin installed again.  The sides alternate in one
          process; warm calls only; the median of --reps (>= 20) with min / max.
  render  the wavefront 1080p 256-spp render of the bent 81 920-triangle stand-in three ways, alternating: the refitted tree (the bind
          pose's splits), the rebuilt tree, and the bind pose itself for scale; inner_steps and tri_tests per traced ray of each.
  trace   --calls rebuilds of one option and nothing else, for a kernel trace around it:
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_rebuild_time.py trace --option binned --level 8
  summary time per kernel and call out of the kernel trace that run wrote (no GPU needed), with bytes moved over time for the kernels
          whose traffic is known:  python scripts/gpu_rebuild_time.py summary KERNEL_TRACE.csv --level 8 --calls 6
  build   cgpt_bvh_build_ex (binned) of the 1.31 M-triangle mesh, warm medians, one RESULT line; --tree PATH imports the package of
          another built checkout (the parent commit's)
  ab-build  `build` of this tree against --parent-tree, --pairs alternating pairs of processes

usage: python scripts/gpu_rebuild_time.py call [--reps 20] [--levels 6 8] [--bend 120] [--out FILE.json]
       python scripts/gpu_rebuild_time.py render [--reps 20] [--level 6] [--bend 120] [--out FILE.json]
       python scripts/gpu_rebuild_time.py trace --option binned|intervals [--level 8] [--calls 6] [--morph-targets 0]
       python scripts/gpu_rebuild_time.py summary KERNEL_TRACE.csv [--level 8] [--calls 6] [--morph-targets 0]
       python scripts/gpu_rebuild_time.py build [--reps 20] [--level 8] [--tree PATH]
       python scripts/gpu_rebuild_time.py ab-build --parent-tree PATH [--pairs 3] [--reps 20] [--out FILE.json]"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    REPO = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

from gpu_skin_time import _fmt, _rotation_x, _stats

W, H, SPP = 1920, 1080, 256
HBM_PEAK = 8.0e12                                                  # bytes / s: the MI355X's HBM3E


def _bent(level, bend):
    """(scene, bind triangles, joints, weights, matrices): the stand-in in the reference layout, a two-joint skin by height, the upper
    joint turned by `bend` degrees about the mesh's centre"""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    s = P.Scene.reference_layout(mesh, 3, 1.0, P.BUILD_SAH_INTERVALS)
    tris = P.triangles_from_arrays(mesh.vertices, mesh.indices)
    y = tris.reshape(-1, 3, 6)[:, :, 1].astype(np.float64)
    t = ((y - y.min()) / (y.max() - y.min())).astype(np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); w = np.zeros(y.shape + (4,), np.float32)
    j[..., 1] = 1; w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    centre = tris.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    m = np.stack([_rotation_x(0.0, centre), _rotation_x(bend, centre)])
    return s, tris, j, w, m


def call(args):
    import cpugpupathtracing_amd as P
    reps = max(args.reps, 20)
    out = {}
    for level in args.levels:
        s, tris, j, w, m = _bent(level, args.bend)
        r = P.Renderer(0)
        r.upload(s)
        r.set_skin(0, tris, j, w, 2)
        r.skin_mesh(0, m)
        sides = {"rebuild_mesh binned": [], "rebuild_mesh intervals": [], "host pose + rebuild_bvh(device) + upload + set_skin": [], "... of which the host pose": []}
        warm = 2
        for k in range(warm + reps):
            for name, option in (("rebuild_mesh binned", P.BUILD_SAH_BINNED), ("rebuild_mesh intervals", P.BUILD_SAH_INTERVALS)):
                t0 = time.perf_counter(); r.rebuild_mesh(0, option); r.synchronize(); dt = time.perf_counter() - t0
                if k >= warm:
                    sides[name].append(dt)
            t0 = time.perf_counter()
            s.skin_mesh(0, tris, j, w, m)
            t1 = time.perf_counter()
            s.rebuild_bvh(0, P.BUILD_SAH_BINNED, device_builder=r)
            r.upload(s)
            r.set_skin(0, tris, j, w, 2)
            r.synchronize()
            t2 = time.perf_counter()
            if k >= warm:
                sides["host pose + rebuild_bvh(device) + upload + set_skin"].append(t2 - t0)
                sides["... of which the host pose"].append(t1 - t0)
            r.skin_mesh(0, m)                                      # both sides start the next round from the posed, skinned mesh
        n = tris.shape[0]
        print(f"{n} triangles, bent {args.bend} degrees")
        stats = {name: _stats(v) for name, v in sides.items()}
        for name, st in stats.items():
            print("  " + _fmt(name, st), flush=True)
        old = stats["host pose + rebuild_bvh(device) + upload + set_skin"]
        for name in ("rebuild_mesh binned", "rebuild_mesh intervals"):
            new = stats[name]
            gap = old["median_ms"] - new["median_ms"]
            print(f"  {name}: {old['median_ms'] / new['median_ms']:.1f} x faster; the gap {gap:.3f} ms against the two spreads together {old['spread_ms'] + new['spread_ms']:.3f} ms: "
                  + ("beyond them" if gap > old["spread_ms"] + new["spread_ms"] else "NOT beyond them"))
        out[str(n)] = stats
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def render(args):
    import cpugpupathtracing_amd as P
    reps = max(args.reps, 20)
    s, tris, j, w, m = _bent(args.level, args.bend)
    ctxs = {}
    for name in ("refitted tree", "rebuilt tree", "bind pose"):
        r = P.Renderer(0)
        r.upload(s)
        if name != "bind pose":
            r.set_skin(0, tris, j, w, 2)
            r.skin_mesh(0, m)
        if name == "rebuilt tree":
            r.rebuild_mesh(0, P.BUILD_SAH_BINNED)
        ctxs[name] = r
    times = {name: [] for name in ctxs}
    per_ray = {}
    for k in range(2 + reps):
        for name, r in ctxs.items():
            r.reset_accumulator(); r.reset_stats()
            t0 = time.perf_counter(); r.render(W, H, SPP, kernel=P.KERNEL_WAVEFRONT, counters=(k == 0)); r.synchronize(); dt = time.perf_counter() - t0
            if k == 0:
                st = r.stats()
                per_ray[name] = {"traced_rays": st.traced_rays, "inner_steps_per_ray": st.inner_steps / st.traced_rays, "tri_tests_per_ray": st.tri_tests / st.traced_rays}
            elif k >= 2:
                times[name].append(dt)
    out = {}
    for name in ctxs:
        st = _stats(times[name])
        out[name] = {"render": st, **per_ray[name]}
        print(_fmt(f"{name}: {W}x{H} {SPP} spp wavefront", st))
        print(f"  inner steps / ray {per_ray[name]['inner_steps_per_ray']:.2f}, triangle tests / ray {per_ray[name]['tri_tests_per_ray']:.2f} ({per_ray[name]['traced_rays']} rays)", flush=True)
    for r in ctxs.values():
        r.close()
    s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def _rebuild_ready(level, bend, n_targets):
    import numpy as np
    import cpugpupathtracing_amd as P
    s, tris, j, w, m = _bent(level, bend)
    r = P.Renderer(0)
    r.upload(s)
    r.set_skin(0, tris, j, w, 2)
    if n_targets:
        rng = np.random.default_rng(3)
        d = (rng.standard_normal((n_targets,) + tris.shape, dtype=np.float32) * np.float32(0.001)).astype(np.float32)
        r.set_morph_targets(0, tris, d)
    r.skin_mesh(0, m)
    return r, s


def trace(args):
    import cpugpupathtracing_amd as P
    r, s = _rebuild_ready(args.level, args.bend, args.morph_targets)
    option = {"binned": P.BUILD_SAH_BINNED, "intervals": P.BUILD_SAH_INTERVALS, "naive": P.BUILD_NAIVE}[args.option]
    for _ in range(args.calls):
        r.rebuild_mesh(0, option)
    r.synchronize()
    r.close(); s.close()


def summary(args):
    n = 20 * 4 ** args.level
    # bytes a call moves through each of the new kernels whose traffic is fixed by the layouts (device_scene.h, bvh_build.hip)
    known = {"prepare_from_scene": n * (16 + 48 + 3 * 12 + 4),                 # a leaf tail and an original record read; box, centroid, index written
             "emit_leaf_triangles": n * (4 + 48 + 48),
             "emit_pair_records": (2 * n - 1) * 52 + (n - 1) * (2 * 52 + 64 + 4),   # every 52-byte BuildNode read once, a splitting node's children again; its record and level entry written
             "morph_gather_set": n * (4 + 72 + 72)}
    per = {}
    with open(args.csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name") or row.get("Name")
            t = float(row["End_Timestamp"]) - float(row["Start_Timestamp"]) if "End_Timestamp" in row else float(row["TotalDurationNs"])
            head = name.replace("(anonymous namespace)::", "").split("(")[0]
            short = (head[5:] if head.startswith("void ") else head).split("::")[-1]                 # the template arguments stay
            e = per.setdefault(short, [0, 0.0])
            e[0] += 1 if "End_Timestamp" in row else int(row.get("Calls", 1)); e[1] += t
    total = sum(v[1] for v in per.values())
    print(f"{args.calls} calls, {n} triangles: {total / args.calls / 1e6:.3f} ms of kernels a call")
    for name, (count, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        line = f"  {name:32s} {count / args.calls:8.1f} launches a call  {ns / args.calls / 1e3:10.1f} us a call"
        if name in known and count:
            each = ns / count * 1e-9
            line += f"   {known[name] / each / 1e9:8.1f} GB/s = {known[name] / each / HBM_PEAK * 100:.1f} % of the HBM peak"
        print(line)


def build(args):
    import ctypes as C
    import numpy as np
    import cpugpupathtracing_amd as P
    from cpugpupathtracing_amd import _native as N
    reps = max(args.reps, 20)
    mesh = P.Mesh.dragon_standin(args.level)
    tris = np.ascontiguousarray(P.triangles_from_arrays(mesh.vertices, mesh.indices), np.float32)
    r = P.Renderer(0)
    ptr = tris.ctypes.data_as(C.POINTER(N.Triangle))
    ts = []
    for k in range(2 + reps):
        t0 = time.perf_counter(); r.build_bvh(ptr, tris.shape[0], P.BUILD_SAH_BINNED); dt = time.perf_counter() - t0
        if k >= 2:
            ts.append(dt)
    st = _stats(ts)
    print(_fmt(f"cgpt_bvh_build_ex binned, {tris.shape[0]} triangles", st))
    print("RESULT " + json.dumps(st), flush=True)
    r.close()


def ab_build(args):
    trees = {"this": REPO, "parent": os.path.abspath(args.parent_tree)}
    values = {"this": [], "parent": []}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "build", "--reps", str(args.reps), "--tree", trees[name]], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                                  # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            values[name].append(res)
            print(f"{name:7s} run {pair}: median {res['median_ms']:.3f} ms (min {res['min_ms']:.3f}, max {res['max_ms']:.3f})", flush=True)
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("call"); a.add_argument("--reps", type=int, default=20); a.add_argument("--levels", type=int, nargs="+", default=[6, 8])
    a.add_argument("--bend", type=float, default=120.0); a.add_argument("--out")
    b = sub.add_parser("render"); b.add_argument("--reps", type=int, default=20); b.add_argument("--level", type=int, default=6)
    b.add_argument("--bend", type=float, default=120.0); b.add_argument("--out")
    c = sub.add_parser("trace"); c.add_argument("--option", default="binned"); c.add_argument("--level", type=int, default=8); c.add_argument("--calls", type=int, default=6)
    c.add_argument("--bend", type=float, default=120.0); c.add_argument("--morph-targets", type=int, default=0)
    d = sub.add_parser("summary"); d.add_argument("csv"); d.add_argument("--level", type=int, default=8); d.add_argument("--calls", type=int, default=6)
    d.add_argument("--morph-targets", type=int, default=0)
    e = sub.add_parser("build"); e.add_argument("--reps", type=int, default=20); e.add_argument("--level", type=int, default=8); e.add_argument("--tree")
    f = sub.add_parser("ab-build"); f.add_argument("--parent-tree", required=True); f.add_argument("--pairs", type=int, default=3); f.add_argument("--reps", type=int, default=20); f.add_argument("--out")
    args = ap.parse_args()
    {"call": call, "render": render, "trace": trace, "summary": summary, "build": build, "ab-build": ab_build}[args.cmd](args)


if __name__ == "__main__":
    main()
