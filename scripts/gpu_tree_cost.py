#!/usr/bin/env python3
"""On the GPU box: does the tree cost of cgpt_scene_tree_costs predict the work of a render, and what does the call cost.

  predict  the 81 920-triangle stand-in (--level 6) bent by each of --bends degrees, as gpu_rebuild_time.py bends it.  Per angle: the cost
           of the refitted tree and of the tree rebuilt with the binned builder, each over the cost at the bind pose, and beside them
           inner_steps / traced_rays of the wavefront 1080p render (--spp samples, counters on) through either tree.  The table a
           ratio for cgpt_scene_rebuild_degraded would be chosen from -- if the two columns move together.
  call     Renderer.tree_costs of N = --crowds characters of 1 280 triangles in one call, and of the stand-in at --levels, against the
           only older route to the number: Renderer.export_bvh per object and the host mirror (tree_cost) over it.  The sides alternate
           in one process; warm calls; the median of --reps (>= 20) with min / max.
  trace    --calls cost calls of the stand-in at --level and nothing else, for a kernel trace around it:
           rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_tree_cost.py trace --level 8
           tree_cost_batch reads 64 B a record and a 4-byte name; a float4 copy reaches 6.3 TB/s on this device.

usage: python scripts/gpu_tree_cost.py predict [--level 6] [--bends 0 30 60 90 120] [--spp 256] [--out FILE.json]
       python scripts/gpu_tree_cost.py call [--reps 20] [--crowds 1 16 64 256] [--levels 6 8] [--out FILE.json]
       python scripts/gpu_tree_cost.py trace [--level 8] [--calls 20]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

from gpu_rebuild_time import H, W, _bent
from gpu_skin_time import _fmt, _rotation_x, _stats


def predict(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    s, tris, j, w, _ = _bent(args.level, 0.0)
    centre = tris.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    r = P.Renderer(0)
    r.upload(s)
    bind = float(r.tree_costs([0])["cost"][0])
    r.set_skin(0, tris, j, w, 2)
    rows = []
    print(f"{tris.shape[0]} triangles; bind-pose cost {bind:.4f}; wavefront {W}x{H}, {args.spp} spp")
    print("bend  refitted: cost/bind  steps/ray   rebuilt: cost/bind  steps/ray")
    for bend in args.bends:
        r.upload(s)                                                # every angle starts from the bind tree
        r.set_skin(0, tris, j, w, 2)
        r.skin_mesh(0, np.stack([_rotation_x(0.0, centre), _rotation_x(bend, centre)]))
        row = {"bend": bend}
        for name in ("refitted", "rebuilt"):
            if name == "rebuilt":
                r.rebuild_mesh(0, P.BUILD_SAH_BINNED)
            cost = float(r.tree_costs([0])["cost"][0])
            r.reset_accumulator(); r.reset_stats()
            r.render(W, H, args.spp, kernel=P.KERNEL_WAVEFRONT, counters=True)
            st = r.stats()
            row[name] = {"cost": cost, "cost_over_bind": cost / bind, "inner_steps_per_ray": st.inner_steps / st.traced_rays, "traced_rays": st.traced_rays}
        rows.append(row)
        print(f"{bend:5.0f}  {row['refitted']['cost_over_bind']:19.4f}  {row['refitted']['inner_steps_per_ray']:9.3f}   {row['rebuilt']['cost_over_bind']:18.4f}  "
              f"{row['rebuilt']['inner_steps_per_ray']:9.3f}", flush=True)
    r.close(); s.close()
    if args.out:
        json.dump({"bind_cost": bind, "rows": rows}, open(args.out, "w"), indent=1)


def _alternate(r, objs, reps):
    import cpugpupathtracing_amd as P
    sides = {"tree_costs (device)": [], "export_bvh + host mirror": []}
    for k in range(2 + reps):
        t0 = time.perf_counter(); dev = r.tree_costs(objs); t1 = time.perf_counter()
        host = [P.tree_cost(r.export_bvh(o)).cost for o in objs]
        t2 = time.perf_counter()
        if k >= 2:
            sides["tree_costs (device)"].append(t1 - t0)
            sides["export_bvh + host mirror"].append(t2 - t1)
    worst = max(abs(d / h - 1.0) for d, h in zip(dev["cost"], host))
    return {name: _stats(v) for name, v in sides.items()}, worst


def call(args):
    import cpugpupathtracing_amd as P
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from skin_cases import strip_mesh
    reps = max(args.reps, 20)
    out = {}
    for n in args.crowds:
        s = P.Scene()
        s.add_material(P.Material())
        for k in range(n):
            s.add_mesh(P.Mesh.from_arrays(*strip_mesh(1280, origin=(0.0, 1.5 * k, 0.0))), 0, P.BUILD_SAH_INTERVALS)
        s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=5.0, is_light=True))
        s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 1))
        s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
        s.set_settings(P.Settings())
        r = P.Renderer(0)
        r.upload(s)
        stats, worst = _alternate(r, list(range(n)), reps)
        print(f"{n} characters of 1 280 triangles, one call (device and mirror agree to {worst:.1e})")
        for name, st in stats.items():
            print("  " + _fmt(name, st), flush=True)
        out[f"crowd_{n}"] = stats
        r.close(); s.close()
    for level in args.levels:
        s, tris, _, _, _ = _bent(level, 0.0)
        r = P.Renderer(0)
        r.upload(s)
        stats, worst = _alternate(r, [0], reps)
        print(f"{tris.shape[0]} triangles, one mesh (device and mirror agree to {worst:.1e}; the export reads back {64 * (tris.shape[0] - 1) / 1e6:.1f} MB of records)")
        for name, st in stats.items():
            print("  " + _fmt(name, st), flush=True)
        out[f"mesh_{tris.shape[0]}"] = stats
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def trace(args):
    import cpugpupathtracing_amd as P
    s, tris, _, _, _ = _bent(args.level, 0.0)
    r = P.Renderer(0)
    r.upload(s)
    for _ in range(args.calls):
        r.tree_costs([0])
    print(f"{args.calls} calls over {tris.shape[0] - 1} records: tree_cost_batch reads {68 * (tris.shape[0] - 1) / 1e6:.2f} MB a call")
    r.close(); s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("predict", "call", "trace"))
    ap.add_argument("--level", type=int, default=None)
    ap.add_argument("--levels", type=int, nargs="*", default=[6, 8])
    ap.add_argument("--bends", type=float, nargs="*", default=[0.0, 30.0, 60.0, 90.0, 120.0])
    ap.add_argument("--crowds", type=int, nargs="*", default=[1, 16, 64, 256])
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.level is None:
        a.level = 8 if a.mode == "trace" else 6
    {"predict": predict, "call": call, "trace": trace}[a.mode](a)
