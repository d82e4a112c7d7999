#!/usr/bin/env python3
"""On the GPU box: what posing a mesh from morph targets on the device (cgpt_scene_morph_mesh) costs against the refit
a caller had before it, alone and fused with a skin, and in either stored layout.  The mesh is the 1.31 M-triangle stand-in
(dragon_standin(8)) with --targets (52) targets installed; K of them are active in a pose, the others have weight zero.

  pose    warm calls only, each ended by a synchronise: morph_mesh per call and refit_mesh per call of the same build, given the host
          mirror's triangles of the same pose (the host's own posing time, cgpth_morph_triangles, is reported beside it), alternating,
          the median of --reps (>= 20) with min / max, for every K of --active and for the targets stored in leaf-slot order and as
          given; then the same with a two-joint skin installed and posed (morph + skin in one kernel, against the refit of the host's
          composition).  The acceptance comparison: the device call must be faster than refit_mesh by more than the two spreads together.
  trace   a fixed number of poses per K and layout, without and with the skin, plus plain skin poses, for a kernel trace around it:
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_morph_time.py trace
  summary the kernels' times out of the kernel trace that run wrote (DIR/.../*_kernel_trace.csv), in launch order per configuration, with the bytes
          each must move and the rate (no GPU needed): python scripts/gpu_morph_time.py summary KERNEL_TRACE.csv --active 1 8 52
  ab      the default bench of this tree against a built checkout of the parent commit, three alternating pairs
          (scripts/gpu_transform_time.py: ab).

usage: python scripts/gpu_morph_time.py pose [--reps 20] [--active 1 8 52] [--targets 52] [--level 8] [--out FILE.json]
       python scripts/gpu_morph_time.py trace [--active 1 8 52] [--targets 52] [--calls 10] [--level 8]
       python scripts/gpu_morph_time.py summary KERNEL_TRACE.csv [--active 1 8 52] [--calls 10]
       python scripts/gpu_morph_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_skin_time import _fmt, _rotation_x, _stats


def _setup(level, n_targets):
    """(renderer, scene, base triangles, deltas, skin): the stand-in as the one object of a scene.  Target 0 is random displacements of a
    hundredth of the mesh's size and a fifth of a normal; the others are that array rolled along the triangles, so that the 5 GB of 52
    targets cost no random numbers.  The skin is gpu_skin_time's two-joint bend."""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    r = P.Renderer(0)
    s.add_mesh(mesh, 0, P.BUILD_SAH_INTERVALS, device_builder=r)
    r.upload(s)
    tris = P.triangles_from_arrays(mesh.vertices, mesh.indices)
    n = tris.shape[0]
    rng = np.random.default_rng(11)
    size = float(np.ptp(tris.reshape(-1, 6)[:, :3], axis=0).max())
    d0 = rng.standard_normal((n, 3, 6), dtype=np.float32)
    d0[..., :3] *= np.float32(0.01 * size); d0[..., 3:] *= np.float32(0.2)
    d0 = d0.reshape(n, 18)
    deltas = np.empty((n_targets, n, 18), np.float32)
    for k in range(n_targets):
        deltas[k] = np.roll(d0, 7919 * k, axis=0)
    y = tris.reshape(-1, 3, 6)[:, :, 1].astype(np.float64)
    t = ((y - y.min()) / (y.max() - y.min())).astype(np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); w = np.zeros(y.shape + (4,), np.float32)
    j[..., 1] = 1; w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    centre = tris.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)
    matrices = lambda deg: np.stack([_rotation_x(0.0, centre), _rotation_x(deg, centre)])
    return r, s, tris, deltas, (j, w, matrices)


def _weights(n_targets, k_active, phase):
    """k_active nonzero weights spread over the n_targets, small enough that 52 of them leave a mesh; phase varies them from call to call"""
    import numpy as np
    w = np.zeros(n_targets, np.float32)
    idx = np.linspace(0, n_targets - 1, k_active).round().astype(int)
    w[idx] = (0.5 + 0.02 * phase) / k_active * np.where(np.arange(k_active) % 2, -1.0, 1.0) + 0.3 / k_active
    return w


def pose(args):
    import cpugpupathtracing_amd as P
    reps = max(args.reps, 20)
    r, s, tris, deltas, (j, sw, matrices) = _setup(args.level, args.targets)
    out = {"triangles": int(tris.shape[0]), "targets": args.targets}
    print(f"{tris.shape[0]} triangles, {args.targets} targets installed", flush=True)
    for skinned in (False, True):
        if skinned:
            r.set_skin(0, tris, j, sw, 2)
            r.skin_mesh(0, matrices(20.0))
        results, composed = {}, {}
        for k_active in args.active:                                           # the refit's input: two poses, alternated so no call repeats the last
            t_host, composed[k_active] = [], []
            for k in range(2):
                t0 = time.perf_counter(); m = P.morph_triangles(tris, deltas, _weights(args.targets, k_active, k)); t_host.append(time.perf_counter() - t0)
                if skinned:
                    m = P.skin_triangles(m, j, sw, matrices(20.0))
                    t_host[-1] = time.perf_counter() - t0
                composed[k_active].append(m)
            results[k_active] = {"host_morph_and_skin" if skinned else "host_morph_triangles": _stats(t_host)}
        for leaf in (1, 0):
            r.set_tuning(morph_leaf_order=leaf)
            r.set_morph_targets(0, tris, deltas)
            for k_active in args.active:
                for k in range(3):                                             # warm-up: allocations, first launches
                    r.morph_mesh(0, _weights(args.targets, k_active, k)); r.refit_mesh(0, composed[k_active][k & 1])
                t_morph, t_refit = [], []
                for k in range(reps):
                    w = _weights(args.targets, k_active, 3 + k)
                    t0 = time.perf_counter(); r.morph_mesh(0, w); r.synchronize(); t_morph.append(time.perf_counter() - t0)
                    t0 = time.perf_counter(); r.refit_mesh(0, composed[k_active][k & 1]); r.synchronize(); t_refit.append(time.perf_counter() - t0)
                results[k_active]["morph_mesh_leaf_order" if leaf else "morph_mesh_as_given"] = _stats(t_morph)
                results[k_active]["refit_mesh" if leaf else "refit_mesh_again"] = _stats(t_refit)
        for k_active, res in results.items():
            name = f"K={k_active}{' + skin' if skinned else ''}"
            print(name)
            for key in res:
                print("  " + _fmt(key, res[key]), flush=True)
            a, b, c = res["morph_mesh_leaf_order"], res["refit_mesh"], res["morph_mesh_as_given"]
            margin = b["median_ms"] - a["median_ms"]
            res["faster_by_ms"] = margin; res["combined_spread_ms"] = a["spread_ms"] + b["spread_ms"]
            res["accepted"] = bool(margin > res["combined_spread_ms"])
            print(f"  morph_mesh is faster than refit_mesh by {margin:.3f} ms ({b['median_ms'] / a['median_ms']:.1f}x); the two spreads together are "
                  f"{res['combined_spread_ms']:.3f} ms: {'ACCEPTED' if res['accepted'] else 'NOT ACCEPTED'}")
            gain = c["median_ms"] - a["median_ms"]
            res["leaf_order_gain_ms"] = gain; res["layout_spreads_ms"] = a["spread_ms"] + c["spread_ms"]
            print(f"  leaf-slot order is faster than as given by {gain:.3f} ms per call; the two spreads together are {res['layout_spreads_ms']:.3f} ms", flush=True)
            out[name] = res
    r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)
    if not all(v["accepted"] for v in out.values() if isinstance(v, dict)):
        sys.exit(1)


def trace(args):
    r, s, tris, deltas, (j, sw, matrices) = _setup(args.level, args.targets)
    for skinned in (False, True):
        if skinned:
            r.clear_morph_targets(0)
            r.set_skin(0, tris, j, sw, 2)
            for k in range(args.calls + 1):                                    # the plain skin kernel (no targets installed), for its rate in the same session
                r.skin_mesh(0, matrices(10.0 + k))
        for leaf in (1, 0):
            r.set_tuning(morph_leaf_order=leaf)
            r.set_morph_targets(0, tris, deltas)
            for k_active in args.active:
                for k in range(args.calls + 1):
                    r.morph_mesh(0, _weights(args.targets, k_active, k))
    r.synchronize()
    print(f"{args.calls + 1} poses each: skin no/yes x leaf order 1/0 x K in {args.active}; {args.calls + 1} plain skin poses")
    r.close(); s.close()


def summary(args):
    """From the kernel trace (--output-format csv: *_kernel_trace.csv) rocprofv3 wrote around `trace`: the launches of morph_triangles come in groups of calls + 1 in the order
    trace makes them; the first of a group (cold for that K) is left out.  Bytes a triangle: 72 (K + 1) read + 48 of the leaf record
    rewritten (16 of them read first) + 48 + 48 of the original-order and the normal records = 72 K + 232, plus 72 of joints and weights
    with the skin; skin_triangles: 72 + 72 read, 160 written and read = 304."""
    import csv
    import statistics
    with open(args.db[0], newline="") as f:
        rows = sorted(((r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), int(r["Start_Timestamp"])) for r in csv.DictReader(f)), key=lambda x: x[2])
    n_tris = args.triangles
    skin = [d / 1e3 for name, d, g in rows if "skin_triangles" in name][1:]
    if skin:
        m = statistics.median(skin)
        print(f"skin_triangles<true>            median {m:8.2f} us (min {min(skin):.2f}, max {max(skin):.2f}; {len(skin)} launches)  {304 * n_tris / m / 1e6:6.2f} TB/s of 304 B a triangle")
    morph = [(name, d / 1e3) for name, d, g in rows if "morph_triangles" in name]
    per = args.calls + 1
    groups = [(sk, leaf, k) for sk in (0, 1) for leaf in (1, 0) for k in args.active]
    assert len(morph) == per * len(groups), (len(morph), per, len(groups))
    med = {}
    for gi, (sk, leaf, k) in enumerate(groups):
        d = [x[1] for x in morph[gi * per + 1:(gi + 1) * per]]
        m = statistics.median(d)
        med[(sk, leaf, k)] = m
        nbytes = 72 * k + 232 + 72 * sk
        print(f"morph_triangles skin {sk} leaf order {leaf} K {k:3d}: median {m:8.2f} us (min {min(d):.2f}, max {max(d):.2f}; {len(d)} launches)  "
              f"{nbytes * n_tris / m / 1e6:6.2f} TB/s of {nbytes} B a triangle")
    for sk in (0, 1):
        for leaf in (1, 0):
            ks = sorted(args.active)
            if len(ks) > 1:
                slope = (med[(sk, leaf, ks[-1])] - med[(sk, leaf, ks[0])]) / (ks[-1] - ks[0])
                print(f"skin {sk} leaf order {leaf}: {slope:.2f} us per added active target ({72 * n_tris / slope / 1e6:.2f} TB/s of its 72 B a triangle)")
    levels = [d / 1e3 for name, d, g in rows if "refit_level" in name]
    poses = per * (len(groups) + 1)                                            # what `trace` calls: per morph_mesh a group, per skin_mesh without targets
    print(f"refit_level: {len(levels)} launches in {poses} poses, {sum(levels) / poses:.1f} us per pose")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("pose"); a.add_argument("--reps", type=int, default=20); a.add_argument("--out")
    b = sub.add_parser("trace")
    d = sub.add_parser("summary"); d.add_argument("db", nargs=1); d.add_argument("--triangles", type=int, default=1310720)
    for p in (a, b, d):
        p.add_argument("--active", type=int, nargs="+", default=[1, 8, 52])
    for p in (a, b):
        p.add_argument("--targets", type=int, default=52); p.add_argument("--level", type=int, default=8)
    for p in (b, d):
        p.add_argument("--calls", type=int, default=10)
    c = sub.add_parser("ab"); c.add_argument("--parent-tree", required=True); c.add_argument("--pairs", type=int, default=3)
    c.add_argument("--steps", type=int, default=5); c.add_argument("--warmup", type=int, default=2); c.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "ab":
        from gpu_transform_time import ab
        ab(args)
    else:
        {"pose": pose, "trace": trace, "summary": summary}[args.cmd](args)
