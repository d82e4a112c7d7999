#!/usr/bin/env python3
"""On the GPU box: what posing many objects in one call (cgpt_scene_pose_objects) costs against the single calls it
replaces, on the same build and context.

  crowd   N separate stand-in meshes in a row (--levels: 3 is 1280 triangles, 4 is 5120), each with gpu_skin_time's two-joint bend, for
          every N of --counts and, with --targets K > 0 as well, with K morph targets installed and active on every object (their
          weights are posed once, outside the timed span; the timed poses give matrices, so either side runs the fused kernel once an
          object).  One side is one pose_objects call, the other N skin_mesh calls; each side ends with a synchronise; the two
          alternate in one process; warm calls only; the median of --reps (>= 20) with min / max, per call and per object.
  one     a batch of one on the 1.31 M-triangle mesh (--level 8) at --joints 2 1024 against skin_mesh, alternating: the figure a
          later change folds the single path on.
  trace   --side batch | single: --calls poses of one side of one crowd configuration and nothing else, for a kernel trace around it:
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_pose_batch_time.py trace --side batch --count 256
  summary kernels and kernel time per pose call out of the kernel trace that run wrote (no GPU needed):
          python scripts/gpu_pose_batch_time.py summary KERNEL_TRACE.csv --side batch --calls 12
  single  skin_mesh and morph_mesh of the 1.31 M-triangle mesh, warm medians, one RESULT line; --tree PATH imports the package of
          another built checkout (the parent commit's)
  ab-single  `single` of this tree against --parent-tree, --pairs alternating pairs of processes
  ab      the default bench of this tree against a built checkout of the parent commit, three alternating pairs
          (scripts/gpu_transform_time.py: ab).

usage: python scripts/gpu_pose_batch_time.py crowd [--reps 20] [--counts 1 16 64 256] [--levels 3 4] [--targets 0 8] [--out FILE.json]
       python scripts/gpu_pose_batch_time.py one [--reps 20] [--joints 2 1024] [--level 8] [--out FILE.json]
       python scripts/gpu_pose_batch_time.py trace --side batch|single [--count 256] [--mesh-level 3] [--morph-targets 0] [--calls 12]
       python scripts/gpu_pose_batch_time.py summary KERNEL_TRACE.csv --side batch|single [--calls 12]
       python scripts/gpu_pose_batch_time.py single [--reps 20] [--level 8] [--tree PATH]
       python scripts/gpu_pose_batch_time.py ab-single --parent-tree PATH [--pairs 3] [--reps 20] [--out FILE.json]
       python scripts/gpu_pose_batch_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:
    REPO = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from gpu_skin_time import _fmt, _rotation_x, _stats


def _crowd(level, count, n_targets, weights_by_batch=False):
    """(renderer, scene, matrices(phase)): `count` copies of the stand-in side by side as the objects of a scene, each skinned to two
    joints by height; with n_targets, each with the same n_targets random displacement sets installed and posed with every one active
    (by morph_mesh, or with weights_by_batch by one pose_objects call: `trace` sets them through the side it does not trace)"""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    v0 = np.array(mesh.vertices, np.float32, copy=True)
    width = float(np.ptp(v0[:, 0])) * 1.1
    r = P.Renderer(0)
    binds = []
    for k in range(count):
        v = v0.copy(); v[:, 0] += np.float32(width * (k - 0.5 * (count - 1)))
        s.add_mesh(P.Mesh.from_arrays(v, mesh.indices), 0)
        binds.append(P.triangles_from_arrays(v, mesh.indices))
    r.upload(s)
    y = binds[0].reshape(-1, 3, 6)[:, :, 1].astype(np.float64)
    t = ((y - y.min()) / (y.max() - y.min())).astype(np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); w = np.zeros(y.shape + (4,), np.float32)
    j[..., 1] = 1; w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    n = binds[0].shape[0]
    rng = np.random.default_rng(11)
    deltas = None
    if n_targets:
        deltas = rng.standard_normal((n_targets, n, 3, 6), dtype=np.float32)
        deltas[..., :3] *= np.float32(0.01 * width); deltas[..., 3:] *= np.float32(0.2)
        deltas = deltas.reshape(n_targets, n, 18)
    centres = [b.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0) for b in binds]
    for k in range(count):
        r.set_skin(k, binds[k], j, w, 2)
        if n_targets:
            r.set_morph_targets(k, binds[k], deltas)
            if not weights_by_batch:
                r.morph_mesh(k, np.full(n_targets, 0.4 / n_targets, np.float32))
    if n_targets and weights_by_batch:
        r.pose_objects([(k, None, np.full(n_targets, 0.4 / n_targets, np.float32)) for k in range(count)])
    matrices = lambda phase: [np.stack([_rotation_x(0.0, c), _rotation_x(5.0 + phase + 0.1 * k, c)]) for k, c in enumerate(centres)]
    return r, s, matrices


def _both_sides(r, matrices, reps, warm=3):
    t_batch, t_single = [], []
    for k in range(warm + reps):
        ms = matrices(k)
        entries = [(o, m, None) for o, m in enumerate(ms)]
        t0 = time.perf_counter(); r.pose_objects(entries); r.synchronize(); tb = time.perf_counter() - t0
        ms = matrices(k + 0.5)
        t0 = time.perf_counter()
        for o, m in enumerate(ms):
            r.skin_mesh(o, m)
        r.synchronize(); ts = time.perf_counter() - t0
        if k >= warm:
            t_batch.append(tb); t_single.append(ts)
    return _stats(t_batch), _stats(t_single)


def crowd(args):
    reps = max(args.reps, 20)
    out = {}
    for level in args.levels:
        for n_targets in args.targets:
            for count in args.counts:
                r, s, matrices = _crowd(level, count, n_targets)
                batch, single = _both_sides(r, matrices, reps)
                tris = 20 * 4 ** level
                name = f"{count} x {tris} triangles, {n_targets} targets"
                print(name)
                print("  " + _fmt("one pose_objects call", batch))
                print("  " + _fmt(f"{count} skin_mesh calls", single))
                print(f"  per object: batch {batch['median_ms'] / count * 1e3:.1f} us, single calls {single['median_ms'] / count * 1e3:.1f} us; "
                      f"the batch takes {batch['median_ms'] / single['median_ms']:.3f} of the single calls' time", flush=True)
                out[name] = {"batch": batch, "single": single, "count": count, "triangles": tris, "targets": n_targets}
                r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def one(args):
    from gpu_skin_time import _setup
    reps = max(args.reps, 20)
    out = {}
    for n_joints in args.joints:
        r, s, tris, j, w, matrices = _setup(args.level, n_joints)
        t_batch, t_single = [], []
        for k in range(3 + reps):
            m = matrices(5.0 + k)
            t0 = time.perf_counter(); r.pose_objects([(0, m, None)]); r.synchronize(); tb = time.perf_counter() - t0
            m = matrices(5.5 + k)
            t0 = time.perf_counter(); r.skin_mesh(0, m); r.synchronize(); ts = time.perf_counter() - t0
            if k >= 3:
                t_batch.append(tb); t_single.append(ts)
        name = f"{tris.shape[0]} triangles, {n_joints} joints"
        out[name] = {"batch_of_one": _stats(t_batch), "skin_mesh": _stats(t_single)}
        print(name)
        print("  " + _fmt("pose_objects of one entry", out[name]["batch_of_one"]))
        print("  " + _fmt("skin_mesh", out[name]["skin_mesh"]), flush=True)
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def trace(args):
    r, s, matrices = _crowd(args.mesh_level, args.count, args.morph_targets, weights_by_batch=args.side == "single")
    r.synchronize()
    for k in range(args.calls):
        ms = matrices(k)
        if args.side == "batch":
            r.pose_objects([(o, m, None) for o, m in enumerate(ms)])
        else:
            for o, m in enumerate(ms):
                r.skin_mesh(o, m)
    r.synchronize()
    print(f"{args.calls} poses of {args.count} objects, side {args.side}: level {args.mesh_level}, {args.morph_targets} targets (their weights were set through the other side's call)")
    r.close(); s.close()


def summary(args):
    """The kernels of the traced side alone: the batch's are named *_batch, the single calls' are the library's others; copies, fills and
    the other side's kernels (which set the morph weights) are listed apart."""
    import csv
    import re
    with open(args.db[0], newline="") as f:
        rows = [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(f)]
    names = {}
    for name, d in rows:
        m = re.search(r"(\w+)(<[^(]*>)?\(", name.replace("(anonymous namespace)::", ""))
        key = (m.group(1) + (m.group(2) or "")) if m else name[:60]
        c, t = names.get(key, (0, 0))
        names[key] = (c + 1, t + d)
    ours = lambda key: ("_batch" in key) == (args.side == "batch") and not key.startswith("__amd")
    count = sum(c for key, (c, t) in names.items() if ours(key))
    total = sum(t for key, (c, t) in names.items() if ours(key))
    print(f"side {args.side}: {count} kernels, {total / 1e3:.1f} us of kernel time over {args.calls} pose calls: {count / args.calls:.1f} kernels and {total / 1e3 / args.calls:.1f} us a call")
    for key, (c, t) in sorted(names.items(), key=lambda kv: -kv[1][1]):
        print(f"  {'' if ours(key) else '(not counted) '}{key:60s} {c:6d} launches {t / 1e3:10.1f} us")


def single(args):
    import numpy as np
    from gpu_skin_time import _setup
    reps = max(args.reps, 20)
    r, s, tris, j, w, matrices = _setup(args.level, 2)
    t_skin, t_morph = [], []
    for k in range(3 + reps):
        t0 = time.perf_counter(); r.skin_mesh(0, matrices(5.0 + k)); r.synchronize(); t = time.perf_counter() - t0
        if k >= 3:
            t_skin.append(t)
    rng = np.random.default_rng(3)
    d = rng.standard_normal((1, tris.shape[0], 18), dtype=np.float32) * np.float32(0.01)
    r.set_morph_targets(0, tris, d)
    for k in range(3 + reps):
        t0 = time.perf_counter(); r.morph_mesh(0, np.float32([0.1 + 0.01 * k])); r.synchronize(); t = time.perf_counter() - t0
        if k >= 3:
            t_morph.append(t)
    r.close(); s.close()
    print("RESULT " + json.dumps({"skin_mesh": _stats(t_skin)["median_ms"], "morph_and_skin_mesh": _stats(t_morph)["median_ms"]}), flush=True)


def ab_single(args):
    trees = {"this": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parent": os.path.abspath(args.parent_tree)}
    values = {"this": {}, "parent": {}}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "single", "--reps", str(args.reps), "--tree", trees[name]], cwd=trees[name],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                              # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for k, v in res.items():
                values[name].setdefault(k, []).append(v)
            print(f"{name:7s} run {pair}: " + "  ".join(f"{k}: {v:.3f} ms" for k, v in res.items()), flush=True)
    for name, v in values.items():
        for k, xs in v.items():
            print(f"{name:7s} {k}: mean {sum(xs) / len(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})")
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("crowd"); a.add_argument("--counts", type=int, nargs="+", default=[1, 16, 64, 256]); a.add_argument("--levels", type=int, nargs="+", default=[3, 4])
    a.add_argument("--targets", type=int, nargs="+", default=[0, 8])
    b = sub.add_parser("one"); b.add_argument("--joints", type=int, nargs="+", default=[2, 1024])
    c = sub.add_parser("trace"); c.add_argument("--side", choices=["batch", "single"], required=True); c.add_argument("--count", type=int, default=256)
    c.add_argument("--mesh-level", type=int, default=3); c.add_argument("--morph-targets", type=int, default=0)
    d = sub.add_parser("summary"); d.add_argument("db", nargs=1); d.add_argument("--side", choices=["batch", "single"], required=True)
    e = sub.add_parser("single"); e.add_argument("--tree")
    f = sub.add_parser("ab-single"); f.add_argument("--parent-tree", required=True); f.add_argument("--pairs", type=int, default=3)
    g = sub.add_parser("ab"); g.add_argument("--parent-tree", required=True); g.add_argument("--pairs", type=int, default=3)
    g.add_argument("--steps", type=int, default=5); g.add_argument("--warmup", type=int, default=2)
    for p in (a, b, e, f):
        p.add_argument("--reps", type=int, default=20)
    for p in (b, e):
        p.add_argument("--level", type=int, default=8)
    for p in (c, d):
        p.add_argument("--calls", type=int, default=12)
    for p in (a, b, f, g):
        p.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "ab":
        from gpu_transform_time import ab
        ab(args)
    else:
        {"crowd": crowd, "one": one, "trace": trace, "summary": summary, "single": single, "ab-single": ab_single}[args.cmd](args)
