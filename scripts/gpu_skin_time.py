#!/usr/bin/env python3
"""On the GPU box: what posing a skinned mesh on the device (cgpt_scene_skin_mesh) costs against the refit a caller had
before it.  The mesh is the 1.31 M-triangle stand-in (dragon_standin(8)) with a two-joint bend unless --joints says otherwise.

  pose    warm calls only: skin_mesh per call and refit_mesh per call of the same build, given the host mirror's triangles of the same pose
          (the host's own posing time, cgpth_skin_triangles, is reported beside it), alternating, the median of --reps (>= 20) with
          min / max; then the acceptance comparison: skin_mesh must be faster than refit_mesh by more than the two spreads together.
          With --joints 2 64 1024 also skin_mesh with the joint matrices in LDS and through the vector cache at each count (wall time).
  trace   a fixed number of poses (LDS), poses (vector cache) and refits for a kernel trace around it, one process per joint count:
          rocprofv3 --kernel-trace --stats -- python scripts/gpu_skin_time.py trace --joints 64
          gives skin_triangles<true>, skin_triangles<false>, refit_triangles and refit_level their own times; skin_mesh's host remainder
          is `pose`'s wall time minus the kernels.
  summary the kernels' times out of the result databases those rocprofv3 runs wrote (no GPU needed):
          python scripts/gpu_skin_time.py summary DIR/skin_results.db ...
  ab      the default bench of this tree against a built checkout of the parent commit, three alternating pairs
          (scripts/gpu_transform_time.py: ab).

usage: python scripts/gpu_skin_time.py pose [--reps 20] [--joints 2 64 1024] [--level 8] [--random-joints] [--out FILE.json]
       python scripts/gpu_skin_time.py trace [--joints 2] [--calls 20] [--level 8] [--random-joints]
       python scripts/gpu_skin_time.py summary RESULTS.db [RESULTS.db ...]
       python scripts/gpu_skin_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _rotation_x(deg, about):
    import numpy as np
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    a = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.concatenate([a, (about - a @ about)[:, None]], axis=1).astype(np.float32).reshape(12)


def _setup(level, n_joints, random_joints=False):
    """(renderer, bind triangles, joints, weights, matrices(deg)): the stand-in as the one object of a scene, skinned to n_joints joints:
    a corner's two influences are the joints below and above its height, so 2 joints are the bend and more joints a chain of bends.
    random_joints: four uniformly random joints and random weights per corner instead -- no two lanes agree, the worst case for the
    LDS banks and the cache alike (not a character, a stress case)."""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    r = P.Renderer(0)
    s.add_mesh(mesh, 0, P.BUILD_SAH_INTERVALS, device_builder=r)
    r.upload(s)
    tris = P.triangles_from_arrays(mesh.vertices, mesh.indices)
    y = tris.reshape(-1, 3, 6)[:, :, 1].astype(np.float64)
    h = (y - y.min()) / (y.max() - y.min()) * (n_joints - 1)
    below = np.minimum(np.floor(h), max(n_joints - 2, 0)).astype(np.int64)
    t = (h - below).astype(np.float32) if n_joints > 1 else np.zeros_like(h, np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); w = np.zeros(y.shape + (4,), np.float32)
    j[..., 0] = below; j[..., 1] = np.minimum(below + 1, n_joints - 1)
    w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    if random_joints:
        rng = np.random.default_rng(7)
        j[:] = rng.integers(0, n_joints, j.shape).astype(np.uint16)
        x = rng.uniform(0.1, 1.0, w.shape)
        w[:] = (x / x.sum(-1, keepdims=True)).astype(np.float32)
    centre = tris.reshape(-1, 6)[:, :3].astype(np.float64).mean(axis=0)

    def matrices(deg):
        return np.stack([_rotation_x(deg * k / max(n_joints - 1, 1), centre) for k in range(n_joints)])
    r.set_skin(0, tris, j, w, n_joints)
    return r, s, tris, j, w, matrices


def _stats(xs):
    import numpy as np
    xs = np.asarray(xs) * 1e3
    return {"median_ms": float(np.median(xs)), "min_ms": float(xs.min()), "max_ms": float(xs.max()), "spread_ms": float(xs.max() - xs.min()), "n": len(xs)}


def _fmt(name, st):
    return f"{name}: median {st['median_ms']:.3f} ms (min {st['min_ms']:.3f}, max {st['max_ms']:.3f}, spread {st['spread_ms']:.3f}; {st['n']} warm calls)"


def pose(args):
    import cpugpupathtracing_amd as P
    reps = max(args.reps, 20)
    out = {}
    for n_joints in args.joints:
        r, s, tris, j, w, matrices = _setup(args.level, n_joints, args.random_joints)
        posed = [P.skin_triangles(tris, j, w, matrices(5.0 + k)) for k in range(2)]   # the refit's input, alternated so no call repeats the last
        t_host = []
        for k in range(3):
            t0 = time.perf_counter(); P.skin_triangles(tris, j, w, matrices(7.0 + k)); t_host.append(time.perf_counter() - t0)
        for k in range(3):                                     # warm-up: allocations, first launches
            r.skin_mesh(0, matrices(1.0 + k)); r.refit_mesh(0, posed[k & 1])
        t_skin, t_refit, t_vc = [], [], []
        for k in range(reps):
            m = matrices(10.0 + k)
            t0 = time.perf_counter(); r.skin_mesh(0, m); r.synchronize(); t_skin.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); r.refit_mesh(0, posed[k & 1]); r.synchronize(); t_refit.append(time.perf_counter() - t0)
        r.set_tuning(skin_joints_lds=0)
        r.skin_mesh(0, matrices(2.0))
        for k in range(reps):
            m = matrices(10.0 + k)
            t0 = time.perf_counter(); r.skin_mesh(0, m); r.synchronize(); t_vc.append(time.perf_counter() - t0)
        r.set_tuning(skin_joints_lds=1)
        res = {"triangles": int(tris.shape[0]), "skin_mesh_lds": _stats(t_skin), "skin_mesh_vector_cache": _stats(t_vc), "refit_mesh": _stats(t_refit),
               "host_skin_triangles": _stats(t_host)}
        print(f"{n_joints} joints{' (random per corner)' if args.random_joints else ''}, {tris.shape[0]} triangles")
        for name in ("skin_mesh_lds", "skin_mesh_vector_cache", "refit_mesh", "host_skin_triangles"):
            print("  " + _fmt(name, res[name]), flush=True)
        a, b = res["skin_mesh_lds"], res["refit_mesh"]
        margin = b["median_ms"] - a["median_ms"]
        res["faster_by_ms"] = margin; res["combined_spread_ms"] = a["spread_ms"] + b["spread_ms"]
        res["accepted"] = bool(margin > res["combined_spread_ms"])
        print(f"  skin_mesh is faster than refit_mesh by {margin:.3f} ms ({b['median_ms'] / a['median_ms']:.1f}x); the two spreads together are "
              f"{res['combined_spread_ms']:.3f} ms: {'ACCEPTED' if res['accepted'] else 'NOT ACCEPTED'}", flush=True)
        out[str(n_joints)] = res
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)
    if not all(v["accepted"] for v in out.values()):
        sys.exit(1)


def trace(args):
    import cpugpupathtracing_amd as P
    n_joints = args.joints[0]
    r, s, tris, j, w, matrices = _setup(args.level, n_joints, args.random_joints)
    posed = P.skin_triangles(tris, j, w, matrices(5.0))
    r.skin_mesh(0, matrices(1.0)); r.refit_mesh(0, posed)
    for lds in (1, 0):
        r.set_tuning(skin_joints_lds=lds)
        for k in range(args.calls):
            r.skin_mesh(0, matrices(10.0 + k))
    for k in range(args.calls):
        r.refit_mesh(0, posed)
    r.synchronize()
    print(f"{n_joints} joints: {args.calls + 1} poses with the matrices in LDS, {args.calls} through the vector cache, {args.calls + 1} refits")
    r.close(); s.close()


def summary(args):
    """Per kernel of the refit unit, from the result databases rocprofv3 wrote around `trace` (no GPU needed): launches and
    median / min / max in microseconds, the first (cold) launch of a triangle pass left out, and the level launches behind each triangle
    pass summed per call."""
    import sqlite3
    import statistics
    keys = ("skin_triangles<true>", "skin_triangles<false>", "refit_triangles", "refit_level", "fold_object_box")
    for path in args.db:
        db = sqlite3.connect(path)
        rows = db.execute("select name, duration, lds_size, scratch_size, grid_x, workgroup_x from kernels order by start").fetchall()
        print(f"--- {path}")
        by, order = {}, []
        for name, dur, lds, scratch, grid, block in rows:
            key = next((k for k in keys if k in name), None)
            if key is None:
                continue
            by.setdefault(key, []).append((dur / 1e3, lds, scratch, grid, block))
            order.append((key, dur / 1e3))
        for key, v in by.items():
            d = [x[0] for x in v]
            d = d[1:] if "triangles" in key else d
            print(f"{key:24s} launches {len(v):4d}  median {statistics.median(d):8.2f}  min {min(d):8.2f}  max {max(d):8.2f} us   "
                  f"LDS {v[-1][1]} B, scratch {v[-1][2]}, grid {v[-1][3]} threads in blocks of {v[-1][4]}")
        sums, cur = {}, None
        for key, d in order:
            if "triangles" in key:
                cur = key
                sums.setdefault(cur, []).append(0.0)
            elif key == "refit_level" and cur:
                sums[cur][-1] += d
        for key, s in sums.items():
            s = s[1:]
            print(f"refit_level summed over the launches behind {key}: median {statistics.median(s):.1f} us (min {min(s):.1f}, max {max(s):.1f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("pose"); a.add_argument("--reps", type=int, default=20); a.add_argument("--joints", type=int, nargs="+", default=[2])
    a.add_argument("--level", type=int, default=8); a.add_argument("--out"); a.add_argument("--random-joints", action="store_true")
    b = sub.add_parser("trace"); b.add_argument("--joints", type=int, nargs=1, default=[2]); b.add_argument("--calls", type=int, default=20)
    b.add_argument("--level", type=int, default=8); b.add_argument("--random-joints", action="store_true")
    c = sub.add_parser("ab"); c.add_argument("--parent-tree", required=True); c.add_argument("--pairs", type=int, default=3)
    c.add_argument("--steps", type=int, default=5); c.add_argument("--warmup", type=int, default=2); c.add_argument("--out")
    d = sub.add_parser("summary"); d.add_argument("db", nargs="+")
    args = ap.parse_args()
    if args.cmd == "ab":
        from gpu_transform_time import ab
        ab(args)
    else:
        {"pose": pose, "trace": trace, "summary": summary}[args.cmd](args)
