#!/usr/bin/env python3
"""On the GPU box: what playing an animation clip on the device (cgpt_scene_animate_objects) costs against the host
loop it replaces, on the same build and context.

  crowd   N separate stand-in meshes in a row (--level: 3 is 1280 triangles), each skinned to --joints joints (a chain, blended by
          height) with a skeleton; one clip with a rotation and a translation channel on every joint, shared by all, each character at
          its own time.  One side is one animate_objects call; the other evaluates the mirror on the host (P.animate_joints, once per
          character) and gives the matrices to one pose_objects call.  Each side ends with a synchronise; the two alternate in one
          process; warm calls only; the median of --reps (>= 20) with min / max.  Reported apart: the host evaluation; the upload (a
          host-to-device copy of the N x joints x 48 bytes alone, timed by itself); pose_objects with matrices that already exist
          (the batch alone); and animate_objects minus that batch: the kernel, its readback and the one extra synchronise.
  trace   --calls animate_objects calls of one crowd and nothing else, for a kernel trace around it:
          rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_animate_time.py trace --count 256
  summary the time of animate_joints_batch per call out of the kernel trace that run wrote (no GPU needed):
          python scripts/gpu_animate_time.py summary KERNEL_TRACE.csv
  pose    one pose_objects call of the 256-character crowd, warm median, one RESULT line; --tree PATH imports the package of another
          built checkout (the parent commit's)
  ab-pose `pose` of this tree against --parent-tree, --pairs alternating pairs of processes
  ab      the default bench of this tree against a built checkout of the parent commit, three alternating pairs
          (scripts/gpu_transform_time.py: ab).

usage: python scripts/gpu_animate_time.py crowd [--reps 20] [--counts 1 16 64 256] [--joints 64] [--level 3] [--out FILE.json]
       python scripts/gpu_animate_time.py trace [--count 256] [--joints 64] [--level 3] [--calls 12]
       python scripts/gpu_animate_time.py summary KERNEL_TRACE.csv
       python scripts/gpu_animate_time.py pose [--reps 20] [--count 256] [--tree PATH]
       python scripts/gpu_animate_time.py ab-pose --parent-tree PATH [--pairs 3] [--reps 20] [--out FILE.json]
       python scripts/gpu_animate_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2] [--out FILE.json]"""
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

from gpu_skin_time import _fmt, _stats


def _quat_x(deg):
    import numpy as np
    h = np.deg2rad(deg) / 2
    return [np.sin(h), 0.0, 0.0, np.cos(h)]


def _crowd(level, count, n_joints, rigged=True):
    """(renderer, scene, skeleton, clip data, clip handle): `count` copies of the stand-in side by side, each skinned to a chain of
    n_joints joints up its height (two neighbouring joints per corner), with the skeleton installed and one clip created"""
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
    lo, hi = y.min(), y.max()
    x = (y - lo) / (hi - lo) * max(n_joints - 1, 1)
    j0 = np.minimum(np.floor(x), max(n_joints - 2, 0)).astype(np.int64)
    t = (x - j0).astype(np.float32) if n_joints > 1 else np.zeros(y.shape, np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); w = np.zeros(y.shape + (4,), np.float32)
    j[..., 0] = j0; j[..., 1] = np.minimum(j0 + 1, n_joints - 1)
    w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    for k in range(count):
        r.set_skin(k, binds[k], j, w, n_joints)
    # the chain: joint i sits (hi - lo) / n_joints above joint i - 1; the inverse bind matrices undo the rest pose's translations
    step = (hi - lo) / n_joints
    parents = np.arange(-1, n_joints - 1).astype(np.int32)
    rest = np.tile(np.float32([0, step, 0, 0, 0, 0, 1, 1, 1, 1]), (n_joints, 1)); rest[0, 1] = lo
    ib = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (n_joints, 1))
    ib[:, 7] = -(lo + step * np.arange(n_joints))
    skeleton = (parents, ib, rest, None)
    channels, times, values = [], [], []
    for i in range(n_joints):                                  # a rotation (3 keys, LINEAR) and a translation (2 keys) on every joint
        channels.append((i, 1, 1, 3, len(times), len(values))); times += [0.0, 0.5, 1.0]; values += _quat_x(0.0) + _quat_x(20.0 / n_joints) + _quat_x(-10.0 / n_joints)
        channels.append((i, 0, 1, 2, len(times), len(values))); times += [0.0, 1.0]; values += [0.0, float(rest[i, 1]), 0.0, 0.0, float(rest[i, 1]) * 1.05, 0.0]
    clip = (n_joints, np.asarray(channels, np.uint32), np.asarray(times, np.float32), np.asarray(values, np.float32))
    handle = None
    if rigged:
        for k in range(count):
            r.set_skeleton(k, *skeleton)
        handle = r.create_clip(*clip)
    return r, s, skeleton, clip, handle


def _mirror(P, skeleton, clip, times):
    return [P.animate_joints(skeleton, clip, t) for t in times]


def crowd(args):
    import numpy as np
    import torch
    import cpugpupathtracing_amd as P
    reps, warm = max(args.reps, 20), 3
    out = {}
    for count in args.counts:
        r, s, skeleton, clip, handle = _crowd(args.level, count, args.joints)
        t_anim, t_host_side, t_eval, t_batch, t_upload = [], [], [], [], []
        staging = np.zeros((count, args.joints, 12), np.float32)
        for k in range(warm + reps):
            when = [0.01 * k + 0.9 * c / count for c in range(count)]
            t0 = time.perf_counter(); r.animate_objects([(c, handle, t, None) for c, t in enumerate(when)]); r.synchronize(); ta = time.perf_counter() - t0
            when = [t + 0.005 for t in when]
            t0 = time.perf_counter()
            ms = _mirror(P, skeleton, clip, when)
            t1 = time.perf_counter()
            r.pose_objects([(c, m, None) for c, m in enumerate(ms)]); r.synchronize()
            t2 = time.perf_counter()
            staging[:] = np.stack(ms)                          # the same bytes by themselves: one host-to-device copy, synchronised
            t3 = time.perf_counter(); d = torch.from_numpy(staging).to("cuda:0"); torch.cuda.synchronize(); t4 = time.perf_counter()
            del d
            if k >= warm:
                t_anim.append(ta); t_host_side.append(t2 - t0); t_eval.append(t1 - t0); t_batch.append(t2 - t1); t_upload.append(t4 - t3)
        st = {"animate_objects": _stats(t_anim), "host_evaluation_and_pose_objects": _stats(t_host_side), "host_evaluation": _stats(t_eval),
              "pose_objects_alone": _stats(t_batch), "upload_alone": _stats(t_upload)}
        name = f"{count} characters x {args.joints} joints ({count * args.joints * 48} bytes of matrices), {20 * 4 ** args.level} triangles each"
        print(name)
        print("  " + _fmt("one animate_objects call", st["animate_objects"]))
        print("  " + _fmt("mirror on the host + one pose_objects call", st["host_evaluation_and_pose_objects"]))
        print("  " + _fmt("  of which the host evaluation", st["host_evaluation"]))
        print("  " + _fmt("  of which pose_objects (matrices given)", st["pose_objects_alone"]))
        print("  " + _fmt("the matrices' upload by itself", st["upload_alone"]))
        extra = st["animate_objects"]["median_ms"] - st["pose_objects_alone"]["median_ms"]
        print(f"  animate_objects - pose_objects: {extra:.3f} ms (the kernel, the readback of the matrices and the one extra synchronise); "
              f"animate_objects takes {st['animate_objects']['median_ms'] / st['host_evaluation_and_pose_objects']['median_ms']:.3f} of the host side's time", flush=True)
        st["extra_ms"] = extra
        out[name] = st
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def trace(args):
    r, s, skeleton, clip, handle = _crowd(args.level, args.count, args.joints)
    r.synchronize()
    for k in range(args.calls):
        r.animate_objects([(c, handle, 0.05 * k + 0.9 * c / args.count, None) for c in range(args.count)])
    r.synchronize()
    print(f"{args.calls} animate_objects calls of {args.count} characters x {args.joints} joints")
    r.close(); s.close()


def summary(args):
    import csv
    with open(args.db[0], newline="") as f:
        rows = [(row["Kernel_Name"], int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) for row in csv.DictReader(f)]
    ours = sorted(d for name, d in rows if "animate_joints_batch" in name)
    if not ours:
        sys.exit("no animate_joints_batch launch in the trace")
    print(f"animate_joints_batch: {len(ours)} launches, median {ours[len(ours) // 2] / 1e3:.1f} us (min {ours[0] / 1e3:.1f}, max {ours[-1] / 1e3:.1f})")
    total = {}
    for name, d in rows:
        key = name.split("(")[0][-60:]
        c, t = total.get(key, (0, 0)); total[key] = (c + 1, t + d)
    for key, (c, t) in sorted(total.items(), key=lambda kv: -kv[1][1]):
        print(f"  {key:60s} {c:6d} launches {t / 1e3:10.1f} us")


def pose(args):
    """pose_objects alone, by the calls both trees have: two joints a character, the matrices computed outside the timed span"""
    import numpy as np
    import cpugpupathtracing_amd as P
    r, s, skeleton, clip, handle = _crowd(args.level, args.count, 2, rigged=False)
    ts = []
    ident = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    for k in range(3 + max(args.reps, 20)):
        m = np.stack([ident, ident]); m[1, 3] = np.float32(0.001 * k)
        entries = [(c, m, None) for c in range(args.count)]
        t0 = time.perf_counter(); r.pose_objects(entries); r.synchronize(); t = time.perf_counter() - t0
        if k >= 3:
            ts.append(t)
    r.close(); s.close()
    print("RESULT " + json.dumps({"pose_objects": _stats(ts)["median_ms"]}), flush=True)


def ab_pose(args):
    trees = {"this": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parent": os.path.abspath(args.parent_tree)}
    values = {"this": [], "parent": []}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "pose", "--reps", str(args.reps), "--tree", trees[name]], cwd=trees[name],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                              # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            v = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])["pose_objects"]
            values[name].append(v)
            print(f"{name:7s} run {pair}: pose_objects of 256 characters {v:.3f} ms", flush=True)
    for name, xs in values.items():
        print(f"{name:7s} pose_objects: mean {sum(xs) / len(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})")
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("crowd"); a.add_argument("--counts", type=int, nargs="+", default=[1, 16, 64, 256])
    c = sub.add_parser("trace"); c.add_argument("--calls", type=int, default=12)
    d = sub.add_parser("summary"); d.add_argument("db", nargs=1)
    e = sub.add_parser("pose"); e.add_argument("--tree")
    f = sub.add_parser("ab-pose"); f.add_argument("--parent-tree", required=True); f.add_argument("--pairs", type=int, default=3)
    g = sub.add_parser("ab"); g.add_argument("--parent-tree", required=True); g.add_argument("--pairs", type=int, default=3)
    g.add_argument("--steps", type=int, default=5); g.add_argument("--warmup", type=int, default=2)
    for p in (a, e, f):
        p.add_argument("--reps", type=int, default=20)
    for p in (a, c):
        p.add_argument("--joints", type=int, default=64)
    for p in (a, c, e):
        p.add_argument("--level", type=int, default=3)
    for p in (c, e):
        p.add_argument("--count", type=int, default=256)
    for p in (a, f, g):
        p.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "ab":
        from gpu_transform_time import ab
        ab(args)
    else:
        {"crowd": crowd, "trace": trace, "summary": summary, "pose": pose, "ab-pose": ab_pose}[args.cmd](args)
