#!/usr/bin/env python3
"""On the GPU box: what blending clips on the device (cgpt_scene_animate_layers) costs against the host loop it
replaces and against the one-clip call, on the same build and context.

  crowd      N separate stand-in meshes in a row (scripts/gpu_animate_time.py's crowd: --level 3 is 1280 triangles, --joints joints a
             character) and four clips shared by all.  Every character blends two layers (LOOP, PINGPONG) or four (all modes) at its own
             times.  One side is one animate_layers call; the other evaluates the mirror on the host (P.animate_layers, once per
             character) and gives the matrices to one pose_objects call; the third is one animate_objects call of one clip.  Each ends
             with a synchronise; they alternate in one process; warm calls only; the median of --reps (>= 20) with min / max.  Reported
             apart: the host evaluation, and what the Python binding spends on the entry tables of an animate_layers call.
  animate    one animate_objects call of the 256-character crowd, warm median, one RESULT line; --tree PATH imports the package of
             another built checkout (the parent commit's)
  ab-animate `animate` of this tree against --parent-tree, --pairs alternating pairs of processes
  ab         the default bench of this tree against a built checkout of the parent commit, three alternating pairs
             (scripts/gpu_transform_time.py: ab).

usage: python scripts/gpu_blend_time.py crowd [--reps 20] [--counts 1 16 64 256] [--joints 64] [--level 3] [--out FILE.json]
       python scripts/gpu_blend_time.py animate [--reps 20] [--count 256] [--joints 64] [--tree PATH]
       python scripts/gpu_blend_time.py ab-animate --parent-tree PATH [--pairs 3] [--reps 20] [--out FILE.json]
       python scripts/gpu_blend_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2] [--out FILE.json]"""
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

from gpu_animate_time import _crowd, _quat_x
from gpu_skin_time import _fmt, _stats


def _variant(clip, n_joints, k):
    """clip k of the four: the crowd's clip with its rotation keys scaled and its key times stretched, so the ranges differ"""
    import numpy as np
    n, channels, times, values = clip
    values = values.copy()
    for path, first_value in zip(channels[:, 1], channels[:, 5]):
        if path == 1:                                          # a rotation channel: three keys
            values[first_value:first_value + 12] = np.float32(_quat_x(0.0) + _quat_x((20.0 + 7.0 * k) / n_joints) + _quat_x((-10.0 - 5.0 * k) / n_joints))
    return n, channels, (times * np.float32(1.0 + 0.25 * k)).astype(np.float32), values


def crowd(args):
    import cpugpupathtracing_amd as P
    from cpugpupathtracing_amd import _native as N
    from cpugpupathtracing_amd.renderer import _layer_tables
    reps, warm = max(args.reps, 20), 3
    modes = (N.ANIM_WRAP_LOOP, N.ANIM_WRAP_PINGPONG, N.ANIM_WRAP_CLAMP, N.ANIM_WRAP_LOOP)
    weights = (1.0, 0.5, 0.25, 2.0)
    out = {}
    for count in args.counts:
        r, s, skeleton, clip, handle = _crowd(args.level, count, args.joints)
        clips = [clip] + [_variant(clip, args.joints, k) for k in (1, 2, 3)]
        handles = [handle] + [r.create_clip(*c) for c in clips[1:]]
        ts = {k: [] for k in ("layers2", "tables2", "host2", "host2_eval", "layers4", "tables4", "host4", "host4_eval", "objects")}
        for k in range(warm + reps):
            when = [0.01 * k + 2.9 * c / count for c in range(count)]
            for depth in (2, 4):
                spec = [[(l, t + 0.37 * l, weights[l], modes[l]) for l in range(depth)] for t in when]
                t0 = time.perf_counter()
                r.animate_layers([(c, [(handles[l], t, w, m) for l, t, w, m in layers], None) for c, layers in enumerate(spec)]); r.synchronize()
                ta = time.perf_counter() - t0
                t0 = time.perf_counter()                               # the same entries once more as far as the C call: the binding's share
                _layer_tables([(c, [(handles[l], t, w, m) for l, t, w, m in layers], None) for c, layers in enumerate(spec)])
                tb = time.perf_counter() - t0
                spec = [[(l, t + 0.005, w, m) for l, t, w, m in layers] for layers in spec]
                t0 = time.perf_counter()
                ms = [P.animate_layers(skeleton, [(clips[l], t, w, m) for l, t, w, m in layers]) for layers in spec]
                t1 = time.perf_counter()
                r.pose_objects([(c, m, None) for c, m in enumerate(ms)]); r.synchronize()
                t2 = time.perf_counter()
                if k >= warm:
                    ts[f"layers{depth}"].append(ta); ts[f"tables{depth}"].append(tb); ts[f"host{depth}"].append(t2 - t0); ts[f"host{depth}_eval"].append(t1 - t0)
            t0 = time.perf_counter(); r.animate_objects([(c, handle, t % 1.0, None) for c, t in enumerate(when)]); r.synchronize(); to = time.perf_counter() - t0
            if k >= warm:
                ts["objects"].append(to)
        st = {k: _stats(v) for k, v in ts.items()}
        name = f"{count} characters x {args.joints} joints, {20 * 4 ** args.level} triangles each"
        print(name)
        for depth in (2, 4):
            print("  " + _fmt(f"one animate_layers call, {depth} layers a character", st[f"layers{depth}"]))
            print("  " + _fmt("  of which the Python binding's entry tables (timed apart)", st[f"tables{depth}"]))
            print("  " + _fmt(f"mirror on the host ({depth} layers) + one pose_objects call", st[f"host{depth}"]))
            print("  " + _fmt("  of which the host evaluation", st[f"host{depth}_eval"]))
        print("  " + _fmt("one animate_objects call, one clip a character", st["objects"]))
        for depth in (2, 4):
            a = st[f"layers{depth}"]["median_ms"]
            print(f"  {depth} layers: animate_layers takes {a / st[f'host{depth}']['median_ms']:.3f} of the host side's time and "
                  f"{a - st['objects']['median_ms']:+.3f} ms against animate_objects", flush=True)
        out[name] = st
        r.close(); s.close()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


def animate(args):
    """animate_objects alone, by the calls both trees have"""
    r, s, skeleton, clip, handle = _crowd(args.level, args.count, args.joints)
    ts = []
    for k in range(3 + max(args.reps, 20)):
        entries = [(c, handle, (0.01 * k + 0.9 * c / args.count) % 1.0, None) for c in range(args.count)]
        t0 = time.perf_counter(); r.animate_objects(entries); r.synchronize(); t = time.perf_counter() - t0
        if k >= 3:
            ts.append(t)
    r.close(); s.close()
    print("RESULT " + json.dumps({"animate_objects": _stats(ts)["median_ms"]}), flush=True)


def ab_animate(args):
    trees = {"this": os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parent": os.path.abspath(args.parent_tree)}
    values = {"this": [], "parent": []}
    for pair in range(args.pairs):
        for name in ("this", "parent"):                                # the same script drives both trees: it uses only calls the parent has
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "animate", "--reps", str(args.reps), "--tree", trees[name]], cwd=trees[name],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                                      # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            v = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])["animate_objects"]
            values[name].append(v)
            print(f"{name:7s} run {pair}: animate_objects of 256 characters {v:.3f} ms", flush=True)
    for name, xs in values.items():
        print(f"{name:7s} animate_objects: mean {sum(xs) / len(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f}, spread {(max(xs) - min(xs)) / min(xs) * 100:.2f} %)")
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("crowd"); a.add_argument("--counts", type=int, nargs="+", default=[1, 16, 64, 256])
    e = sub.add_parser("animate"); e.add_argument("--tree"); e.add_argument("--count", type=int, default=256)
    f = sub.add_parser("ab-animate"); f.add_argument("--parent-tree", required=True); f.add_argument("--pairs", type=int, default=3)
    g = sub.add_parser("ab"); g.add_argument("--parent-tree", required=True); g.add_argument("--pairs", type=int, default=3)
    g.add_argument("--steps", type=int, default=5); g.add_argument("--warmup", type=int, default=2)
    for p in (a, e, f):
        p.add_argument("--reps", type=int, default=20)
    for p in (a, e):
        p.add_argument("--joints", type=int, default=64); p.add_argument("--level", type=int, default=3)
    for p in (a, f, g):
        p.add_argument("--out")
    args = ap.parse_args()
    if args.cmd == "ab":
        from gpu_transform_time import ab
        ab(args)
    else:
        {"crowd": crowd, "animate": animate, "ab-animate": ab_animate}[args.cmd](args)
