#!/usr/bin/env python3
"""On the GPU box: what the top-level tree (cgpt_set_top_level) costs and pays.

  ab      the default bench (bench.py --gpus 1) of this tree and of a built checkout of the parent commit, alternating A B A B in child
          processes: with the mode at its default 0 every render runs the kernels it ran before, so the two should differ by no more
          than each one's own run-to-run spread.  Both spreads are printed.
  forest  N placed instances of one small mesh (a level-1 icosphere, 80 triangles, each under its own rotation, scale and shift) over a
          ground quad with two sphere lights, N in 8, 32, 128, 512, the instances in Morton order (Scene.sort_objects_spatially) and in
          a shuffled order, at 1920x1080, ADVANCED: list walk (mode 0) against tree (mode 1) on the same renderer, alternating, for each
          of the three kernels: ms per render (cgpt_stats.kernel_ms, median of the repeats) and the smallest N at which the tree wins.

usage: python scripts/gpu_tlas_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2]
       python scripts/gpu_tlas_time.py forest [--reps 3] [--counts 8,32,128,512] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SPP = {"megakernel": 4, "persistent": 16, "wavefront": 16}        # a list walk over 512 instances is long: short renders


def ab(args):
    trees = {"this": REPO, "parent": os.path.abspath(args.parent_tree)}
    assert os.path.exists(os.path.join(trees["parent"], "bench.py")), trees["parent"]
    values = {"this": [], "parent": []}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            p = subprocess.run([sys.executable, os.path.join(trees[name], "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--cpu-seconds", "0", "--no-roofline-pass"], cwd=trees[name], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                              # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            res = json.loads(line)
            values[name].append(res)
            print(f"{name:7s} run {pair}: " + " ".join(f"{k}={res[k]}" for k in ("value", "unit", "ms_per_step") if k in res), flush=True)
    for name, v in values.items():
        xs = [r["value"] for r in v]
        print(f"{name:7s} value mean {sum(xs) / len(xs):.6g} min {min(xs):.6g} max {max(xs):.6g} spread {(max(xs) - min(xs)) / min(xs) * 100:.2f} %")
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


def _icosphere(level):
    """(vertices (n, 6), indices): the unit icosphere, subdivided `level` times, vertex normals = positions."""
    import numpy as np
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []
        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]; v.append(p / np.linalg.norm(p)); mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab_, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab_, ca), (b, bc, ab_), (c, ca, bc), (ab_, bc, ca)]
        f = nf
    p = np.array(v, np.float32)
    return np.concatenate([p, p], 1), np.array(f, np.uint32).ravel()


def _forest(n, order, seed=1):
    """ground quad, two sphere lights, n instances of the level-1 icosphere on a jittered square grid, each under its own transform."""
    import numpy as np
    import cpugpupathtracing_amd as P
    rng = np.random.default_rng(seed)
    s = P.Scene()
    ground = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.85), intensity=30.0, is_light=True))
    leaf = s.add_material(P.Material(albedo=(0.3, 0.7, 0.35)))
    side = int(np.ceil(n ** 0.5))
    half = 1.6 * side
    gv = np.array([[-half, 0, -half, 0, 1, 0], [half, 0, -half, 0, 1, 0], [half, 0, half, 0, 1, 0], [-half, 0, half, 0, 1, 0]], np.float32)
    s.add_mesh(P.Mesh.from_arrays(gv, np.array([0, 2, 1, 0, 3, 2], np.uint32)), ground)
    for c in ((-0.5 * half, 1.5 * half, 0.5 * half), (0.6 * half, 1.2 * half, -0.3 * half)):
        s.add_light(s.add_sphere(c, 0.15 * half, emitter))
    mesh = P.Mesh.from_arrays(*_icosphere(1))
    cells = [(x, z) for x in range(side) for z in range(side)][:n]
    rng.shuffle(cells)
    for x, z in cells:
        axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
        a = rng.uniform(0.0, 3.0)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        A = (np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)) @ np.diag(rng.uniform(0.7, 1.3, 3))
        b = np.array([3.2 * (x - 0.5 * (side - 1)) + rng.uniform(-0.4, 0.4), rng.uniform(1.3, 2.5), 3.2 * (z - 0.5 * (side - 1)) + rng.uniform(-0.4, 0.4)])
        s.add_mesh(mesh, leaf, transform=np.concatenate([A, b[:, None]], 1).astype(np.float32))
    s.set_camera((0.0, 1.1 * half, 2.2 * half), (0.0, -0.45, -1.0), 50.0, W / H)
    if order == "morton":
        s.sort_objects_spatially()
    return s


def forest(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    kernels = {"megakernel": P.KERNEL_MEGAKERNEL, "persistent": P.KERNEL_PERSISTENT, "wavefront": P.KERNEL_WAVEFRONT}
    out = {}
    for n in [int(x) for x in args.counts.split(",")]:
        for order in ("morton", "shuffled"):
            s = _forest(n, order)
            r = P.Renderer(0)
            r.upload(s)
            for kname, kernel in kernels.items():
                ms = {0: [], 1: []}
                for mode in (0, 1):                                # warm-up of both walks
                    r.set_top_level(bool(mode)); r.reset_accumulator(); r.render(W, H, SPP[kname], seed=1, kernel=kernel, settings=st)
                for i in range(args.reps):
                    for mode in (0, 1):
                        r.set_top_level(bool(mode)); r.reset_accumulator(); r.reset_stats()
                        r.render(W, H, SPP[kname], seed=100 + i, kernel=kernel, settings=st)
                        ms[mode].append(r.stats().kernel_ms)
                a, b = float(np.median(ms[0])), float(np.median(ms[1]))
                out[f"{n}/{order}/{kname}"] = {"list_ms": a, "tree_ms": b, "runs": ms}
                print(f"N {n:4d} {order:8s} {kname:10s} {SPP[kname]:3d} spp: list {a:9.2f} ms  tree {b:9.2f} ms  ({(b / a - 1.0) * 100:+.1f} %)", flush=True)
            r.close(); s.close()
    for order in ("morton", "shuffled"):
        for kname in kernels:
            wins = [int(k.split("/")[0]) for k, v in out.items() if k.endswith(f"/{order}/{kname}") and v["tree_ms"] < v["list_ms"]]
            print(f"{order:8s} {kname:10s}: the tree wins from N = {min(wins) if wins else 'never (of those measured)'}")
    if args.out:
        json.dump({"width": W, "height": H, "spp": SPP, "rows": out}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("ab"); a.add_argument("--parent-tree", required=True); a.add_argument("--pairs", type=int, default=3)
    a.add_argument("--steps", type=int, default=5); a.add_argument("--warmup", type=int, default=2); a.add_argument("--out")
    b = sub.add_parser("forest"); b.add_argument("--reps", type=int, default=3); b.add_argument("--counts", default="8,32,128,512"); b.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    {"ab": ab, "forest": forest}[args.cmd](args)
