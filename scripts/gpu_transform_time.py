#!/usr/bin/env python3
"""On the GPU box: what per-object transforms (cgpt_scene_update_transforms) cost.

  ab      the default bench (bench.py --gpus 1) of this tree and of a built checkout of the parent commit, alternating A B A B in child
          processes: a scene without a transform runs the parent's instantiations, so the two should differ by no more than each one's
          own run-to-run spread.  Both spreads are printed.
  stored  the reference layout around the dragon stand-in (level 6, glass) at 1920x1080, ADVANCED, with the stand-in baked into the world
          (no transform: lobe level 0) and stored in a rotated, scaled frame and brought back by its transform (lobe level 4), alternating,
          for each of the three kernels: ms per render (cgpt_stats.kernel_ms, median of the repeats); for the wavefront pipeline also the
          trace launches' summed time (the pools run concurrently, so the sum exceeds the render's) and round 0's share of it.
  render  one warm-up and one render of that scene with one pool, baked or stored, for a kernel trace around it
          (rocprofv3 --kernel-trace --stats -- python scripts/gpu_transform_time.py render --stored 1): every kernel's own time.
  move    one rigid move of the 1.31 M-triangle mesh (bench.py's big scene: the bumpy icosphere, level 8) by cgpt_scene_update_transforms
          against the same move by cgpt_scene_refit_mesh of every triangle: ms per call (median), host time included.

usage: python scripts/gpu_transform_time.py ab --parent-tree PATH [--pairs 3] [--steps 5] [--warmup 2]
       python scripts/gpu_transform_time.py stored [--reps 3] [--out FILE.json]
       python scripts/gpu_transform_time.py render --stored 1
       python scripts/gpu_transform_time.py move [--reps 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
SPP = {"megakernel": 32, "persistent": 256, "wavefront": 256}     # the megakernel walks a pixel's samples in one thread: a shorter render


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


def _frame():
    """The object-to-world matrix of the stored frame: a rotation by 0.7 rad about (1, 2, 3), a uniform scale of 1.5, a shift."""
    import numpy as np
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    A = (np.eye(3) + np.sin(0.7) * K + (1.0 - np.cos(0.7)) * (K @ K)) * 1.5
    return np.concatenate([A, np.array([[0.5], [-0.25], [1.0]])], 1).astype(np.float32)


def _scenes(level=6):
    """(baked scene, stored scene, the stored scene's matrices): the reference layout around the dragon stand-in; stored: its vertices
    A^-1 (p - b) and normals A^T n, formed in float64, brought back by [A | b]."""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    baked = P.Scene.reference_layout(mesh, 3, W / H)
    m = _frame().astype(np.float64)
    v = np.array(mesh.vertices, np.float32, copy=True)
    v[:, 0:3] = ((mesh.vertices[:, 0:3].astype(np.float64) - m[:, 3]) @ np.linalg.inv(m[:, :3]).T).astype(np.float32)
    v[:, 3:6] = (mesh.vertices[:, 3:6].astype(np.float64) @ m[:, :3]).astype(np.float32)
    stored = P.Scene.reference_layout(P.Mesh.from_arrays(v, mesh.indices), 3, W / H)
    stored.set_transform(0, _frame())                          # object 0 of the layout: the stand-in
    return baked, stored


def stored(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    scenes = dict(zip(("baked", "stored"), _scenes()))
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    kernels = {"megakernel": P.KERNEL_MEGAKERNEL, "persistent": P.KERNEL_PERSISTENT, "wavefront": P.KERNEL_WAVEFRONT}
    rs = {}
    for name, s in scenes.items():
        rs[name] = P.Renderer(0)
        rs[name].upload(s)                                     # sends the scene's transform
    out = {}
    for kname, kernel in kernels.items():
        rows = {"baked": [], "stored": []}
        for name, r in rs.items():                             # warm-up of both lobe levels
            r.reset_accumulator(); r.render(W, H, SPP[kname], seed=1, kernel=kernel, settings=st)
        for i in range(args.reps):
            for name, r in rs.items():
                r.reset_accumulator(); r.reset_stats()
                r.render(W, H, SPP[kname], seed=1000 + i, kernel=kernel, settings=st)
                x = r.stats()
                rows[name].append({"ms": x.kernel_ms, "trace_ms": x.dominant_ms, "round0_ms": x.dominant_round0_ms, "traced_rays": int(x.traced_rays),
                                   "waves_per_simd": int(x.dominant_waves_per_simd), "probe_resolved": int(x.probe_resolved)})
                print(f"{kname:10s} {name:6s} rep {i}: {x.kernel_ms:8.2f} ms  trace {x.dominant_ms:8.2f} ms (round 0 {x.dominant_round0_ms:6.2f})  "
                      f"{x.traced_rays} rays  {x.dominant_waves_per_simd} waves/SIMD  probe resolved {x.probe_resolved}", flush=True)
        med = {n: {k: float(np.median([x[k] for x in rows[n]])) for k in ("ms", "trace_ms", "round0_ms")} for n in rows}
        b, t = med["baked"], med["stored"]
        print(f"{kname}: {W}x{H}, {SPP[kname]} spp, ADVANCED: baked {b['ms']:.2f} ms, stored {t['ms']:.2f} ms ({(t['ms'] / b['ms'] - 1.0) * 100:+.2f} %)")
        if kname == "wavefront":
            print(f"  wf_trace, summed over the pools' concurrent launches: {b['trace_ms']:.2f} -> {t['trace_ms']:.2f} ms (round 0 {b['round0_ms']:.2f} -> {t['round0_ms']:.2f}); "
                  f"the other kernels' own times: rocprofv3 --kernel-trace --stats around the `render` command")
        out[kname] = {"runs": rows, "median": med}
    if args.out:
        json.dump({"width": W, "height": H, "spp": SPP, "kernels": out}, open(args.out, "w"), indent=1)
    for r in rs.values():
        r.close()


def render(args):
    import cpugpupathtracing_amd as P
    s = _scenes()[1 if args.stored else 0]
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    r.upload(s)
    r.set_tuning(pools=1)
    for seed in (1, 2):
        r.reset_accumulator(); r.reset_stats()
        r.render(W, H, SPP["wavefront"], seed=seed, kernel=P.KERNEL_WAVEFRONT, settings=st)
    print(f"stored {args.stored}: {r.stats().kernel_ms:.2f} ms with one pool")
    r.close()


def move(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    from cpugpupathtracing_amd.scene import triangles_from_arrays
    mesh = P.Mesh.bumpy_icosphere(8, (0.0, 6.0, -30.0), (24.0, 10.0, 16.0), 0.15)
    s = P.Scene.reference_layout(mesh, 3, W / H)
    n = s.flatten().n_objects
    r = P.Renderer(0)
    r.upload(s)
    shift = np.array([0.25, 0.0, -0.5], np.float32)
    matrices = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))
    t_x, t_r = [], []
    for i in range(args.reps + 1):
        matrices[0, 3::4] = shift * (i + 1)
        t0 = time.perf_counter()
        r.update_transforms(matrices)
        r.synchronize()
        t_x.append(time.perf_counter() - t0)
    matrices[0, 3::4] = 0.0
    r.update_transforms(matrices)
    v = np.array(mesh.vertices, np.float32, copy=True)
    for i in range(args.reps + 1):
        v[:, 0:3] = mesh.vertices[:, 0:3] + shift * (i + 1)
        t0 = time.perf_counter()
        rows = triangles_from_arrays(v, mesh.indices)          # the host's share of a move by refit: every triangle anew
        t1 = time.perf_counter()
        r.refit_mesh(0, rows)
        r.synchronize()
        t_r.append((time.perf_counter() - t0, time.perf_counter() - t1))
    print(f"{rows.shape[0]} triangles: one rigid move by cgpt_scene_update_transforms {np.median(t_x[1:]) * 1e3:.3f} ms "
          f"(min {min(t_x[1:]) * 1e3:.3f}, max {max(t_x[1:]) * 1e3:.3f}; {n} objects, {n * 80} bytes written); "
          f"by cgpt_scene_refit_mesh {np.median([a for a, _ in t_r[1:]]) * 1e3:.1f} ms with the host's triangle rows, "
          f"{np.median([b for _, b in t_r[1:]]) * 1e3:.1f} ms for the call alone ({rows.nbytes} bytes sent)")
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("ab"); a.add_argument("--parent-tree", required=True); a.add_argument("--pairs", type=int, default=3)
    a.add_argument("--steps", type=int, default=5); a.add_argument("--warmup", type=int, default=2); a.add_argument("--out")
    b = sub.add_parser("stored"); b.add_argument("--reps", type=int, default=3); b.add_argument("--out")
    c = sub.add_parser("render"); c.add_argument("--stored", type=int, default=0)
    d = sub.add_parser("move"); d.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    {"ab": ab, "stored": stored, "render": render, "move": move}[args.cmd](args)
