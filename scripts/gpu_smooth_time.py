#!/usr/bin/env python3
"""On the GPU box: what smooth shading (cgpt_scene_update_smooth_normals) costs.

  ab      the default bench (bench.py --gpus 1) of this tree and of a built checkout of the parent commit, alternating A B A B in child
          processes: a scene without a flag runs the parent's instantiations, so the two should differ by no more than each one's own
          run-to-run spread.  Both spreads are printed.
  smooth  the reference layout around the dragon stand-in (level 6, glass) at 1920x1080, 256 spp, the wavefront pipeline, with the flag
          off and on, alternating: ms per render (cgpt_stats.kernel_ms, median of the repeats) and the trace kernels' share.
  render  one warm-up and one 256-spp render of that scene with one pool, flag off or on, for a kernel trace around it
          (rocprofv3 --kernel-trace --stats -- python scripts/gpu_smooth_time.py render --smooth 1): wf_shade's time.
  upload  cgpt_scene_upload of the 1.31 M-triangle scene (bench.py's big scene: the bumpy icosphere, level 8): seconds per upload (median)
          and the device bytes the library holds after it; --tree PATH measures a built checkout of the parent instead (the call is old).

usage: python scripts/gpu_smooth_time.py ab --parent-tree PATH [--pairs 2] [--steps 5] [--warmup 2]
       python scripts/gpu_smooth_time.py smooth [--reps 3] [--out FILE.json]
       python scripts/gpu_smooth_time.py render --smooth 1
       python scripts/gpu_smooth_time.py upload [--reps 3] [--tree PATH]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 1920, 1080, 256


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
        print(f"{name:7s} value min {min(xs):.6g} max {max(xs):.6g} spread {(max(xs) - min(xs)) / min(xs) * 100:.2f} %")
    if args.out:
        json.dump(values, open(args.out, "w"), indent=1)


def _flags(scene, on):
    """1 on every mesh object that is not a light (the dragon stand-in and the ground quad), else 0."""
    import numpy as np
    from cpugpupathtracing_amd import _native as N
    desc = scene.flatten()
    flags = np.array([1 if on and desc.objects[k].kind == N.OBJECT_MESH else 0 for k in range(desc.n_objects)], np.uint32)
    for k in range(desc.n_lights):
        flags[desc.light_indices[k]] = 0
    return flags


def smooth(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    r.upload(s)
    rows = {0: [], 1: []}
    for on in (0, 1):                                          # warm-up of both lobe levels
        r.update_smooth_normals(_flags(s, on))
        r.reset_accumulator(); r.render(W, H, SPP, seed=1, kernel=P.KERNEL_WAVEFRONT, settings=st)
    for i in range(args.reps):
        for on in (0, 1):
            r.update_smooth_normals(_flags(s, on))
            r.reset_accumulator(); r.reset_stats()
            r.render(W, H, SPP, seed=1000 + i, kernel=P.KERNEL_WAVEFRONT, settings=st)
            stt = r.stats()
            rows[on].append({"ms": stt.kernel_ms, "trace_ms": stt.dominant_ms, "traced_rays": int(stt.traced_rays)})
            print(f"smooth {on} rep {i}: {stt.kernel_ms:8.2f} ms  trace {stt.dominant_ms:8.2f} ms  {stt.traced_rays} rays", flush=True)
    med = {on: float(np.median([x["ms"] for x in rows[on]])) for on in rows}
    print(f"{W}x{H}, {SPP} spp, ADVANCED, wavefront: flat {med[0]:.2f} ms, smooth {med[1]:.2f} ms ({(med[1] / med[0] - 1.0) * 100:+.2f} %)")
    if args.out:
        json.dump({"width": W, "height": H, "spp": SPP, "runs": {str(k): v for k, v in rows.items()}, "median_ms": {str(k): v for k, v in med.items()}},
                  open(args.out, "w"), indent=1)
    r.close()


def render(args):
    import cpugpupathtracing_amd as P
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    r.upload(s)
    r.set_tuning(pools=1)
    r.update_smooth_normals(_flags(s, args.smooth))
    for seed in (1, 2):
        r.reset_accumulator(); r.reset_stats()
        r.render(W, H, SPP, seed=seed, kernel=P.KERNEL_WAVEFRONT, settings=st)
    print(f"smooth {args.smooth}: {r.stats().kernel_ms:.2f} ms with one pool")
    r.close()


def upload(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.bumpy_icosphere(8, (0.0, 6.0, -30.0), (24.0, 10.0, 16.0), 0.15)
    s = P.Scene.reference_layout(mesh, 3, W / H)
    desc = s.flatten()
    r = P.Renderer(0)
    live = getattr(r.L, "cgpt_debug_live_device_bytes")
    live.restype = C.c_uint64
    before = live()
    times = []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        r._check(r.L.cgpt_scene_upload(r._ctx, C.byref(desc)))
        r.synchronize()
        times.append(time.perf_counter() - t0)
    print(f"{desc.n_triangles} triangles, tree {os.path.dirname(os.path.dirname(os.path.abspath(P.__file__)))}: "
          f"upload {np.median(times[1:]) * 1e3:.1f} ms (first {times[0] * 1e3:.1f}, min {min(times[1:]) * 1e3:.1f}, max {max(times[1:]) * 1e3:.1f}), "
          f"device bytes of the scene {live() - before}")
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("ab"); a.add_argument("--parent-tree", required=True); a.add_argument("--pairs", type=int, default=2)
    a.add_argument("--steps", type=int, default=5); a.add_argument("--warmup", type=int, default=2); a.add_argument("--out")
    b = sub.add_parser("smooth"); b.add_argument("--reps", type=int, default=3); b.add_argument("--out")
    c = sub.add_parser("render"); c.add_argument("--smooth", type=int, default=0)
    d = sub.add_parser("upload"); d.add_argument("--reps", type=int, default=3); d.add_argument("--tree", default=REPO)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(getattr(args, "tree", REPO)))
    {"ab": ab, "smooth": smooth, "render": render, "upload": upload}[args.cmd](args)
