#!/usr/bin/env python3
"""On the GPU box: what mesh instancing (cgpt_scene_upload_instanced) saves and what it costs.

The forest of scripts/gpu_tlas_time.py -- N placed instances of a level-1 icosphere (80 triangles, each under its own rotation, scale
and shift) over a ground quad with two sphere lights, in Morton order, the top-level tree on, 1920x1080, ADVANCED -- built with
Scene.add_instance and uploaded both ways, N in 8, 32, 128, 512.  Per N: the upload's wall time (median of the repeats) and the
scene's device bytes for each upload, and ms per render (cgpt_stats.kernel_ms) for each of the three kernels in alternating
plain / instanced pairs on two renderers.  Both uploads run the same kernels on the same records, so the expectation is instanced <=
plain within the plain side's own spread, which is printed.
One more row has a mesh large enough that the plain upload of 512 placements is refused (--big-level, a level-7 icosphere: 327680
triangles, 168 M records against the 2^26 limit): the refusal's message, and the instanced upload's bytes and render times.

Every row runs in a child process of its own under a time limit; after a row that fails or runs out of time nothing more is started.

usage: python scripts/gpu_instancing_time.py [--counts 8,32,128,512] [--pairs 3] [--big-level 7] [--big-count 512] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
W, H = 1920, 1080
SPP = {"megakernel": 4, "persistent": 16, "wavefront": 16}        # as scripts/gpu_tlas_time.py
ROW_SECONDS = 240


def _forest(n, level, seed=1):
    """gpu_tlas_time._forest in Morton order with the instances as instances: the first placement owns the mesh, the others share it."""
    import numpy as np
    import cpugpupathtracing_amd as P
    from gpu_tlas_time import _icosphere
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
    mesh = P.Mesh.from_arrays(*_icosphere(level))
    cells = [(x, z) for x in range(side) for z in range(side)][:n]
    rng.shuffle(cells)
    owner = None
    for x, z in cells:
        axis = rng.standard_normal(3); axis /= np.linalg.norm(axis)
        a = rng.uniform(0.0, 3.0)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        A = (np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)) @ np.diag(rng.uniform(0.7, 1.3, 3))
        b = np.array([3.2 * (x - 0.5 * (side - 1)) + rng.uniform(-0.4, 0.4), rng.uniform(1.3, 2.5), 3.2 * (z - 0.5 * (side - 1)) + rng.uniform(-0.4, 0.4)])
        m = np.concatenate([A, b[:, None]], 1).astype(np.float32)
        if owner is None:
            owner = s.add_mesh(mesh, leaf, transform=m)
        else:
            s.add_instance(owner, leaf, transform=m)
    s.set_camera((0.0, 1.1 * half, 2.2 * half), (0.0, -0.45, -1.0), 50.0, W / H)
    s.sort_objects_spatially()
    return s


def row(args):
    """One N in this process: prints one JSON line."""
    import numpy as np
    import cpugpupathtracing_amd as P
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    kernels = {"megakernel": P.KERNEL_MEGAKERNEL, "persistent": P.KERNEL_PERSISTENT, "wavefront": P.KERNEL_WAVEFRONT}
    s = _forest(args.n, args.level)
    out = {"n": args.n, "level": args.level, "triangles_per_mesh": 20 * 4 ** args.level}
    rs = {}
    for name, instanced in (("plain", False), ("instanced", True)):
        r = P.Renderer(0)
        r.set_top_level(True)
        ms = []
        try:
            for _ in range(args.pairs):
                t0 = time.perf_counter(); r.upload(s, instanced=instanced); r.synchronize(); ms.append(1e3 * (time.perf_counter() - t0))
        except P.DeviceError as e:                               # the plain upload of the big row: refused, and the message is the result
            out[name] = {"refused": str(e)}
            r.close()
            continue
        fp = r.scene_footprint()
        out[name] = {"upload_ms": float(np.median(ms)), "upload_runs": ms, "device_bytes": fp.device_bytes, "n_mesh_copies": fp.n_mesh_copies,
                     "n_leaf_records": fp.n_leaf_records}
        rs[name] = r
    for kname, kernel in kernels.items():
        runs = {name: [] for name in rs}
        for name, r in rs.items():                               # warm-up
            r.reset_accumulator(); r.render(W, H, SPP[kname], seed=1, kernel=kernel, settings=st)
        for i in range(args.pairs):
            for name, r in rs.items():                           # alternating plain, instanced
                r.reset_accumulator(); r.reset_stats()
                r.render(W, H, SPP[kname], seed=100 + i, kernel=kernel, settings=st)
                runs[name].append(r.stats().kernel_ms)
        for name in rs:
            out[name][kname + "_ms"] = float(np.median(runs[name])); out[name][kname + "_runs"] = runs[name]
    if len(rs) == 2:                                             # and the two hold the same image
        for r in rs.values():
            r.reset_accumulator(); r.render(W, H, 1, seed=7, kernel=P.KERNEL_MEGAKERNEL, settings=st)
        out["same_image"] = bool(np.array_equal(rs["plain"].accumulator().view(np.uint32), rs["instanced"].accumulator().view(np.uint32)))
    for r in rs.values():
        r.close()
    s.close()
    print(json.dumps(out), flush=True)


def _show(res):
    for name in ("plain", "instanced"):
        v = res.get(name, {})
        if "refused" in v:
            print(f"N {res['n']:4d} x {res['triangles_per_mesh']:7d} tris  {name:9s}: refused: {v['refused']}", flush=True)
            continue
        spread = lambda k: (max(v[k]) - min(v[k])) / min(v[k]) * 100.0
        print(f"N {res['n']:4d} x {res['triangles_per_mesh']:7d} tris  {name:9s}: upload {v['upload_ms']:9.2f} ms  {v['device_bytes'] / 1e6:10.3f} MB  {v['n_mesh_copies']:4d} copies  " +
              "  ".join(f"{k} {v[k + '_ms']:8.3f} ms (spread {spread(k + '_runs'):4.1f} %)" for k in SPP), flush=True)
    if "same_image" in res:
        print(f"N {res['n']:4d}: one-sample megakernel frames equal to the bit: {res['same_image']}", flush=True)


def main(args):
    rows = [(int(x), 1) for x in args.counts.split(",") if x] + ([(args.big_count, args.big_level)] if args.big_level > 0 else [])
    results = []
    for n, level in rows:
        cmd = [sys.executable, os.path.abspath(__file__), "--row", "--n", str(n), "--level", str(level), "--pairs", str(args.pairs)]
        try:
            p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=ROW_SECONDS)
        except subprocess.TimeoutExpired:
            sys.stderr.write(f"N {n} level {level}: no result within {ROW_SECONDS} s; stopping\n")
            sys.exit(124)
        if p.returncode != 0:                                    # nothing more is started after a failed row
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode if p.returncode > 0 else 1)
        res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        results.append(res)
        _show(res)
        if args.out:
            json.dump({"width": W, "height": H, "spp": SPP, "rows": results}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="8,32,128,512"); ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--big-level", type=int, default=7); ap.add_argument("--big-count", type=int, default=512); ap.add_argument("--out")
    ap.add_argument("--row", action="store_true"); ap.add_argument("--n", type=int, default=8); ap.add_argument("--level", type=int, default=1)
    a = ap.parse_args()
    row(a) if a.row else main(a)
