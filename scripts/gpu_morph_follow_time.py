#!/usr/bin/env python3
"""On the GPU box: what CGPT_TEMPORAL_FOLLOW_MORPHS costs, on the scene of scripts/gpu_pose_time.py -- the reference
layout around the level-8 dragon stand-in (1.31 M triangles, diffuse) at four times its size (that script says why) -- at 1920x1080
after a 4-sample render, default parameters, the packed pixels as the only output.  --targets (52) targets are installed on the
stand-in: target k pushes every corner along its normal by a sine of its height, so the surface stays connected.  Medians of repeated
calls after a warm-up, with min and max; every call ends in a synchronise (the ABI's calls block).
  follow:  for the targets stored in leaf-slot order and as given, without and with gpu_pose_time's two-joint skin posed once (the fused
           path), and K = --active (1 8 52) history-active targets: the flagged call with the stand-in re-morphed before every call
           (cgpt_scene_morph_mesh outside the timed span; guides recomputed, morph_carry_back, reprojection through
           temporal_merge<.., POSE = true>), against `moving`, the unflagged call of the same context with the camera alternating between
           two views (guides recomputed, reprojection).  The difference is the feature's price where it exceeds the two calls' run-to-run
           spreads added together.  Also printed: the bytes morph_carry_back moves per re-posed pixel, from the shapes;
  trace:   --calls flagged calls per layout, skin and K, for a kernel trace around them:
           rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/gpu_morph_follow_time.py trace
  summary: morph_carry_back's times out of that trace (DIR/.../*_kernel_trace.csv), in launch order per configuration, and the slope per added
           history-active target (no GPU needed): python scripts/gpu_morph_follow_time.py summary KERNEL_TRACE.csv
  plain:   the paths this feature leaves alone, in contexts of their own -- cgpt_denoise, cgpt_denoise_temporal warm and
           camera-alternating, the CGPT_TEMPORAL_FOLLOW_TRANSFORMS call with the stand-in turning (level 6, glass: gpu_pose_time's `plain`),
           the CGPT_TEMPORAL_FOLLOW_POSES call with the level-8 stand-in bending, and the call times of cgpt_scene_set_morph_targets (8
           targets, leaf-slot order: it now uploads the slot map) and cgpt_scene_morph_mesh on that mesh;
  ab:      `plain` in child processes, this tree's library and the parent's (--parent-lib) in alternating pairs.
usage: python scripts/gpu_morph_follow_time.py follow [--reps 20] [--active 1 8 52] [--targets 52] [--out FILE.json]
       python scripts/gpu_morph_follow_time.py trace [--calls 6] [--active 1 8 52] [--targets 52]
       python scripts/gpu_morph_follow_time.py summary KERNEL_TRACE.csv [--calls 6] [--active 1 8 52]
       python scripts/gpu_morph_follow_time.py plain [--reps 20]
       python scripts/gpu_morph_follow_time.py ab --parent-lib PATH [--pairs 3] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 1920, 1080
SCALE = 4.0
FOLLOW_TRANSFORMS, FOLLOW_POSES, FOLLOW_MORPHS = 4, 16, 32


def _native():
    from cpugpupathtracing_amd import _native as N
    if os.environ.get("CGPT_LIB_PATH"):                        # another build of the library: it may lack the newest exports
        probe = C.CDLL(os.environ["CGPT_LIB_PATH"])
        for name in [n for n in N.PROTOTYPES if not hasattr(probe, n)]:
            del N.PROTOTYPES[name]
    return N


def _big_scene(r, level=8):
    """gpu_pose_time's posed layout: (scene, the stand-in's triangles, two cameras 0.05 apart)"""
    import numpy as np
    import cpugpupathtracing_amd as P
    mesh = P.Mesh.dragon_standin(level)
    s = P.Scene()
    for m in P.REFERENCE_MATERIALS:
        s.add_material(m)
    big = mesh.vertices.copy()
    big[:, :3] *= np.float32(SCALE)
    mesh = P.Mesh.from_arrays(big, mesh.indices)
    s.add_mesh(mesh, 1, P.BUILD_SAH_INTERVALS, device_builder=r)
    ground = np.array([[-1000, -3, 1000, 0, 1, 0], [-1000, -3, -1000, 0, 1, 0], [1000, -3, -1000, 0, 1, 0], [1000, -3, 1000, 0, 1, 0]], np.float32)
    ground[:, :3] *= np.float32(SCALE)
    s.add_mesh(P.Mesh.from_arrays(ground, np.array([0, 1, 2, 2, 3, 0], np.uint32)), 1)
    for c in ((10.0, 10.0, 10.0), (-10.0, 10.0, -10.0)):
        s.add_light(s.add_sphere(tuple(SCALE * x for x in c), 5.0 * SCALE, 2))
    s.set_camera((0.0, 0.0, 8.0 * SCALE), (0.0, 0.0, -1.0), 60.0, W / H)
    s.set_settings(P.Settings())
    r.upload(s)
    cam_a = s.camera()
    s.set_camera((0.05 * SCALE, 0.0, 8.0 * SCALE), (0.0, 0.0, -1.0), 60.0, W / H)
    cam_b = s.camera()
    return s, P.triangles_from_arrays(mesh.vertices, mesh.indices), (cam_a, cam_b)


def _targets(tris, n_targets):
    """(n_targets, n, 18) float32: target k moves a corner along its normal by 0.5 % of the mesh's height times sin((k + 1) pi t + k), t its height"""
    import numpy as np
    c = tris.reshape(-1, 3, 6)
    y = c[..., 1].astype(np.float64)
    t = (y - y.min()) / (y.max() - y.min())
    amp = 0.005 * float(y.max() - y.min())
    d = np.zeros((n_targets,) + c.shape, np.float32)
    for k in range(n_targets):
        d[k, ..., :3] = (amp * np.sin((k + 1) * np.pi * t + k)).astype(np.float32)[..., None] * c[..., 3:]
    return d.reshape(n_targets, -1, 18)


def _skin(tris):
    """gpu_pose_time's two-joint bend: (joints, weights, matrices(k))"""
    import numpy as np
    y = tris.reshape(-1, 3, 6)[:, :, 1]
    t = ((y - y.min()) / (y.max() - y.min())).astype(np.float32)
    j = np.zeros(y.shape + (4,), np.uint16); j[..., 1] = 1
    w = np.zeros(y.shape + (4,), np.float32); w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
    p = tris.reshape(-1, 6)[:, :3]
    centre = 0.5 * (p.min(0) + p.max(0)).astype(np.float64)

    def matrices(k):
        a = np.deg2rad(2.0 * (k % 8))
        cs, sn = np.cos(a), np.sin(a)
        rot = np.array([[1, 0, 0], [0, cs, -sn], [0, sn, cs]])
        m = np.zeros((2, 3, 4), np.float32)
        m[0] = np.eye(3, 4)
        m[1, :, :3], m[1, :, 3] = rot, centre - rot @ centre
        return m
    return j, w, matrices


def _weights(n_targets, k_active, phase):
    """k_active nonzero weights spread over the targets, another value every call"""
    import numpy as np
    w = np.zeros(n_targets, np.float32)
    idx = np.linspace(0, n_targets - 1, k_active).round().astype(int)
    w[idx] = (0.6 + 0.1 * (phase % 5)) * np.where(np.arange(k_active) % 2, -1.0, 1.0)
    return w


def _stats(t):
    import numpy as np
    return {"median_ms": 1e3 * float(np.median(t)), "min_ms": 1e3 * min(t), "max_ms": 1e3 * max(t)}


def _timed(fn, reps, before=None):
    for k in (0, 1):                                           # warm-up (allocations, code objects)
        if before:
            before(k)
        fn(k)
    t = []
    for k in range(2, reps + 2):
        if before:
            before(k)
        t0 = time.perf_counter(); fn(k); t.append(time.perf_counter() - t0)
    return _stats(t)


def _fmt(s):
    return f"median {s['median_ms']:8.3f} ms   min {s['min_ms']:8.3f}   max {s['max_ms']:8.3f}"


def _calls(r, N):
    import numpy as np
    px = np.empty((H, W), np.uint32)
    up = px.ctypes.data_as(C.POINTER(C.c_uint32))
    L, ctx = r.L, r._ctx

    def temporal(cam, flags=0):
        params = N.TemporalParams(64.0, 0.9, 0.01, flags)
        rc = L.cgpt_denoise_temporal(ctx, C.byref(cam), None, C.byref(params), None, 0, up, px.size)
        assert rc == 0, L.cgpt_last_error(ctx)

    def denoise(cam):
        rc = L.cgpt_denoise(ctx, C.byref(cam), None, None, 0, up, px.size)
        assert rc == 0, L.cgpt_last_error(ctx)
    return temporal, denoise


def follow(args, tracing=False):
    import numpy as np
    N = _native()
    import cpugpupathtracing_amd as P
    r = P.Renderer(0)
    s, tris, (cam_a, cam_b) = _big_scene(r)
    deltas = _targets(tris, args.targets)
    j, sw, matrices = _skin(tris)
    temporal, _ = _calls(r, N)
    r.render(W, H, 4)
    out = {"triangles": int(tris.shape[0]), "targets": args.targets, "runs": []}
    print(f"{tris.shape[0]} triangles, {args.targets} targets installed, {W}x{H}, 4 spp accumulated, default parameters, pixels out", flush=True)
    for leaf in (1, 0):
        r.set_tuning(morph_leaf_order=leaf)
        r.clear_skin(0)
        r.set_morph_targets(0, tris, deltas)
        for skinned in (False, True):
            if skinned:
                r.set_skin(0, tris, j, sw, 2)
                r.skin_mesh(0, matrices(3))                    # posed once: every morph from here on goes through the joints
            r.morph_mesh(0, _weights(args.targets, 1, 0))
            if not tracing:
                moving = _timed(lambda k: temporal(cam_b if k % 2 else cam_a), args.reps)
            for k_active in args.active:
                morph = lambda k: r.morph_mesh(0, _weights(args.targets, k_active, k))
                tag = f"layout {'leaf-slot' if leaf else 'as given'}, {'morph + skin' if skinned else 'morph alone'}, K = {k_active}"
                if tracing:
                    r.temporal_reset()                         # no history: the call that stores the history's K launches no carry-back
                    morph(0); temporal(cam_a, FOLLOW_POSES | FOLLOW_MORPHS)
                    for k in range(1, args.calls + 1):
                        morph(k); temporal(cam_a, FOLLOW_POSES | FOLLOW_MORPHS)
                    print(f"  {tag}: {args.calls} flagged calls", flush=True)
                    continue
                flagged = _timed(lambda k: temporal(cam_a, FOLLOW_POSES | FOLLOW_MORPHS), args.reps, morph)
                st = r.previous_hits()[..., 3].view(np.uint32)
                posed, dropped = int((st == 1).sum()), int((st == 2).sum())
                kept = float(np.mean(r.temporal_history()[..., 3] > 4))
                cost = flagged["median_ms"] - moving["median_ms"]
                spreads = (flagged["max_ms"] - flagged["min_ms"]) + (moving["max_ms"] - moving["min_ms"])
                gathered = 4 + 48 + (4 if leaf else 0) + 72 + 72 * k_active + (72 if skinned else 0)
                print(f"  {tag}\n    flagged, re-morphed before every call   {_fmt(flagged)}\n    unflagged, camera alternating           {_fmt(moving)}\n"
                      f"    difference {cost:+.3f} ms; the two spreads together {spreads:.3f} ms: {'a cost' if cost > spreads else 'within the spreads'}\n"
                      f"    {posed} of {W * H} pixels re-posed ({posed / (W * H):.1%}), {dropped} dropped; {kept:.1%} of the pixels carry a reprojected history\n"
                      f"    morph_carry_back from the shapes: 64 B a pixel streamed; {gathered} B gathered a re-posed pixel (index, current corners, "
                      f"{'slot, ' if leaf else ''}base, 72 B a history-active target{', joints and weights' if skinned else ''})"
                      f"{' and 36 matrix rows of 16 B through the vector cache' if skinned else ''}", flush=True)
                out["runs"].append({"leaf_order": leaf, "skinned": skinned, "active": k_active, "flagged": flagged, "moving": moving, "difference_ms": cost,
                                    "spreads_ms": spreads, "reposed_pixels": posed, "dropped_pixels": dropped, "gathered_bytes_per_reposed_pixel": gathered})
    if args.out and not tracing:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    r.close()


def summary(args):
    import csv
    rows = [row for row in csv.DictReader(open(args.csv)) if "morph_carry_back" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    us = [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows]
    per = args.calls                                           # the call that stores the history's K launches none
    k = 0
    for leaf in (1, 0):
        for skinned in (False, True):
            med = []
            for k_active in args.active:
                chunk = sorted(us[k:k + per]); k += per
                if not chunk:
                    continue
                med.append(chunk[len(chunk) // 2])
                print(f"layout {'leaf-slot' if leaf else 'as given'}, {'morph + skin' if skinned else 'morph alone'}, K = {k_active:3d}: morph_carry_back median "
                      f"{med[-1]:8.1f} us (min {chunk[0]:.1f}, max {chunk[-1]:.1f}; {len(chunk)} launches)")
            if len(med) == len(args.active) and len(med) > 1:
                print(f"  per added history-active target: {(med[-1] - med[0]) / (args.active[-1] - args.active[0]):.2f} us")
    print(f"{len(us)} morph_carry_back launches in the trace, {k} used")


def plain(args):
    import numpy as np
    N = _native()
    import cpugpupathtracing_amd as P
    res = {}
    r = P.Renderer(0)                                          # gpu_pose_time's `plain`: level 6, glass, no skin, no targets
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
    r.upload(s)
    cam_a = s.camera()
    s.set_camera((0.05, 0.0, 8.0), (0.0, 0.0, -1.0), 60.0, W / H)
    cam_b = s.camera()
    n_obj = s.flatten().n_objects
    temporal, denoise = _calls(r, N)
    r.render(W, H, 4)

    def turn(k):
        a = np.deg2rad(2.0 * k)
        m = np.tile(np.eye(3, 4, dtype=np.float32), (n_obj, 1, 1))
        m[0, :, :3] = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        r.update_transforms(m)
    res["denoise"] = _timed(lambda k: denoise(cam_a), args.reps)
    res["temporal, warm (same camera)"] = _timed(lambda k: temporal(cam_a), args.reps)
    res["temporal, camera alternating"] = _timed(lambda k: temporal(cam_b if k % 2 else cam_a), args.reps)
    res["temporal + FOLLOW_TRANSFORMS, mesh turning"] = _timed(lambda k: temporal(cam_a, FOLLOW_TRANSFORMS), args.reps, turn)
    r.close()
    r = P.Renderer(0)                                          # gpu_pose_time's `pose`: level 8, the two-joint skin
    s, tris, (cam_a, cam_b) = _big_scene(r)
    j, sw, matrices = _skin(tris)
    r.set_skin(0, tris, j, sw, 2)
    temporal, _ = _calls(r, N)
    r.render(W, H, 4)
    res["temporal + FOLLOW_POSES, mesh bending"] = _timed(lambda k: temporal(cam_a, FOLLOW_POSES), args.reps, lambda k: r.skin_mesh(0, matrices(k)))
    r.clear_skin(0)
    deltas = _targets(tris, 8)
    res["set_morph_targets, 8 targets, leaf-slot order"] = _timed(lambda k: r.set_morph_targets(0, tris, deltas), 3)
    res["morph_mesh, 8 of 8 targets active"] = _timed(lambda k: r.morph_mesh(0, _weights(8, 8, k)), args.reps)
    r.close()
    print(f"{W}x{H}, 4 spp accumulated, default parameters, pixels out; {args.reps} calls after a warm-up")
    for name, st in res.items():
        print(f"  {name:52s} {_fmt(st)}")
    print("RESULT " + json.dumps({k: v["median_ms"] for k, v in res.items()}))


def ab(args):
    libs = {"this": None, "parent": os.path.abspath(args.parent_lib)}
    assert os.path.exists(libs["parent"]), libs["parent"]
    values = {"this": {}, "parent": {}}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            env = dict(os.environ)
            if libs[name]:
                env["CGPT_LIB_PATH"] = libs[name]
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "plain", "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=400)
            if p.returncode != 0:                              # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for k, v in res.items():
                values[name].setdefault(k, []).append(v)
            print(f"{name:7s} run {pair}: " + "  ".join(f"{k}: {v:.3f} ms" for k, v in res.items()), flush=True)
    for k in values["this"]:
        a, b = values["this"][k], values["parent"][k]
        mean = sum(a) / len(a)
        inside = min(b) <= mean <= max(b)
        spreads = (max(a) - min(a)) + (max(b) - min(b))
        verdict = "within the parent's min-max" if inside else ("the difference lies inside the two spreads" if abs(mean - sum(b) / len(b)) <= spreads else "OUTSIDE")
        print(f"{k:52s} this mean {mean:.3f} (min {min(a):.3f} max {max(a):.3f})  parent mean {sum(b) / len(b):.3f} (min {min(b):.3f} max {max(b):.3f}) ms: {verdict}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("follow", "trace", "summary", "plain", "ab"))
    ap.add_argument("csv", nargs="?")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--active", type=int, nargs="+", default=[1, 8, 52])
    ap.add_argument("--targets", type=int, default=52)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "follow":
        follow(a)
    elif a.mode == "trace":
        follow(a, tracing=True)
    elif a.mode == "summary":
        summary(a)
    elif a.mode == "plain":
        plain(a)
    else:
        ab(a)
