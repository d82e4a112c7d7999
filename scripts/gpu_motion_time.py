#!/usr/bin/env python3
"""On the GPU box: what CGPT_TEMPORAL_FOLLOW_TRANSFORMS costs, on the C3 scene (the glass dragon stand-in, level 6, in
the reference layout) at 1920x1080 after a 4-sample render, default parameters, the packed pixels as the only output -- the set-up of
scripts/gpu_temporal_time.py.  Medians of repeated calls after a warm-up; every call ends in a synchronise (the ABI's calls block).
  plain:   cgpt_denoise_temporal without the flag: the camera of the history (warm) and the camera alternating between two views 0.05
           apart (guides recomputed, reprojection) -- the numbers the `ab` mode compares with the parent commit's library;
  moving:  the camera-alternating call alone (for a kernel trace of temporal_merge<.., MOTION = false>);
  spin:    the flagged call with the stand-in turning 2 degrees before every call (cgpt_scene_update_transforms outside the timed span;
           guides recomputed, reprojection through temporal_merge<.., MOTION = true>); its difference to `moving` is the feature's price;
  ab:      `plain` in child processes, this tree's library and the parent's (--parent-lib) in alternating pairs.
usage: python scripts/gpu_motion_time.py plain|moving|spin [repeats]
       python scripts/gpu_motion_time.py ab --parent-lib PATH [--pairs 3] [--repeats 30]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 1920, 1080


def measure(which, reps):
    import numpy as np
    from cpugpupathtracing_amd import _native as N
    if os.environ.get("CGPT_LIB_PATH"):                        # another build of the library: it may lack the newest helper exports
        probe = C.CDLL(os.environ["CGPT_LIB_PATH"])
        for name in [n for n in N.PROTOTYPES if not hasattr(probe, n)]:
            del N.PROTOTYPES[name]
    import cpugpupathtracing_amd as P
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, 4)
    L, ctx = r.L, r._ctx
    cam_a = s.camera()
    s.set_camera((0.05, 0.0, 8.0), (0.0, 0.0, -1.0), 60.0, W / H)
    cam_b = s.camera()
    px = np.empty((H, W), np.uint32)
    up = px.ctypes.data_as(C.POINTER(C.c_uint32))
    follow = N.TemporalParams(64.0, 0.9, 0.01, getattr(N, "TEMPORAL_FOLLOW_TRANSFORMS", 0))
    n_obj = s.flatten().n_objects

    def temporal(cam, params=None):
        rc = L.cgpt_denoise_temporal(ctx, C.byref(cam), None, C.byref(params) if params is not None else None, None, 0, up, px.size)
        assert rc == 0, L.cgpt_last_error(ctx)

    def turn(k):                                               # the stand-in (object 0) about the vertical axis through the origin
        a = np.deg2rad(2.0 * k)
        m = np.tile(np.eye(3, 4, dtype=np.float32), (n_obj, 1, 1))
        m[0, :, :3] = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        r.update_transforms(m)

    def median_ms(fn, before=None):
        for k in (0, 1):                                       # warm-up (allocations, code objects)
            if before:
                before(k)
            fn(k)
        t = []
        for k in range(2, reps + 2):
            if before:
                before(k)
            t0 = time.perf_counter(); fn(k); t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t)), 1e3 * min(t), 1e3 * max(t)

    res = {}
    if which == "plain":
        res["temporal, warm (same camera)"] = median_ms(lambda k: temporal(cam_a))
    if which in ("plain", "moving"):
        res["temporal, camera alternating (guides + reprojection)"] = median_ms(lambda k: temporal(cam_b if k % 2 else cam_a))
    if which == "spin":
        res["temporal + FOLLOW_TRANSFORMS, mesh turning (guides + carried-back reprojection)"] = median_ms(lambda k: temporal(cam_a, follow), turn)
        hist = r.temporal_history()[..., 3]
        print(f"  after the turning calls {float(np.mean(hist > 4)):.1%} of the pixels carry a reprojected history (the glass first hits drop theirs)")
    print(f"C3 scene {W}x{H}, 4 spp accumulated, default parameters, pixels out; {reps} calls after a warm-up")
    for name, (med, best, worst) in res.items():
        print(f"  {name:84s} median {med:8.3f} ms   best {best:8.3f}   worst {worst:8.3f}")
    print("RESULT " + json.dumps({k: v[0] for k, v in res.items()}))
    r.close()


def ab(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args(argv)
    libs = {"this": None, "parent": os.path.abspath(args.parent_lib)}
    assert os.path.exists(libs["parent"]), libs["parent"]
    values = {"this": {}, "parent": {}}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            env = dict(os.environ)
            if libs[name]:
                env["CGPT_LIB_PATH"] = libs[name]
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "plain", str(args.repeats)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                              # nothing more is started after a failed run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for k, v in res.items():
                values[name].setdefault(k, []).append(v)
            print(f"{name:7s} run {pair}: " + "  ".join(f"{k}: {v:.3f} ms" for k, v in res.items()), flush=True)
    for name, d in values.items():
        for k, xs in d.items():
            print(f"{name:7s} {k:56s} min {min(xs):.3f} max {max(xs):.3f} ms (spread {(max(xs) - min(xs)) / min(xs) * 100:.2f} %)")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
    if mode == "ab":
        ab(sys.argv[2:])
    else:
        assert mode in ("plain", "moving", "spin"), mode
        measure(mode, int(sys.argv[2]) if len(sys.argv) > 2 else 30)
