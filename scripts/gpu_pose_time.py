#!/usr/bin/env python3
"""On the GPU box: what CGPT_TEMPORAL_FOLLOW_POSES costs, on the reference layout around the dragon stand-in (`moving`
and `pose`: level 8, 1.31 M triangles, diffuse, the whole layout four times its size; `plain`: the C3 scene of
scripts/gpu_motion_time.py, level 6, glass) at 1920x1080 after a 4-sample render, default parameters, the packed pixels as the only output.  Medians of repeated calls after a warm-up, with min and max; every call ends in a
synchronise (the ABI's calls block).
  moving:  cgpt_denoise_temporal without the flag, the camera alternating between two views 0.05 apart (guides recomputed, reprojection),
           in a context that holds the stand-in's two-joint skin (so the guides come from guides_tri_kernel, as in `pose`);
  pose:    the flagged call with the stand-in re-posed before every call (cgpt_scene_skin_mesh outside the timed span; guides recomputed,
           pose_carry_back, reprojection through temporal_merge<.., POSE = true>); its difference to `moving` is the feature's price,
           beyond the two calls' run-to-run spreads added together;
  plain:   the unflagged calls in a context without a skin -- cgpt_denoise, cgpt_denoise_temporal (warm and camera-alternating) and the
           CGPT_TEMPORAL_FOLLOW_TRANSFORMS call with the stand-in turning -- the numbers the `ab` mode compares with the parent's library;
  ab:      `plain` in child processes, this tree's library and the parent's (--parent-lib) in alternating pairs.
`pose` also prints the bytes pose_carry_back moves, computed from the shapes: per pixel 32 B of guides and 32 B of record written; per posed
pixel 4 B of triangle index and 192 B of triangle data (48 B current corners, 72 B bind, 24 B joints, 48 B weights; neighbouring pixels
share them) and 36 matrix rows of 16 B through the vector cache.
Why four times the size: intersect_triangle keeps the reference's absolute determinant epsilon, |e1 . (d x e2)| < 0.001 is no hit (SURVEY
A-9).  A level-8 triangle of the stand-in at its own size has edges of about 0.03, a determinant of at most 1e-3: every one of them is
rejected and the mesh is not there, for the guides and the renders alike (at level 7 a third of the hits is already lost).  Scaled by
four the determinant grows by sixteen and the same picture comes back with the mesh in it.
usage: python scripts/gpu_pose_time.py moving|pose|plain [repeats]
       python scripts/gpu_pose_time.py ab --parent-lib PATH [--pairs 3] [--repeats 20]"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H = 1920, 1080
SCALE = 4.0                                                    # of the posed layout (the docstring says why)


def measure(which, reps):
    import numpy as np
    from cpugpupathtracing_amd import _native as N
    if os.environ.get("CGPT_LIB_PATH"):                        # another build of the library: it may lack the newest exports
        probe = C.CDLL(os.environ["CGPT_LIB_PATH"])
        for name in [n for n in N.PROTOTYPES if not hasattr(probe, n)]:
            del N.PROTOTYPES[name]
    import cpugpupathtracing_amd as P
    posing = which in ("moving", "pose")
    mesh = P.Mesh.dragon_standin(8 if posing else 6)
    r = P.Renderer(0)
    if posing:                                                 # the reference layout (Main.cpp:777-819) with the mesh's tree built on the device
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
    else:
        s = P.Scene.reference_layout(mesh, 3, W / H)
    r.upload(s)
    L, ctx = r.L, r._ctx
    cam_a = s.camera()
    s.set_camera((0.05 * (SCALE if posing else 1.0), 0.0, 8.0 * (SCALE if posing else 1.0)), (0.0, 0.0, -1.0), 60.0, W / H)
    cam_b = s.camera()
    px = np.empty((H, W), np.uint32)
    up = px.ctypes.data_as(C.POINTER(C.c_uint32))
    n_obj = s.flatten().n_objects
    centre = None
    if posing:                                                 # the two-joint bend of render_main --bend: the weight on joint 1 is the height
        bind = P.triangles_from_arrays(mesh.vertices, mesh.indices)
        y = bind.reshape(-1, 3, 6)[:, :, 1]
        lo, hi = float(y.min()), float(y.max())
        t = ((y - lo) / (hi - lo)).astype(np.float32)
        j = np.zeros((bind.shape[0], 3, 4), np.uint16); j[..., 1] = 1
        w = np.zeros((bind.shape[0], 3, 4), np.float32); w[..., 0] = np.float32(1.0) - t; w[..., 1] = t
        r.set_skin(0, bind, j, w, 2)
        p = bind.reshape(-1, 6)[:, :3]
        centre = 0.5 * (p.min(0) + p.max(0)).astype(np.float64)
    r.render(W, H, 4)

    def temporal(cam, flags=0):
        params = N.TemporalParams(64.0, 0.9, 0.01, flags)
        rc = L.cgpt_denoise_temporal(ctx, C.byref(cam), None, C.byref(params), None, 0, up, px.size)
        assert rc == 0, L.cgpt_last_error(ctx)

    def denoise(cam):
        rc = L.cgpt_denoise(ctx, C.byref(cam), None, None, 0, up, px.size)
        assert rc == 0, L.cgpt_last_error(ctx)

    def bend(k):                                               # joint 1 about the x axis through the middle of the mesh, 2 degrees a call
        a = np.deg2rad(2.0 * (k % 8))
        c, sn = np.cos(a), np.sin(a)
        rot = np.array([[1, 0, 0], [0, c, -sn], [0, sn, c]])
        m = np.zeros((2, 3, 4), np.float32)
        m[0] = np.eye(3, 4)
        m[1, :, :3], m[1, :, 3] = rot, centre - rot @ centre
        r.skin_mesh(0, m)

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
        res["denoise"] = median_ms(lambda k: denoise(cam_a))
        res["temporal, warm (same camera)"] = median_ms(lambda k: temporal(cam_a))
    if which in ("plain", "moving"):
        res["temporal, camera alternating (guides + reprojection)"] = median_ms(lambda k: temporal(cam_b if k % 2 else cam_a))
    if which == "plain":
        res["temporal + FOLLOW_TRANSFORMS, mesh turning"] = median_ms(lambda k: temporal(cam_a, N.TEMPORAL_FOLLOW_TRANSFORMS), turn)
    if which == "pose":
        res["temporal + FOLLOW_POSES, mesh bending (guides + carry-back + reprojection)"] = median_ms(lambda k: temporal(cam_a, N.TEMPORAL_FOLLOW_POSES), bend)
        st = r.previous_hits()[..., 3].view(np.uint32)
        posed, dropped = int((st == 1).sum()), int((st == 2).sum())
        hist = r.temporal_history()[..., 3]
        print(f"  {posed} of {W * H} pixels re-posed ({posed / (W * H):.1%}), {dropped} dropped; {float(np.mean(hist > 4)):.1%} of the pixels carry a "
              f"reprojected history")
        streamed, gathered, cached = 64 * W * H + 4 * posed, 192 * posed, 576 * posed
        print(f"  pose_carry_back bytes from the shapes: {streamed / 1e6:.1f} MB streamed (64 B a pixel, 4 B of index a posed pixel), {gathered / 1e6:.1f} MB of triangle data "
              f"(192 B a posed pixel, shared by the pixels of a triangle), {cached / 1e6:.1f} MB of matrix rows through the vector cache")
    print(f"stand-in level {8 if posing else 6}, {W}x{H}, 4 spp accumulated, default parameters, pixels out; {reps} calls after a warm-up")
    for name, (med, best, worst) in res.items():
        print(f"  {name:84s} median {med:8.3f} ms   min {best:8.3f}   max {worst:8.3f}")
    print("RESULT " + json.dumps({k: v[0] for k, v in res.items()}))
    r.close()


def ab(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
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
            print(f"{name:7s} {k:56s} mean {sum(xs) / len(xs):.3f} min {min(xs):.3f} max {max(xs):.3f} ms (spread {(max(xs) - min(xs)) / min(xs) * 100:.2f} %)")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "pose"
    if mode == "ab":
        ab(sys.argv[2:])
    else:
        assert mode in ("moving", "pose", "plain"), mode
        measure(mode, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
