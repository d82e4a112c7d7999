#!/usr/bin/env python3
"""On the GPU box: what the display stage (cgpt_tonemap) costs, and that the default bench stays where the parent's is.

  call   the warm 1080p call in three cases -- manual exposure, auto exposure, auto exposure on the denoised source -- beside
         Renderer.pixels() (cgpt_read_pixels) of the same frame, which moves the same input bytes to the host's side of the call.  The four
         sides alternate in one process; the median of --reps (>= 20) warm calls with min / max.  Every tonemap call reads back both
         outputs (33 MB of float4 and 8 MB of pixels at 1080p); pixels-only is listed beside it.
  bench  --pairs (3) alternating pairs of the default bench, `bench.py --gpus 1 --steps S --warmup W`, in a checkout of the parent commit
         with its own build (--parent DIR: the binding resolves the new exports, so the parent's library needs the parent's package) and
         in this tree; the result lines as they come and the two means.

usage: python scripts/gpu_tonemap_time.py call [--reps 20] [--spp 16] [--out profiles/r37/tonemap_call.json]
       python scripts/gpu_tonemap_time.py bench --parent DIR [--pairs 3] [--steps 10] [--warmup 3] [--out profiles/r37/bench_ab.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))

from gpu_skin_time import _fmt, _stats

W, H = 1920, 1080


def call(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    from cpugpupathtracing_amd.tonemap import tonemap_params
    reps = max(args.reps, 20)
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H, P.BUILD_SAH_INTERVALS)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, args.spp)
    r.denoise()
    px = np.empty((H, W), np.uint32)

    def pixels_only(**kw):                                                     # the call with dst_rgba NULL
        p, _ = tonemap_params(**kw)
        r._check(r.L.cgpt_tonemap(r._ctx, C.byref(p), None, 0, px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))

    sides = {
        "cgpt_read_pixels": lambda: r.pixels(),
        "tonemap manual (rgba + pixels)": lambda: r.tonemap(auto=False),
        "tonemap auto (rgba + pixels)": lambda: r.tonemap(auto=True),
        "tonemap auto, denoised (rgba + pixels)": lambda: r.tonemap(source="denoised", auto=True),
        "tonemap manual, pixels only": lambda: pixels_only(auto=False),
        "tonemap auto, pixels only": lambda: pixels_only(auto=True),
        "tonemap auto, denoised, pixels only": lambda: pixels_only(source="denoised", auto=True),
    }
    times = {name: [] for name in sides}
    for k in range(2 + reps):                                                  # two warm-up rounds, then the sides alternate
        for name, f in sides.items():
            t0 = time.perf_counter(); f(); t1 = time.perf_counter()
            if k >= 2:
                times[name].append(t1 - t0)
    out = {name: _stats(v) for name, v in times.items()}
    info = r.exposure()
    print(f"{W}x{H}, {args.spp} spp; the last reading: index {info.mean_index:.2f}, exposure {info.exposure:.4f}, {info.n_counted} counted, {info.n_ignored} ignored")
    for name, st in out.items():
        print("  " + _fmt(name, st), flush=True)
    r.close(); s.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)


def bench(args):
    if not args.parent or not os.path.exists(os.path.join(args.parent, "bench.py")):
        sys.exit("bench: --parent DIR must be a built checkout of the parent commit")
    rows = {"parent": [], "this tree": []}
    for pair in range(args.pairs):
        for name, root in (("parent", args.parent), ("this tree", REPO)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)], cwd=root,
                                 capture_output=True, text=True, timeout=900)
            if out.returncode != 0:                                           # a failed run ends the comparison: nothing more is started
                sys.exit(f"bench.py failed in {root} (status {out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
            rows[name].append(json.loads(line))
            print(f"pair {pair} {name}: {line}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rows, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("call", "bench"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"call": call, "bench": bench}[a.mode](a)
