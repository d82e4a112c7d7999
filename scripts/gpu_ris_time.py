#!/usr/bin/env python3
"""On the GPU box: what resampled light sampling (cgpt_set_nee_candidates) costs and buys.

  ab      the default bench (bench.py --gpus 1) with this build and with a build of the parent commit, alternating A B A B in child
          processes: the one-candidate renders run the parent's instantiations, so the two should differ by no more than each one's own
          run-to-run spread.  Both spreads are printed.
  lights  the many-light scene -- the reference layout around the dragon stand-in plus 64 small sphere lights of mixed power, defined
          below -- at 1920x1080, 256 spp, the wavefront pipeline, for M in 1, 2, 4, 8, 16, 32: ms per render (cgpt_stats.kernel_ms,
          median of the repeats), RMSE against a 16 384-spp M = 1 image, and the equal-time efficiency 1 / (MSE ms) relative to M = 1.
  render  one warm-up and one 256-spp render of the many-light scene at M candidates with one pool, for a kernel trace around it
          (rocprofv3 --kernel-trace --stats -- python scripts/gpu_ris_time.py render --m 8): wf_shade's time per launch, i.e. per round.

usage: python scripts/gpu_ris_time.py ab --parent-lib PATH [--pairs 2] [--steps 5] [--warmup 2]
       python scripts/gpu_ris_time.py lights [--reps 3] [--ref-spp 16384] [--out FILE.json]
       python scripts/gpu_ris_time.py render --m 8"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
W, H, SPP = 1920, 1080, 256
CANDIDATES = (1, 2, 4, 8, 16, 32)


def many_light_scene():
    import numpy as np
    import cpugpupathtracing_amd as P
    s = P.Scene.reference_layout(P.Mesh.dragon_standin(6), 3, W / H)
    rng = np.random.default_rng(64)
    n = 0
    while n < 64:
        pos = np.array([rng.uniform(-14.0, 14.0), rng.uniform(-1.5, 9.0), rng.uniform(-14.0, 6.0)])
        if np.linalg.norm(pos) < 4.5:                          # clear of the mesh
            continue
        hue = rng.dirichlet((1.0, 1.0, 1.0)) * 3.0
        power = float(10.0 ** rng.uniform(0.0, 2.0))           # 1 .. 100, log-uniform
        m = s.add_material(P.Material(emissive=tuple(np.minimum(hue, 2.0)), intensity=power, is_light=True))
        s.add_light(s.add_sphere(tuple(pos), float(rng.uniform(0.15, 0.4)), m))
        n += 1
    return s


def ab(args):
    libs = {"this": None, "parent": os.path.abspath(args.parent_lib)}
    assert os.path.exists(libs["parent"]), libs["parent"]
    values = {"this": [], "parent": []}
    for pair in range(args.pairs):
        for name in ("this", "parent"):
            env = dict(os.environ)
            if libs[name]:
                env["CGPT_LIB_PATH"] = libs[name]
            p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--cpu-seconds", "0", "--no-roofline-pass"], env=env, capture_output=True, text=True, timeout=300)
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


def lights(args):
    import numpy as np
    import cpugpupathtracing_amd as P
    s = many_light_scene()
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, args.ref_spp, seed=0xBEEF, kernel=P.KERNEL_WAVEFRONT, settings=st)
    ref = r.accumulator()[..., :3].astype(np.float64) / args.ref_spp
    print(f"many-light scene {W}x{H}, ADVANCED, wavefront; reference {args.ref_spp} spp at M = 1: {r.stats().kernel_ms:.1f} ms, mean radiance {ref.mean():.4f}", flush=True)
    rows = []
    for M in CANDIDATES:
        r.set_nee_candidates(M)
        r.reset_accumulator(); r.render(W, H, SPP, seed=1, kernel=P.KERNEL_WAVEFRONT, settings=st)      # warm-up
        ms, mse = [], []
        for i in range(args.reps):
            r.reset_accumulator(); r.reset_stats()
            r.render(W, H, SPP, seed=1000 + i, kernel=P.KERNEL_WAVEFRONT, settings=st)
            stt = r.stats()
            ms.append(stt.kernel_ms)
            img = r.accumulator()[..., :3].astype(np.float64) / SPP
            mse.append(float(np.mean((img - ref) ** 2)))
        rows.append({"M": M, "ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "mse_raw": float(np.mean(mse)),
                     "trace_ms": stt.dominant_ms, "trace_launches": stt.dominant_launches, "traced_rays": int(stt.traced_rays)})
    # the reference carries SPP / ref_spp of the M = 1 variance itself: taken off every raw MSE
    ref_noise = rows[0]["mse_raw"] / (1.0 + args.ref_spp / SPP)
    for row in rows:
        row["mse"] = row["mse_raw"] - ref_noise
        row["rmse"] = row["mse"] ** 0.5
        row["efficiency"] = (rows[0]["mse_raw"] - ref_noise) * rows[0]["ms"] / (row["mse"] * row["ms"])
        print(f"M {row['M']:2d}  {row['ms']:8.2f} ms (min {row['ms_min']:.2f} max {row['ms_max']:.2f})  trace {row['trace_ms']:8.2f} ms in {row['trace_launches']} launches  "
              f"RMSE {row['rmse']:.5f} (raw MSE {row['mse_raw']:.3e})  efficiency vs M = 1 {row['efficiency']:.2f}x", flush=True)
    best = max(rows, key=lambda x: x["efficiency"])
    print(f"equal-time efficiency peaks at M = {best['M']}: {best['efficiency']:.2f}x")
    if args.out:
        json.dump({"width": W, "height": H, "spp": SPP, "ref_spp": args.ref_spp, "rows": rows}, open(args.out, "w"), indent=1)
    r.close()


def render(args):
    import cpugpupathtracing_amd as P
    s = many_light_scene()
    st = P.Settings(render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    r.upload(s)
    r.set_tuning(pools=1)
    r.set_nee_candidates(args.m)
    for seed in (1, 2):
        r.reset_accumulator(); r.reset_stats()
        r.render(W, H, SPP, seed=seed, kernel=P.KERNEL_WAVEFRONT, settings=st)
    print(f"M {args.m}: {r.stats().kernel_ms:.2f} ms with one pool")
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("ab"); a.add_argument("--parent-lib", required=True); a.add_argument("--pairs", type=int, default=2)
    a.add_argument("--steps", type=int, default=5); a.add_argument("--warmup", type=int, default=2); a.add_argument("--out")
    b = sub.add_parser("lights"); b.add_argument("--reps", type=int, default=3); b.add_argument("--ref-spp", type=int, default=16384); b.add_argument("--out")
    c = sub.add_parser("render"); c.add_argument("--m", type=int, default=1)
    args = ap.parse_args()
    {"ab": ab, "lights": lights, "render": render}[args.cmd](args)
