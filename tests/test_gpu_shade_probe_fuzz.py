"""Randomised check of the shade kernel's probe (wf_shade: "Probe"): random small scenes -- meshes of several sizes and build options
(leaf roots, roots with leaf children, deep trees), spheres, planes, triangle objects, sphere and mesh lights, in random object order and
number (below and above probe_max_objects) -- random cameras, frame sizes (not multiples of the tile), settings, render modes and tuning
knobs.  Every case renders the wavefront pipeline with probe 1 and with probe 0 and the persistent kernel: accumulators and packed pixels
bit-identical, traced_rays equal, probe_resolved 0 with the knob off and never more than the rays after the primaries.  Every generated
case is compared.  CGPT_FUZZ_CASES / CGPT_FUZZ_SEED widen the run (default: 40 cases, seed 1; a failing case prints its parameters)."""
import os

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from scenes import GROUND_I, GROUND_V, standin_mesh

pytestmark = pytest.mark.gpu


def _quad(rng):
    c = rng.uniform(-4, 4, 3)
    a, b = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
    n = np.cross(a, b); n = n / max(1e-6, np.linalg.norm(n))
    v = np.array([np.concatenate([c + sa * a + sb * b, n]) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))], np.float32)
    return v, GROUND_I


def _random_scene(rng, meshes):
    s = P.Scene()
    mats = []
    for _ in range(int(rng.integers(2, 6))):
        kind = int(rng.integers(0, 5))
        alb = tuple(rng.uniform(0.2, 0.95, 3))
        m = [P.Material(albedo=alb), P.Material(albedo=alb, specular=float(rng.uniform(0.2, 0.8))), P.Material(albedo=alb, specular=1.0),
             P.Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517),
             P.Material(albedo=alb, specular=0.3, refractivity=0.3, ior=1.3)][kind]
        mats.append(s.add_material(m))
    light_mat = s.add_material(P.Material(emissive=(1.0, 0.9, 0.8), intensity=float(rng.uniform(3, 12)), is_light=True))
    n_objects = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 9, 12]))
    lights, kinds = [], []
    for k in range(n_objects):
        kind = rng.choice(["mesh", "mesh", "ground", "quad", "quads", "sphere", "sphere", "plane", "triangle", "sphere_light", "mesh_light"])
        mat = int(rng.choice(mats))
        if kind == "mesh":
            v, i = meshes[int(rng.integers(0, len(meshes)))]
            scale = float(rng.uniform(0.3, 1.2))
            v = v * np.array([scale] * 3 + [1] * 3, np.float32) + np.concatenate([rng.uniform(-3, 3, 3), np.zeros(3)]).astype(np.float32)
            s.add_mesh(P.Mesh.from_arrays(v, i), mat, int(rng.choice([P.BUILD_NAIVE, P.BUILD_SAH_INTERVALS, P.BUILD_SAH_PRIMITIVES])))
        elif kind == "ground":
            s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), mat, P.BUILD_SAH_INTERVALS)
        elif kind == "quad":                                         # a leaf root
            s.add_mesh(P.Mesh.from_arrays(*_quad(rng)), mat, P.BUILD_SAH_INTERVALS)
        elif kind == "quads":                                        # a few quads far apart: a root with leaf children, or a shallow tree
            parts = [_quad(rng) for _ in range(int(rng.integers(2, 5)))]
            v = np.vstack([q[0] + np.array([20.0 * j, 0, 0, 0, 0, 0], np.float32) for j, q in enumerate(parts)])
            i = np.concatenate([q[1] + 4 * j for j, q in enumerate(parts)]).astype(np.uint32)
            s.add_mesh(P.Mesh.from_arrays(v, i), mat, int(rng.choice([P.BUILD_NAIVE, P.BUILD_SAH_INTERVALS, P.BUILD_SAH_PRIMITIVES])))
        elif kind == "sphere":
            s.add_sphere(tuple(rng.uniform(-5, 5, 3)), float(rng.uniform(0.3, 2.5)), mat)
        elif kind == "plane":
            n = rng.normal(0, 1, 3) + (0, 1.5, 0)
            s.add_plane(tuple(n / np.linalg.norm(n)), (0.0, float(rng.uniform(-5, -2)), 0.0), mat)
        elif kind == "triangle":
            p = rng.uniform(-4, 4, (3, 3)).astype(np.float32)
            n = rng.normal(0, 1, 3); n = (n / np.linalg.norm(n)).astype(np.float32)
            s.add_triangle(p, np.tile(n, (3, 1)), mat)
        elif kind == "sphere_light":
            lights.append(s.add_sphere(tuple(rng.uniform(-10, 10, 3) + (0, 8, 0)), float(rng.uniform(1, 5)), light_mat))
        else:
            v, i = _quad(rng)
            v = v + np.array([0, 9, 0, 0, 0, 0], np.float32)
            lights.append(s.add_mesh(P.Mesh.from_arrays(v, i), light_mat, P.BUILD_SAH_INTERVALS))
        kinds.append(str(kind))
    for li in lights:
        s.add_light(li)
    return s, kinds


def test_random_scenes_and_knobs_probe_on_off_and_persistent():
    cases = int(os.environ.get("CGPT_FUZZ_CASES", "40"))
    rng = np.random.default_rng(int(os.environ.get("CGPT_FUZZ_SEED", "1")))
    meshes = [standin_mesh(lv) for lv in (0, 1, 2, 3)]
    n_resolved = 0
    for case in range(cases):
        s, kinds = _random_scene(rng, meshes)
        W, H = int(rng.integers(9, 130)), int(rng.integers(5, 90))
        spp = int(rng.choice([1, 2, 3, 5, 8, 13, 33]))
        first = int(rng.choice([0, 0, 3]))
        seed = int(rng.integers(0, 2 ** 31))
        mode = int(rng.choice([P.MODE_ADVANCED] * 4 + [P.MODE_BRUTE_FORCE, P.MODE_COMPARISON]))
        debug = int(rng.choice([P.DEBUG_NONE] * 6 + [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH]))
        st = P.Settings(max_ray_depth=int(rng.choice([0, 1, 3, 5, 7])), next_event_estimation_enabled=bool(rng.random() < 0.8),
                        cosine_weighted_diffuse_reflection_enabled=bool(rng.random() < 0.7), russian_roulette_enabled=bool(rng.random() < 0.7),
                        render_mode=mode, debug_render_mode=debug)
        pos = rng.uniform(-6, 6, 3) + (0, 2, 8)
        view = -pos + rng.uniform(-1, 1, 3)
        if rng.random() < 0.2:                                       # now and then an axis-parallel centre ray
            W, H = W + (W & 1), H + (H & 1)
            view = np.array([(0, 0, -1), (0, -1, 0), (1, 0, 0)][int(rng.integers(0, 3))], np.float64)
        s.set_camera(tuple(pos), tuple(view / np.linalg.norm(view)), float(rng.uniform(30, 90)), W / H)
        s.set_settings(st)
        knobs = {}
        for pick in rng.choice(7, size=int(rng.integers(0, 4)), replace=False):
            knobs.update([{"batch": int(rng.integers(1, 9))}, {"path_order": int(rng.integers(0, 3))}, {"retire_misses": 0}, {"pools": int(rng.integers(1, 4))},
                          {"bands": int(rng.integers(2, 33)), "bands_min_paths": 0}, {"spec_dedupe": 0}, {"probe_max_objects": int(rng.integers(0, 13))}][int(pick)])
        desc = (f"case {case}: objects {kinds} {W}x{H} spp {spp} first {first} seed {seed} mode {mode} debug {debug} depth {st.max_ray_depth} "
                f"nee {st.next_event_estimation_enabled} cos {st.cosine_weighted_diffuse_reflection_enabled} rr {st.russian_roulette_enabled} knobs {knobs}")
        results = {}
        for name, k, kn in (("pers", P.KERNEL_PERSISTENT, {}), ("probe0", P.KERNEL_WAVEFRONT, {**knobs, "probe": 0}), ("probe1", P.KERNEL_WAVEFRONT, {**knobs, "probe": 1})):
            r = P.Renderer(0)
            try:
                r.upload(s)
                if kn:
                    r.set_tuning(**kn)
                if first:
                    r.render(W, H, first, seed=seed, kernel=P.KERNEL_MEGAKERNEL)
                r.reset_stats()
                r.render(W, H, spp, seed=seed, kernel=k)
                stats = r.stats()
                results[name] = (r.accumulator().copy(), r.pixels().copy(), stats.traced_rays, stats.probe_resolved)
            finally:
                r.close()
        ref = results["pers"]
        for name, (acc, px, rays, resolved) in results.items():
            if not np.array_equal(acc.view(np.uint32), ref[0].view(np.uint32)) or not np.array_equal(px, ref[1]) or rays != ref[2]:
                bad = np.argwhere((acc.view(np.uint32) != ref[0].view(np.uint32)).any(axis=-1))
                print("MISMATCH", name, desc, "rays", rays, ref[2], "first bad pixels", bad[:5].tolist(), flush=True)
                raise AssertionError("probe changes a result: " + desc)
            assert resolved <= rays - W * H * spp, desc
            if name != "probe1" or debug != P.DEBUG_NONE or mode == P.MODE_BRUTE_FORCE or len(kinds) > knobs.get("probe_max_objects", 128):
                assert resolved == 0, (name, desc)
        n_resolved += results["probe1"][3] > 0
    print(f"all {cases} cases ok, {n_resolved} with decided rays")
    assert n_resolved > 0 or cases < 10
