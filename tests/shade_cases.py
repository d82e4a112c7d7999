"""The sample sets of the shade-step tests (test_shade_reference.py, test_gpu_shade_step.py): each call is one cgpt_shade_samples batch --
a ModelScene, the settings, the NEE candidate count and the sample records -- built from fixed seeds.  evaluate() runs the model of
tests/shade_ref.py on a call once (float64, float32, and the float64 evaluations of an undecided sample's other branches) and keeps it.

Hits are built by hand on a plane, a sphere or a triangle so that the incoming direction is exact: cosines 1, 0.5, 1e-2, 1e-4, 1e-8 and
1e-20 against the normal (0, 0, +-1), from both sides; from 1e-4 down the direction is (1, 0, -+c), a unit vector in float32 whose
cosine is exactly c.  The hits on the icosphere (normals) come from smooth_ref.intersect_mesh / transform_ref.model_intersect in float64,
rounded to float32: a hit record is an input of the shade step, and this way the CPU tests see the very samples the GPU tests run.
"""
from __future__ import annotations

import numpy as np

import shade_ref as S
import smooth_ref as SM
import transform_ref as TR

COSINES = (1.0, 0.5, 1e-2, 1e-4, 1e-8, 1e-20)
TILTED = np.array([0.36, -0.48, 0.8])                                          # a unit vector in float64; float32 rounds it
WHITE_LIGHT = dict(emissive=(1.0, 0.9, 0.8), intensity=10.0, is_light=True)
_evaluated = {}


def _seeds(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def _tangent(n):
    t = np.cross(n, (0.0, 0.0, 1.0) if abs(n[2]) < 0.9 else (1.0, 0.0, 0.0))
    return t / np.linalg.norm(t)


def direction(normal, c, side):
    """A float32 direction meeting `normal` at cosine c from its front (side = +1) or its back (-1)."""
    n = np.asarray(normal, np.float64)
    axis = abs(abs(n[2]) - 1.0) < 1e-12
    if axis and c <= 1e-4:
        return np.array([1.0, 0.0, -side * c * np.sign(n[2])], np.float32)
    t = np.array([1.0, 0.0, 0.0]) if axis else _tangent(n)
    return (np.sqrt(max(0.0, 1.0 - c * c)) * t - side * c * n).astype(np.float32)


def hits(obj, normal, point, cosines=COSINES, sides=(1, -1), reps=8, seed=1, t=1.0, **state):
    """reps samples per (cosine, side) on object obj at `point` with the shading normal `normal`; state: throughput, depth, is_specular."""
    dirs = [direction(normal, c, s) for c in cosines for s in sides]
    a = S.samples(len(dirs) * reps)
    d = np.repeat(np.array(dirs, np.float32), reps, 0)
    a["d"], a["t"], a["obj"] = d, np.float32(t), obj
    a["o"] = np.asarray(point, np.float32) - d * np.float32(t)
    a["rng"] = _seeds(a.shape[0], seed)
    a["throughput"] = state.get("throughput", (1.0, 0.75, 0.5))
    a["depth"], a["is_specular"] = state.get("depth", 1), state.get("is_specular", 0)
    return a


def forced(a, k, words):
    """Copies of the samples a, one per word, whose k-th draw is that word."""
    out = []
    for w in words:
        b = a.copy()
        b["rng"] = S.state_with_draw(k, w & 0xFFFFFFFF)
        out.append(b)
    return np.concatenate(out)


def around(u):
    """Words either side of the float u: the neighbouring words (the same float32 or the next) and the neighbouring floats."""
    w = S.word_for_float(u)
    return [max(0, w - 512), max(0, w - 1), w, min(0xFFFFFFFF, w + 1), min(0xFFFFFFFF, w + 512)]


ENDS = (0, 0xFFFFFF80, 0xFFFFFFFF)                                             # random_float 0 and 1.0f (twice)


def call(name, scene, st, smp, candidates=1):
    return dict(name=name, scene=scene, settings=st, samples=smp, candidates=candidates)


# ---- 1. the reference's lobes, level 0 ----------------------------------------------------------------------------------------------------------
def _reference_scene(extra=None):
    sc = S.ModelScene()
    mats = dict(diffuse=sc.material(albedo=(0.8, 0.6, 0.4)), mirror=sc.material(albedo=(0.9, 0.9, 0.7), specular=1.0),
                half=sc.material(albedo=(0.7, 0.7, 0.2), specular=0.5),
                glass=sc.material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517),
                mixed=sc.material(albedo=(0.05, 0.6, 0.3), specular=0.3, refractivity=0.4, absorption=(0.1, 0.2, 0.3), ior=1.517),
                light=sc.material(**WHITE_LIGHT))
    objs = {}
    for m in ("diffuse", "mirror", "half", "glass", "mixed"):
        objs[m, "up"] = sc.plane((0, 0, 1), (0, 0, 0), mats[m])
        objs[m, "down"] = sc.plane((0, 0, -1), (0, 0, 0), mats[m])
        objs[m, "tilted"] = sc.plane(TILTED, (0, 0, 0), mats[m])
    objs["sphere"] = sc.sphere((0.5, 0.25, -1.0), 1.0, mats["glass"])
    objs["sphere_diffuse"] = sc.sphere((0.5, 0.25, -1.0), 1.0, mats["diffuse"])
    quad = np.array([[-2, -2, 0, 0, 0, 1], [2, -2, 0, 0, 0, 1], [2, 2, 0, 0, 0, 1], [-2, 2, 0, 0, 0, 1]], np.float32)
    objs["mesh"] = sc.mesh(quad, [0, 1, 2, 2, 3, 0], mats["half"])
    objs["light"] = sc.sphere((1.0, -2.0, 6.0), 1.5, mats["light"], light=True)
    objs["triangle"] = sc.triangle([[-2, -2, 0], [2, -2, 0], [0, 3, 0]], (0, 0, 1), mats["mixed"])
    if extra:
        extra(sc)
    return sc, mats, objs


def _reference_samples(objs):
    parts, seed = [], 100
    for m in ("diffuse", "mirror", "half", "glass", "mixed"):
        for which, n in (("up", (0, 0, 1)), ("down", (0, 0, -1)), ("tilted", TILTED)):
            seed += 1
            parts.append(hits(objs[m, which], n, (0.25, -0.5, 0.0) if which != "tilted" else (0, 0, 0), COSINES if which != "tilted" else COSINES[:3], reps=8, seed=seed, t=1.5))
    # the spheres: the hit point is wherever o + d t lands; the normal is computed from it (rays through and past the centre line)
    for key in ("sphere", "sphere_diffuse"):
        a = S.samples(96)
        rng = np.random.default_rng(7)
        p = rng.standard_normal((96, 3)); p /= np.linalg.norm(p, axis=1, keepdims=True)
        d = rng.standard_normal((96, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        a["d"], a["t"], a["obj"] = d, 2.0, objs[key]
        a["o"] = (np.array([0.5, 0.25, -1.0]) + p - 2.0 * d).astype(np.float32)
        a["rng"], a["depth"], a["throughput"] = _seeds(96, 8), 2, (0.5, 1.0, 0.25)
        parts.append(a)
    b = hits(objs["mesh"], (0, 0, 1), (0.5, 0.5, 0.0), reps=6, seed=9)
    b["tri"] = np.arange(b.shape[0]) % 2
    parts.append(b)
    b = hits(objs["triangle"], (0, 0, 1), (0.25, 0.5, 0.0), reps=6, seed=10)
    b["tri"] = np.arange(b.shape[0]) * 7919                                   # a triangle object ignores tri (get_hit): whatever an earlier mesh left
    parts.append(b)
    return np.concatenate(parts)


def reference_lobes():
    sc, mats, objs = _reference_scene()
    base = _reference_samples(objs)
    calls = []
    for cosine in (True, False):
        for rr in (True, False):
            calls.append(call(f"lobes_cosine{int(cosine)}_rr{int(rr)}", sc, S.settings(cosine=cosine, rr=rr, nee=True), base))
    # forced draws, NEE off so that the draw order is fixed: roulette (rr on: draw 0), r (draw 1 / 0), Fresnel (draw 2 / 1)
    few = np.concatenate([hits(objs[m, w], n, (0, 0, 0), (1.0, 0.5, 1e-2), reps=1, seed=11) for m in ("half", "glass", "mixed", "diffuse")
                          for w, n in (("up", (0, 0, 1)), ("tilted", TILTED))])
    on = np.concatenate([forced(few, 0, ENDS + tuple(around(0.7)) + tuple(around(0.6))), forced(few, 1, ENDS + tuple(around(0.5)) + tuple(around(0.3)) + tuple(around(0.7))),
                         forced(few, 2, ENDS)])
    off = np.concatenate([forced(few, 0, ENDS + tuple(around(0.5)) + tuple(around(0.3)) + tuple(around(0.7))), forced(few, 1, ENDS)])
    calls.append(call("lobes_forced_rr1", sc, S.settings(nee=False, rr=True), on))
    calls.append(call("lobes_forced_rr0", sc, S.settings(nee=False, rr=False, cosine=False), off))
    return calls


# ---- 2. the state rules -------------------------------------------------------------------------------------------------------------------------
def state_rules():
    sc, mats, objs = _reference_scene()
    light_plane = sc.plane((0, 0, 1), (0, 0, 0), mats["light"])
    calls = []
    few = np.concatenate([hits(objs[m, "up"], (0, 0, 1), (0, 0, 0), (1.0, 0.5), reps=4, seed=21) for m in ("diffuse", "half", "glass", "mixed")])
    for maxd in (0, 1, 5):
        parts = []
        for depth in sorted({0, max(0, maxd - 1), maxd}):
            a = few.copy(); a["depth"] = depth
            parts.append(a)
        calls.append(call(f"state_depth_max{maxd}", sc, S.settings(max_ray_depth=maxd), np.concatenate(parts)))
    for nee in (True, False):
        parts = []
        for depth in (0, 2):
            for spec in (0, 1):
                a = hits(light_plane, (0, 0, 1), (0, 0, 0), (1.0, 0.5, 1e-8), reps=2, seed=22, depth=depth, is_specular=spec)
                parts.append(a)
        miss = hits(0, (0, 0, 1), (0, 0, 0), (0.5,), reps=4, seed=23)
        miss["obj"], miss["t"] = S.NO_HIT, 1e34
        parts.append(miss)
        calls.append(call(f"state_light_nee{int(nee)}", sc, S.settings(nee=nee), np.concatenate(parts)))
    view = np.concatenate([few.copy(), few.copy()])
    view["depth"][:few.shape[0]] = 0
    view["bvh_depth"] = np.arange(view.shape[0]) % 45
    view["obj"][::5] = S.NO_HIT
    calls.append(call("state_bvh_view", sc, S.settings(debug_mode=2), view))
    return calls


# ---- 3. stuck total internal reflection -----------------------------------------------------------------------------------------------------------
def stuck_tir():
    sc = S.ModelScene()
    glass = sc.material(albedo=(0.9, 0.8, 0.7), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517)
    mixed = sc.material(albedo=(0.9, 0.5, 0.7), specular=0.2, refractivity=0.7, absorption=(0.1, 0.2, 0.3), ior=1.517)
    dim = sc.material(albedo=(0.3, 0.2, 0.25), specular=0.1, refractivity=0.85, ior=2.4)
    planes = [sc.plane((0, 0, 1), (0, 0, 0), m) for m in (glass, mixed, dim)]
    sc.sphere((0, 0, 5), 1.0, sc.material(**WHITE_LIGHT), light=True)
    calls = []
    for rr in (True, False):
        for maxd in (5, 12):
            parts = []
            for k, pl in enumerate(planes):
                for depth in range(0, maxd + 1, 2 if maxd > 5 else 1):
                    # from inside (side -1): cos 0.5 and 0.2 are beyond the critical angle of 1.517 and 2.4, 0.9 is not
                    parts.append(hits(pl, (0, 0, 1), (0, 0, 0), (0.5, 0.2, 0.9), sides=(-1,), reps=6, seed=31 + k + 7 * depth, depth=depth, t=0.75))
            calls.append(call(f"stuck_rr{int(rr)}_max{maxd}", sc, S.settings(max_ray_depth=maxd, rr=rr, nee=False), np.concatenate(parts)))
    return calls


# ---- 4. GGX reflection, level 1 -------------------------------------------------------------------------------------------------------------------
ROUGHNESS = (1e-3, 0.05, 0.5, 1.0)


ORDINARY, GRAZING = COSINES[:3], COSINES[3:]
REPS = 48                                # samples per (object, cosine, side) in the rough cases: one number for every call


def ggx():
    """Per roughness: the ordinary cosines on (0, 0, +-1) and, from 0.9 down, on the tilted normal; cosine 1 on the tilted normal (a call of
    its own: the visible-normal sample's tangent is rounding noise at normal incidence on a normal that is no axis); the grazing cosines;
    the forced draws.  A tolerance is a call's largest float32 deviation, so the ranges that condition differently are calls of their own."""
    calls = []
    st = S.settings(rr=False)                                                  # r is draw 0, u1 draw 1, u2 draw 2 (diffuse weight 0: no NEE draw)
    for k, r in enumerate(ROUGHNESS):
        sc = S.ModelScene()
        m = sc.material(albedo=(0.9, 0.7, 0.5), specular=1.0, roughness=r)
        planes = [(sc.plane(n, (0, 0, 0), m), n, w) for w, n in (("up", (0, 0, 1)), ("down", (0, 0, -1)), ("tilted", TILTED))]
        sc.sphere((0, 0, 5), 1.0, sc.material(**WHITE_LIGHT), light=True)
        axis, (to, tn, _) = planes[:2], planes[2]
        ordinary = [hits(o, n, (0, 0, 0), ORDINARY if w != "tilted" else (0.9, 0.5, 1e-2), reps=REPS, seed=41 + 3 * k + j) for j, (o, n, w) in enumerate(planes)]
        grazing = [hits(o, n, (0, 0, 0), GRAZING, reps=REPS, seed=51 + 3 * k + j) for j, (o, n, w) in enumerate(axis)]
        edge = np.concatenate([hits(o, n, (0, 0, 0), COSINES if w != "tilted" else ORDINARY, reps=1, seed=61 + 3 * k + j) for j, (o, n, w) in enumerate(planes)])
        calls.append(call(f"ggx_r{r}_ordinary", sc, st, np.concatenate(ordinary)))
        calls.append(call(f"ggx_r{r}_tilted_normal_incidence", sc, st, hits(to, tn, (0, 0, 0), (1.0,), reps=REPS, seed=57 + k)))
        calls.append(call(f"ggx_r{r}_grazing", sc, st, np.concatenate(grazing)))
        calls.append(call(f"ggx_r{r}_forced", sc, st, np.concatenate([forced(edge, 1, ENDS), forced(edge, 2, ENDS)])))
    return calls


# ---- 5. rough glass, level 2 ------------------------------------------------------------------------------------------------------------------------
IORS = (1.0, 1.517, 2.4)


def rough_glass():
    """Per transmission roughness: the ordinary cosines at every ior, with both sides of the macro-normal's
    critical angle from inside; the grazing cosines at ior 1.517 and 2.4; ior 1.0 from cosine 1e-2 down (a call of its own: k = 1 - (1 - c^2) is a cancellation there -- 1e-4 at
    c = 1e-2, the margin itself -- and the refracted ray's cosine, the Smith term's argument, the difference of two nearly equal numbers);
    the forced Fresnel draw."""
    calls = []
    st = S.settings(rr=False)                                                  # r draw 0, u1 1, u2 2, the Fresnel float 3 (where k >= 0)
    for j, r in enumerate(ROUGHNESS):
        sc = S.ModelScene()
        parts, edge, low, graze = [], [], [], []
        for k, ior in enumerate(IORS):
            m = sc.material(albedo=(0.95, 0.9, 0.85), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=ior, transmission_roughness=r)
            o = sc.plane((0, 0, 1), (0, 0, 0), m)
            crit = np.sqrt(max(0.0, 1.0 - 1.0 / (ior * ior)))                # the macro-normal's critical cosine from inside
            inside = tuple(c for c in (crit + 0.02, crit - 0.02) if 0.0 < c < 1.0)
            if ior == 1.0:
                parts.append(hits(o, (0, 0, 1), (0, 0, 0), (1.0, 0.5, 0.05), reps=REPS, seed=71 + 3 * j + k, t=2.0))
                low.append(hits(o, (0, 0, 1), (0, 0, 0), COSINES[2:], reps=REPS, seed=81 + 3 * j + k, t=2.0))
            else:
                parts.append(hits(o, (0, 0, 1), (0, 0, 0), ORDINARY, reps=REPS, seed=71 + 3 * j + k, t=2.0))
                graze.append(hits(o, (0, 0, 1), (0, 0, 0), GRAZING, reps=REPS, seed=76 + 3 * j + k, t=2.0))
                parts.append(hits(o, (0, 0, 1), (0, 0, 0), inside, sides=(-1,), reps=REPS, seed=91 + 3 * j + k, t=2.0))
            edge.append(hits(o, (0, 0, 1), (0, 0, 0), (1.0, 0.5, 0.05) + inside, reps=1, seed=111 + 3 * j + k, t=2.0))
        sc.sphere((0, 0, 5), 1.0, sc.material(**WHITE_LIGHT), light=True)
        calls.append(call(f"rough_glass_r{r}", sc, st, np.concatenate(parts)))
        calls.append(call(f"rough_glass_r{r}_grazing", sc, st, np.concatenate(graze)))
        calls.append(call(f"rough_glass_r{r}_ior1_grazing", sc, st, np.concatenate(low)))
        calls.append(call(f"rough_glass_r{r}_forced", sc, st, forced(np.concatenate(edge), 3, ENDS)))
    return calls


# ---- 6. NEE and RIS ---------------------------------------------------------------------------------------------------------------------------------
def _light_quad(z, x0, size):
    return np.array([[x0, -size, z, 0, 0, -1], [x0, size, z, 0, 0, -1], [x0 + 2 * size, size, z, 0, 0, -1], [x0 + 2 * size, -size, z, 0, 0, -1]], np.float32), [0, 1, 2, 2, 3, 0]


def _nee_scene(which):
    sc = S.ModelScene()
    floor = sc.plane((0, 0, 1), (0, 0, 0), sc.material(albedo=(0.9, 0.7, 0.5), specular=0.25))
    bright, faint = sc.material(emissive=(1.0, 0.9, 0.8), intensity=30.0, is_light=True), sc.material(emissive=(0.2, 0.5, 1.0), intensity=0.05, is_light=True)
    if which == "sphere":
        sc.sphere((1.0, -2.0, 6.0), 1.5, bright, light=True)
    elif which == "sphere_mesh":
        sc.sphere((1.0, -2.0, 6.0), 1.5, faint, light=True)
        sc.mesh(*_light_quad(4.0, -3.0, 1.0), bright, light=True)
    elif which == "below_above":
        sc.sphere((0.0, 1.0, -4.0), 1.0, bright, light=True)
        sc.sphere((1.0, -2.0, 6.0), 1.5, faint, light=True)
    elif which == "all_below":
        sc.sphere((0.0, 1.0, -4.0), 1.0, bright, light=True)
        sc.mesh(*_light_quad(-3.0, -1.0, 1.0), faint, light=True)
    else:                                                                     # two mesh lights: five draws a candidate, so the reservoir draw can be forced
        sc.mesh(*_light_quad(4.0, -3.0, 1.0), bright, light=True)
        sc.mesh(*_light_quad(5.0, 2.0, 0.5), faint, light=True)
    return sc, floor


def nee_ris():
    calls = []
    for which in ("sphere", "sphere_mesh", "below_above", "all_below", "two_meshes"):
        sc, floor = _nee_scene(which)
        rng = np.random.default_rng(5)
        a = hits(floor, (0, 0, 1), (0, 0, 0), (1.0, 0.5, 1e-2), sides=(1,), reps=40, seed=131)
        shift = np.zeros((a.shape[0], 3), np.float32); shift[:, :2] = rng.uniform(-1.5, 1.5, (a.shape[0], 2))
        a["o"] += shift
        for M in (1, 2, 32):
            smp = a
            if which == "two_meshes" and M > 1:
                few = a[::12]
                smp = np.concatenate([a, forced(few, 4, ENDS), forced(few, 5 * M - 1, ENDS)])
            calls.append(call(f"nee_{which}_M{M}", sc, S.settings(rr=True), smp, M))
    return calls


# ---- 7. normals, levels 3 and 4 ---------------------------------------------------------------------------------------------------------------------
NORMAL_TRANSFORMS = {
    "plain": None,
    "rotated_scaled": TR.affine(TR.rotation((0.3, 1.0, -0.2), 0.7) @ np.diag([1.5, 0.75, 1.25]), (0.4, -0.3, 0.2)),
    "mirrored": TR.affine(np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 0.5)),
}


def normals():
    calls = []
    center, radius = np.array(SM.SPHERE_CENTER), SM.SPHERE_RADIUS
    for name, m in NORMAL_TRANSFORMS.items():
        sc = S.ModelScene()
        diffuse, glossy = sc.material(albedo=(0.8, 0.6, 0.4)), sc.material(albedo=(0.9, 0.7, 0.5), specular=1.0, roughness=0.3)
        mesh = SM.icosphere(SM.SPHERE_LEVEL, SM.SPHERE_CENTER, SM.SPHERE_RADIUS)
        objs = [sc.mesh(*mesh, mat, smooth=True, transform=m) for mat in (diffuse, glossy)]
        sc.sphere((2.0, 9.0, 3.0), 1.5, sc.material(**WHITE_LIGHT), light=True)
        rows = sc.objects[objs[0]]["rows"]
        M34 = np.array(TR.IDENTITY if m is None else m, np.float64).reshape(3, 4)
        rng = np.random.default_rng(17)
        n = 600
        # object-space rays: from outside towards the sphere, from inside outwards, and grazing the silhouette
        tgt = rng.standard_normal((n, 3)); tgt /= np.linalg.norm(tgt, axis=1, keepdims=True)
        scale = np.concatenate([rng.uniform(0.0, 0.9, n // 3), rng.uniform(0.0, 0.5, n // 3), rng.uniform(0.93, 0.999, n - 2 * (n // 3))])
        org = rng.standard_normal((n, 3)); org /= np.linalg.norm(org, axis=1, keepdims=True)
        org = center + org * np.where(np.arange(n) // (n // 3) == 1, 0.3 * radius, 4.0 * radius)[:, None]
        aim = center + tgt * (scale * radius)[:, None]
        o_w = org @ M34[:, :3].T + M34[:, 3]
        d_w = (aim - org) @ M34[:, :3].T
        d_w /= np.linalg.norm(d_w, axis=1, keepdims=True)
        o32, d32 = o_w.astype(np.float32), d_w.astype(np.float32)
        t, tri = TR.model_intersect(rows, TR.IDENTITY if m is None else m, o32, d32)
        hit = tri >= 0
        a = S.samples(int(hit.sum()))
        a["o"], a["d"], a["t"], a["tri"] = o32[hit], d32[hit], t[hit].astype(np.float32), tri[hit]
        a["obj"] = np.where(np.arange(a.shape[0]) % 2 == 0, objs[0], objs[1])
        a["rng"], a["depth"] = _seeds(a.shape[0], 151), 1
        calls.append(call(f"normals_{name}", sc, S.settings(rr=False), a))
    return calls


# Calls whose undecided share (ill-conditioned samples included) is above the 2 % cap, each with its cause.  Every sample of such a call still
# runs on the device and is checked by the rule of its kind (test_gpu_shade_step.py); test_shade_reference.py asserts the cap for every other
# call and that each entry here is still needed.
CAP_EXCEPTIONS = (
    (r"lobes_forced_rr[01]$", "the probes sit within 512 words of specular + refractivity, a float32 sum that float64 rounds differently: undecided by construction"),
    (r"ggx_r.*_tilted_normal_incidence$", "normal incidence on a normal that is no axis: (ox, oy) is rounding noise and the tangent t1 normalises it"),
    (r"ggx_r0\.001_grazing$", "a near-mirror sends a grazing ray out grazing: the outgoing cosine, tested against 0 and fed to the Smith term, is below the margin"),
    (r"ggx_r.*_forced$", "u1 = 1.0f puts the point on the rim of the projected disc, where 1 - p1^2 - p2^2 cancels and the unstretched normal is short"),
    (r"rough_glass_r0\.001_grazing$", "as ggx_r0.001_grazing: the reflected and the refracted cosine of a near-polished interface at grazing incidence"),
    (r"rough_glass_r.*_ior1_grazing$", "ior 1.0: k = 1 - (1 - c^2) cancels (1e-4 at c = 1e-2) and the ray leaves at the incoming grazing angle"),
    (r"rough_glass_r.*_forced$", "at ior 1.0 the Fresnel term is 0 and the forced draw 0 ties with it"),
    (r"nee_(sphere|below_above)_M32$", "32 candidates a sample, each with a ball rejection, two cosine tests and a reservoir test: about a hundred comparisons on one path"),
)


def cap_exception(name):
    import re
    return next((cause for pat, cause in CAP_EXCEPTIONS if re.search(pat, name)), None)


CASES = dict(reference_lobes=reference_lobes, state_rules=state_rules, stuck_tir=stuck_tir, ggx=ggx, rough_glass=rough_glass, nee_ris=nee_ris,
             normals=normals)
_calls = {}


def calls_of(case):
    if case not in _calls:
        _calls[case] = CASES[case]()
    return _calls[case]


def all_calls():
    return [(case, c) for case in CASES for c in calls_of(case)]


def evaluate(c):
    """The model's evaluations of a call, computed once: m64, m32, the tolerances, the kept (decided) samples and the float64
    evaluations of the other branches of the undecided ones."""
    key = c["name"]
    if key not in _evaluated:
        sc = c["scene"]
        if "_device_scene" not in c:
            c["_device_scene"] = sc.device_scene()                             # also records the mesh lights' total_area
        kw = dict(candidates=c["candidates"])
        m64 = S.shade(sc, c["settings"], c["samples"], np.float64, **kw)
        m32 = S.shade(sc, c["settings"], c["samples"], np.float32, **kw)
        tol, keep = S.tolerances(m32, m64)
        others = []
        und = m64["undecided"]
        if und.any():
            sub = c["samples"][und]
            others = [S.shade(sc, c["settings"], sub, np.float64, flip=f, **kw) for f in (1, 2, 3)]
        _evaluated[key] = dict(m64=m64, m32=m32, tol=tol, keep=keep, others=others)
    return _evaluated[key]
