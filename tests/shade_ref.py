"""One shade_bounce call (csrc/device/shade_device.hpp; ref: Source/Main.cpp:404-573) stated in numpy with the float type as a parameter, for
the tests of cgpt_shade_samples.  The float64 evaluation is the reference; the float32 evaluation of the same statement gives the scale of
every tolerance (tolerances()).  Nothing here comes from the device.

What is modelled exactly: the RNG (integer), the order of the draws, every discrete outcome.  What is modelled in `dtype`: every float
operation, in the device's order where the order is visible (dot and cross as (a.x b.x + a.y b.y) + a.z b.z, normalize as a multiplication by
1 / sqrt, the constants kPi = 3.14159265f, kInvPi = 1 / kPi and kNudge = 0.001f as the float32 values the device holds).  The float32
evaluation is not meant to be the device's bits: numpy's sin / cos / exp and the pieces taken from the other reference modules round
differently by a few ulps, which is what the factor of tolerances() covers.

Pieces taken from the project's other statements: smooth_ref.smooth_normal (the interpolated normal and its side rules),
transform_ref.invert / ray_to_object / normal_to_world (a transformed object's ray and normal), rough_glass_ref._visible_normals (the
visible-normal sample in the local frame) and rough_glass_ref.facet_fresnel (the reference's fresnel() at an interface, used for the smooth
and the rough dielectric alike).  The light candidate and the reservoir are written out here (Reservoir below): ris_ref.draw_candidate /
Reservoir and integrator_ref are float64 Monte Carlo over a floor whose normal is +y, drawn from a numpy generator, and state the same
steps for a distribution, not for given draws; test_shade_reference.py ties the two reservoirs together on common candidates, and the
reference's lobes to the C oracle.  glossy_ref.sample_vndf is the single-direction form of _visible_normals.

Decisions.  Every comparison whose two outcomes lead to different results goes through Eval.decide with its margin: the distance of the
two compared numbers relative to the larger of their magnitudes, or -- for a dot product compared with 0 -- relative to the sum of the
magnitudes of its three products (the scale of its rounding error).  A sample's margin is the smallest on its path; below MARGIN the sample
is undecided: float32 may take the other branch.  `flip` evaluates the other branches of such a sample (1: the first undecided comparison
inverted, 2: all of them, 3: all but the first), so that a test can accept any of them.  Continuous operations (clamp, max(0, x)) are no
decisions.  A dot product one of whose vectors was computed (a sampled or reflected direction, a sphere's or an interpolated normal) carries
that vector's own rounding error, so its scale is the product of the two lengths instead.

Conditioning.  Three normalisations follow a cancellation and amplify the rounding error of their operands by operand magnitude / length:
the visible-normal sample's tangent t1 from (ox, oy) (arbitrary at normal incidence on a normal that is no axis), its unstretched vector
(alpha nh.x, alpha nh.y, nh.z) (short when alpha is small and nh.z cancels) and the cosine-weighted direction normal + normalize(dir).
Eval.condition enters 1e-2 * length / magnitude into the margin: below a ratio of 1e-2 the vector has lost two of float32's seven digits
and what follows from it is no statement about the device's arithmetic.  Such a sample is `ill`: undecided, and not even one of the
model's branches -- only finiteness can be asked of the device there.  The same holds where a cosine whose sign is undecided goes on
into the Smith term (Eval.lost): 1 / z^2 of a number without digits.

The GGX horizon rule (shade_device.hpp: ggx_visible_normal): wo is at the horizon when oz = wo.n is not > 0 or oz^2 is below FLT_MIN,
the float32 constant, in either float type -- ggx_lambda's tan^2 would not be a float32 there.
"""
from __future__ import annotations

import numpy as np

import rough_glass_ref as RG
import smooth_ref as SM
import transform_ref as TR

MARGIN = 1e-4
NO_HIT = 0xFFFFFFFF
TERMINATE, SHADOW, ENERGY = 1, 2, 4
CHAIN_SHIFT, CHAIN_REFLECT, CHAIN_REFRACT, CHAIN_TIR = 4, 1, 2, 3
K_PI = np.float32(3.14159265)
K_INV_PI = np.float32(1.0) / K_PI
K_NUDGE = np.float32(0.001)
FLT_MIN = np.float32(1.17549435e-38)
GROUPS = ("d", "o", "throughput", "energy", "shadow_tmax", "pending")          # the float output groups a tolerance is derived for
FLOATS = {"d": ("d", "shadow_d"), "o": ("o", "shadow_o"), "throughput": ("throughput",), "energy": ("energy",), "shadow_tmax": ("shadow_tmax",),
          "pending": ("pending",)}
DISCRETE = ("flags", "rng", "depth", "is_specular", "unwalked")

_M32 = np.uint64(0xFFFFFFFF)
_MUL, _INC, _OUT = 747796405, 2891336453, 277803737
_MUL_INV, _OUT_INV = pow(_MUL, -1, 1 << 32), pow(_OUT, -1, 1 << 32)


# ---- the RNG: PCG-RXS-M-XS-32 (rt_device.hpp: pcg_next), integers ---------------------------------------------------------------------------
def pcg_next(state: int):
    """(word, next state) of one pcg_next on a Python int."""
    old = state & 0xFFFFFFFF
    new = (old * _MUL + _INC) & 0xFFFFFFFF
    w = (((old >> ((old >> 28) + 4)) ^ old) * _OUT) & 0xFFFFFFFF
    return (w >> 22) ^ w, new


def random_float(word):
    """random_float's value for a drawn word: float32(word) * float32(2.3283064365387e-10); 1.0f from 0xFFFFFF80 up."""
    return np.asarray(word, np.uint64).astype(np.float32) * np.float32(2.3283064365387e-10)


def word_for_float(u: float) -> int:
    """A word whose random_float is the float32 nearest to u (u in [0, 1])."""
    return min(0xFFFFFFFF, int(round(float(u) * 4294967296.0)))


def state_with_draw(k: int, word: int) -> int:
    """The PCG state whose k-th output (k = 0: the next one) is `word`: the output function is a bijection of the state."""
    w = (word ^ (word >> 22)) & 0xFFFFFFFF                                     # undo the >> 22 xorshift (22 >= 16: one step)
    x = (w * _OUT_INV) & 0xFFFFFFFF                                           # undo the multiplication
    s = (x >> 28) + 4                                                         # the top four bits are untouched by a shift of at least 4
    old = x
    for _ in range(8):                                                        # undo old ^ (old >> s): 8 * 4 >= 32 bits settle
        old = x ^ (old >> s)
    for _ in range(k):                                                        # step the LCG back
        old = ((old - _INC) * _MUL_INV) & 0xFFFFFFFF
    return old


# ---- the scene as the model and the device both get it ---------------------------------------------------------------------------------------
class ModelScene:
    """Materials, objects and lights once; device_scene() builds the cpugpupathtracing_amd.Scene, the model reads the same float32 data."""

    def __init__(self):
        self.materials, self.objects, self.lights = [], [], []

    def material(self, albedo=(0, 0, 0), specular=0.0, refractivity=0.0, absorption=(0, 0, 0), ior=1.0, emissive=(0, 0, 0), intensity=0.0,
                 is_light=False, roughness=0.0, transmission_roughness=0.0):
        self.materials.append(dict(albedo=albedo, specular=specular, refractivity=refractivity, absorption=absorption, ior=ior, emissive=emissive,
                                   intensity=intensity, is_light=is_light, roughness=roughness, transmission_roughness=transmission_roughness))
        return len(self.materials) - 1

    def plane(self, normal, point, mat):
        self.objects.append(dict(kind="plane", normal=np.asarray(normal, np.float32), point=np.asarray(point, np.float32), mat=mat))
        return len(self.objects) - 1

    def sphere(self, center, radius, mat, light=False):
        self.objects.append(dict(kind="sphere", center=np.asarray(center, np.float32), radius=np.float32(radius), mat=mat))
        if light:
            self.lights.append(len(self.objects) - 1)
        return len(self.objects) - 1

    def triangle(self, positions, normals, mat, smooth=False):
        p = np.asarray(positions, np.float32).reshape(3, 3)
        n = np.asarray(normals, np.float32)
        n = np.broadcast_to(n.reshape(3), (3, 3)) if n.size == 3 else n.reshape(3, 3)
        rows = np.concatenate([p, n], 1).reshape(1, 18).astype(np.float32)
        self.objects.append(dict(kind="triangle", rows=rows, mat=mat, smooth=smooth, transform=None, positions=p, normals=n))
        return len(self.objects) - 1

    def mesh(self, vertices, indices, mat, smooth=False, transform=None, light=False):
        v = np.ascontiguousarray(vertices, np.float32)
        i = np.ascontiguousarray(indices, np.uint32).ravel()
        self.objects.append(dict(kind="mesh", rows=SM.triangle_rows((v, i)), mat=mat, smooth=smooth, vertices=v, indices=i,
                                 transform=None if transform is None else np.ascontiguousarray(transform, np.float32).reshape(3, 4)))
        if light:
            self.lights.append(len(self.objects) - 1)
        return len(self.objects) - 1

    def lobe_level(self):
        """LobeLevel (csrc/device/kernel_variant.h)."""
        if any(o.get("transform") is not None and not TR.is_identity(o["transform"]) for o in self.objects):
            return 4
        if any(o.get("smooth") for o in self.objects):
            return 3
        if any(np.float32(m["transmission_roughness"]) > 0 for m in self.materials):
            return 2
        return 1 if any(np.float32(m["roughness"]) > 0 for m in self.materials) else 0

    def device_scene(self):
        """The cpugpupathtracing_amd.Scene of this description; records each mesh's total_area as the host library computes it."""
        import cpugpupathtracing_amd as P
        s = P.Scene()
        for m in self.materials:
            s.add_material(P.Material(**{k: (tuple(float(x) for x in v) if isinstance(v, (tuple, list, np.ndarray)) else v) for k, v in m.items()}))
        for o in self.objects:
            if o["kind"] == "plane":
                s.add_plane(o["normal"], o["point"], o["mat"])
            elif o["kind"] == "sphere":
                s.add_sphere(o["center"], float(o["radius"]), o["mat"])
            elif o["kind"] == "triangle":
                s.add_triangle(o["positions"], o["normals"], o["mat"], smooth=o["smooth"])
            else:
                mesh = P.Mesh.from_arrays(o["vertices"], o["indices"])
                k = s.add_mesh(mesh, o["mat"], smooth=o["smooth"], transform=o["transform"])
                o["total_area"] = np.float32(s.bvh_info(k).total_area)
        for l in self.lights:
            s.add_light(l)
        s.set_camera((0.0, 1.0, 5.0), (0.0, 0.0, -1.0), 60.0, 1.0)
        return s


    def oracle_scene(self):
        """The same description in the C oracle (planes, spheres and meshes with the reference's materials: no roughness, flag or transform)."""
        from oracle import OracleScene
        o = OracleScene()
        for m in self.materials:
            assert not m["roughness"] and not m["transmission_roughness"]
            o.add_material(**{k: v for k, v in m.items() if k not in ("roughness", "transmission_roughness")})
        for ob in self.objects:
            if ob["kind"] == "plane":
                o.add_plane(ob["normal"], ob["point"], ob["mat"])
            elif ob["kind"] == "sphere":
                o.add_sphere(ob["center"], float(ob["radius"]), ob["mat"])
            else:
                assert ob["kind"] == "mesh" and not ob["smooth"] and ob["transform"] is None
                o.add_mesh(ob["vertices"], ob["indices"], ob["mat"])
        for l in self.lights:
            o.add_light(l)
        return o


def settings(max_ray_depth=5, nee=True, cosine=True, rr=True, debug_mode=0):
    return dict(max_ray_depth=max_ray_depth, nee=nee, cosine=cosine, rr=rr, debug_mode=debug_mode)


def device_settings(st):
    import cpugpupathtracing_amd as P
    return P.Settings(max_ray_depth=st["max_ray_depth"], next_event_estimation_enabled=st["nee"],
                      cosine_weighted_diffuse_reflection_enabled=st["cosine"], russian_roulette_enabled=st["rr"], debug_render_mode=st["debug_mode"])


def samples(n):
    """n cgpt_shade_sample records as a numpy record array (the dtype of cpugpupathtracing_amd.renderer.SHADE_SAMPLE), zeroed: throughput 1."""
    dt = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("t", np.float32), ("obj", np.uint32), ("tri", np.uint32), ("bvh_depth", np.uint32),
                   ("throughput", np.float32, 3), ("rng", np.uint32), ("depth", np.uint32), ("is_specular", np.uint32)])
    a = np.zeros(n, dt)
    a["throughput"] = 1.0
    return a


# ---- vector helpers in the device's operation order ------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _dot_scale(a, b, computed=False):
    """The scale of dot(a, b)'s rounding error: the sum of the magnitudes of its products, or -- computed: a boolean or one per row, the
    vectors carry errors of their own -- the product of the lengths."""
    exact = (np.abs(a[..., 0] * b[..., 0]) + np.abs(a[..., 1] * b[..., 1])) + np.abs(a[..., 2] * b[..., 2])
    return np.where(computed, np.sqrt(_dot(a, a) * _dot(b, b)), exact)


def _normalize(a):
    return a * (1.0 / np.sqrt(_dot(a, a)))[..., None]


def _reflect(d, n):
    return d - (2.0 * n) * _dot(d, n)[..., None]


def _w3(mask, a, b):
    return np.where(mask[:, None], a, b)


class Eval:
    """The state of one evaluation over n samples: the RNG, the margins, the undecided counts and the flip rule."""

    def __init__(self, rng, dtype, flip):
        self.s = np.asarray(rng, np.uint32).astype(np.uint64)
        self.dtype, self.flip = dtype, flip
        n = self.s.shape[0]
        self.margin = np.full(n, np.inf)
        self.n_und = np.zeros(n, np.int64)
        self.ill = np.zeros(n, bool)

    def condition(self, length, magnitude, mask):
        """a normalisation after a cancellation (module docstring)"""
        with np.errstate(all="ignore"):
            m = np.where(magnitude > 0, 1e-2 * length / np.where(magnitude > 0, magnitude, 1), 1.0).astype(np.float64)
        m = np.where(np.isnan(m), 0.0, m)
        self.ill |= mask & (m < MARGIN)
        self.margin = np.where(mask, np.minimum(self.margin, m), self.margin)

    def word(self, mask):
        old = self.s
        new = (old * np.uint64(_MUL) + np.uint64(_INC)) & _M32
        w = (((old >> ((old >> np.uint64(28)) + np.uint64(4))) ^ old) * np.uint64(_OUT)) & _M32
        self.s = np.where(mask, new, old)
        return (w >> np.uint64(22)) ^ w

    def uniform(self, mask):
        return random_float(self.word(mask)).astype(self.dtype)

    def decide(self, cond, m, mask):
        """cond where it is decided; an undecided comparison of a sample in `mask` is inverted as the flip rule says."""
        m = np.where(np.isnan(m), 0.0, m).astype(np.float64)
        und = mask & (m < MARGIN)
        self.margin = np.where(mask, np.minimum(self.margin, m), self.margin)
        k = self.n_und
        flip = und & {0: np.zeros_like(und), 1: k == 0, 2: np.ones_like(und), 3: k >= 1}[self.flip]
        self.n_und = k + und
        return cond ^ flip

    def lost(self, x, scale, mask):
        """x is used as a number after its sign was tested (a cosine in the Smith term): where the sign is undecided the number has no digits,
        and the sample is ill-conditioned whichever branch is taken."""
        with np.errstate(all="ignore"):
            m = np.where(scale > 0, np.abs(x) / np.where(scale > 0, scale, 1), 0.0)
        self.ill |= mask & ~(m >= MARGIN)

    def less(self, a, b, mask, exact=False):
        """a < b with the margin |a - b| / max(|a|, |b|).  exact: both numbers are float32 inputs or drawn floats, the same in either float
        type, so the comparison is the device's own whatever the distance: decided."""
        with np.errstate(all="ignore"):
            scale = np.maximum(np.abs(a), np.abs(b))
            m = np.where(scale > 0, np.abs(a - b) / np.where(scale > 0, scale, 1), 0.0)
        if exact:
            m = np.ones_like(m)
        return self.decide(a < b, m, mask)

    def sign(self, x, scale, mask, positive):
        """x > 0 (positive) or x < 0 with the margin |x| / scale."""
        with np.errstate(all="ignore"):
            m = np.where(scale > 0, np.abs(x) / np.where(scale > 0, scale, 1), 0.0)
        return self.decide(x > 0 if positive else x < 0, m, mask)


# ---- sampling (rt_device.hpp) -----------------------------------------------------------------------------------------------------------------
def _ball(ev, mask):
    n = mask.shape[0]
    out = np.zeros((n, 3), ev.dtype)
    todo = mask.copy()
    while todo.any():
        x = ev.uniform(todo) * 2.0 - 1.0
        y = ev.uniform(todo) * 2.0 - 1.0
        z = ev.uniform(todo) * 2.0 - 1.0
        v = np.stack([x, y, z], -1)
        out = _w3(todo, v, out)
        dd = _dot(v, v)
        again = ev.less(np.ones_like(dd), dd, todo)                            # dot(dir, dir) > 1
        todo = todo & again
    return out


def _uniform_hemisphere(ev, normal, mask):
    d = _ball(ev, mask)
    dn = _dot(d, normal)
    neg = ev.sign(dn, _dot_scale(d, normal, True), mask, False)
    d = _w3(neg, d * -1.0, d)
    return _normalize(d)


def _cosine_weighted(ev, normal, mask):
    v = normal + _normalize(_ball(ev, mask))
    ev.condition(np.sqrt(_dot(v, v)), np.sqrt(_dot(normal, normal)) + 1.0, mask)
    return _normalize(v)


def _lambda(a2, z):
    return 0.5 * (-1.0 + np.sqrt(1.0 + a2 * (np.maximum(0.0, 1.0 - z * z) / (z * z))))


def _visible_normal(ev, u1, u2, d, normal, facing, alpha, mask, computed):
    """ggx_visible_normal: (ok, n, oz, h).  facing: the decided dot(d, normal) < 0 (n = normal), exact zero included as the device has it.
    computed: the normal is no input (per sample)."""
    dt = ev.dtype
    dn = _dot(d, normal)
    n = _w3(~facing & (dn != 0), -normal, normal)
    sign = np.where(np.signbit(n[:, 2]), -1.0, 1.0).astype(dt)                # Duff et al. 2017
    a = -1.0 / (sign + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    tx = np.stack([1.0 + sign * n[:, 0] * n[:, 0] * a, sign * b, -sign * n[:, 0]], -1)
    ty = np.stack([b, sign + n[:, 1] * n[:, 1] * a, -n[:, 1]], -1)
    wo = -d
    ox, oy, oz = _dot(wo, tx), _dot(wo, ty), _dot(wo, n)
    ok = ev.sign(oz, _dot_scale(wo, n, computed), mask, True)
    ev.lost(oz, _dot_scale(wo, n, computed), mask)
    oz2 = oz * oz
    ok = ok & ~ev.less(oz2, np.full_like(oz2, FLT_MIN), mask & ok)             # the horizon rule: oz^2 >= FLT_MIN
    safe = mask & ok
    local = np.stack([np.where(safe, ox, 0.0), np.where(safe, oy, 0.0), np.where(safe, oz, 1.0)], -1).astype(dt)
    hl, length = RG._visible_normals(local, alpha.astype(dt), u1, u2, lengths=True)
    hl = hl.astype(dt)
    mag = np.sqrt(_dot_scale(wo, tx) ** 2 + _dot_scale(wo, ty) ** 2)        # 0: ox = oy = 0 exactly, t1 = (1, 0, 0) in either float type
    ev.condition(np.sqrt(ox * ox + oy * oy), mag, safe)
    ev.condition(length, np.ones_like(length), safe)
    h = hl[:, 0:1] * tx + hl[:, 1:2] * ty + hl[:, 2:3] * n
    return ok, n, oz, h


# ---- get_hit -----------------------------------------------------------------------------------------------------------------------------------
def _hit_normals(ev, scene, level, o, d, t, obj, tri, pos, act):
    dt = ev.dtype
    normal = np.zeros_like(pos)
    computed = np.zeros(act.shape[0], bool)                                   # the normal is no input: a sphere's, an interpolated or a transformed one
    for k, ob in enumerate(scene.objects):
        sel = act & (obj == k)
        if not sel.any():
            continue
        i = np.nonzero(sel)[0]
        if ob["kind"] == "plane":
            normal[i] = ob["normal"].astype(dt)
        elif ob["kind"] == "sphere":
            normal[i] = _normalize(pos[i] - ob["center"].astype(dt))
            computed[i] = True
        else:
            rows = ob["rows"]
            tk = tri[i].astype(np.int64) if ob["kind"] == "mesh" else np.zeros(i.size, np.int64)
            r = rows[tk]
            no = r[:, 3:6].astype(dt)
            m = ob.get("transform")
            xform = level >= 4 and m is not None and not TR.is_identity(m)
            rec = TR.invert(m) if xform else None
            if level >= 3 and ob.get("smooth"):
                if xform:
                    P_, d_ = TR.ray_to_object(rec, o[i], d[i], dtype=dt)
                    P_ = P_ + d_ * t[i][:, None]
                else:
                    P_, d_ = pos[i], d[i]
                tri_args = (r[:, 0:3], r[:, 6:9], r[:, 12:15], r[:, 3:6], r[:, 9:12], r[:, 15:18], P_, d_, dt)
                no, rule, sm = SM.smooth_normal(*tri_args, margins=True)
                sub = np.zeros(act.shape[0], bool); sub[i] = True
                full = np.full(act.shape[0], np.inf); full[i] = sm
                geo = np.zeros(act.shape[0], bool); geo[i] = rule == SM.GEOMETRIC
                other = ev.decide(geo, full, sub)[i] != geo[i]                  # the side rule of step 5, inverted where the flip rule says so
                if other.any():
                    no = SM.smooth_normal(*tri_args, invert_side=other)[0]
            normal[i] = TR.normal_to_world(rec, no, dtype=dt) if xform else no
            computed[i] = xform or bool(level >= 3 and ob.get("smooth"))
    return normal, computed


# ---- lights ------------------------------------------------------------------------------------------------------------------------------------
def _sample_light(ev, scene, pos, mask):
    """sample_light: (to_light, light normal, emission, distance, area) for the samples in mask."""
    dt = ev.dtype
    n = mask.shape[0]
    nl = len(scene.lights)
    pick = np.zeros(n, np.int64)
    if nl > 1:
        pick = (ev.word(mask) % np.uint64(nl)).astype(np.int64)
    lpos, lnormal, emission, area = np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros(n, dt)
    for k, li in enumerate(scene.lights):
        sel = mask & (pick == k)
        ob = scene.objects[li]
        mat = scene.materials[ob["mat"]]
        e = np.asarray(mat["emissive"], np.float32).astype(dt) * np.float32(mat["intensity"]).astype(dt)
        emission = _w3(sel, e, emission)
        if ob["kind"] == "mesh":
            rows = ob["rows"]
            tk = np.zeros(n, np.int64)
            if rows.shape[0] > 1:
                tk = (ev.word(sel) % np.uint64(rows.shape[0])).astype(np.int64)
            r = rows[tk].astype(dt)
            a, b = ev.uniform(sel), ev.uniform(sel)
            fold = ev.less(np.ones_like(a), a + b, sel)
            a, b = np.where(fold, 1.0 - a, a), np.where(fold, 1.0 - b, b)
            g = 1.0 - b - a
            p = a[:, None] * r[:, 0:3] + b[:, None] * r[:, 6:9] + g[:, None] * r[:, 12:15]
            lpos, lnormal = _w3(sel, p, lpos), _w3(sel, r[:, 3:6], lnormal)
            area = np.where(sel, (ob["total_area"] / np.float32(2.0)).astype(dt), area)
        else:
            c = ob["center"].astype(dt)
            with np.errstate(all="ignore"):
                to_pos = _normalize(pos - c)
                dirn = _uniform_hemisphere(ev, to_pos, sel)
                p = c + ob["radius"].astype(dt) * dirn
                lpos, lnormal = _w3(sel, p, lpos), _w3(sel, _normalize(p - c), lnormal)
            r2 = (ob["radius"] * ob["radius"]).astype(dt)
            area = np.where(sel, 2.0 * K_PI.astype(dt) * r2, area)
    to_light = lpos - pos
    dist = np.sqrt(_dot(to_light, to_light))
    return _normalize(to_light), lnormal, emission, dist, area


def _unshadowed(scene_nl, albedo, thr, ndl, nldl, area, dist, emission, dw, dt):
    brdf = albedo * K_INV_PI.astype(dt)
    solid = (nldl * area) / (dist * dist)
    pdf = 1.0 / solid
    return thr * (ndl / pdf)[:, None] * brdf * emission * dt(scene_nl) * dw[:, None]


class Reservoir:
    """The streaming reservoir of shade_bounce<.., RIS> for n samples: candidate j with the unshadowed contribution c (its weight the sum
    of c's components where both cosine tests passed, else 0) is kept when the reservoir is empty or u * wsum < w.  The same three steps
    as ris_ref.Reservoir, which states them in float64 for a distribution; test_shade_reference.py feeds both the same candidates."""

    def __init__(self, n, dt):
        self.wsum, self.w_y, self.dist_y = np.zeros(n, dt), np.zeros(n, dt), np.zeros(n, dt)
        self.c_y, self.dir_y = np.zeros((n, 3), dt), np.zeros((n, 3), dt)

    def update(self, ev, c, up, u, direction, dist, lit):
        w = np.where(up, c[:, 0] + c[:, 1] + c[:, 2], 0.0).astype(self.wsum.dtype)
        self.wsum = np.where(lit, self.wsum + w, self.wsum)
        can = lit & (w > 0.0)
        empty = self.w_y == 0.0
        take = can & (empty | ev.less(u * self.wsum, w, can & ~empty))
        self.c_y, self.dir_y = _w3(take, c, self.c_y), _w3(take, direction, self.dir_y)
        self.w_y, self.dist_y = np.where(take, w, self.w_y), np.where(take, dist, self.dist_y)
        return take

    def pending(self, M):
        return self.c_y * (self.wsum / (self.wsum.dtype.type(M) * self.w_y))[:, None]


# ---- the bounce --------------------------------------------------------------------------------------------------------------------------------
def shade(scene, st, smp, dtype=np.float64, candidates=1, level=None, flip=0):
    """shade_bounce<false, level, RIS> on the records smp.  Returns a dict of arrays: the cgpt_shade_result fields, `margin` (float64) and
    `undecided` (margin < MARGIN).  level: default the scene's; candidates: cgpt_set_nee_candidates."""
    dt = dtype
    level = scene.lobe_level() if level is None else level
    n = smp.shape[0]
    ev = Eval(smp["rng"], dt, flip)
    o, d, t = smp["o"].astype(dt), smp["d"].astype(dt), smp["t"].astype(dt)
    obj, tri = smp["obj"].astype(np.int64), smp["tri"]
    thr = smp["throughput"].astype(dt)
    depth = smp["depth"].astype(np.int64)
    spec = smp["is_specular"] != 0
    energy = np.zeros((n, 3), dt)
    flags = np.zeros(n, np.uint32)
    ray_o, ray_d = o.copy(), d.copy()
    sh_o, sh_d, sh_t, pending = np.zeros((n, 3), dt), np.zeros((n, 3), dt), np.zeros(n, dt), np.zeros((n, 3), dt)
    unwalked = np.zeros(n, np.uint32)
    maxd = int(st["max_ray_depth"])
    nee = bool(st["nee"])
    ris = nee and candidates > 1
    nl = len(scene.lights)
    act = np.ones(n, bool)

    with np.errstate(all="ignore"):
        # the BVH-depth view, a miss
        view = act & (depth == 0) & (st["debug_mode"] == 2)
        s_ = smp["bvh_depth"].astype(np.float32).astype(dt) / dt(30.0)
        colour = np.stack([0.0 + (1.0 - 0.0) * s_, 1.0 + (0.0 - 1.0) * s_, 0.0 * s_], -1).astype(dt)
        energy = _w3(view, energy + colour, energy)
        flags[view] = TERMINATE | ENERGY
        act &= ~view
        miss = act & (smp["obj"] == NO_HIT)
        flags[miss] = TERMINATE
        act &= ~miss
        obj = np.where(act, obj, 0)

        # the hit and its material
        pos = o + d * t[:, None]
        normal, ncomp = _hit_normals(ev, scene, level, o, d, t, obj, tri, pos, act)
        mi = np.array([ob["mat"] for ob in scene.objects], np.int64)[obj]

        def col(key, width=None):
            a = np.array([np.asarray(m[key], np.float32) for m in scene.materials], np.float32)[mi]
            return a.astype(dt)
        albedo, specular, refr, absorption, ior = col("albedo"), col("specular"), col("refractivity"), col("absorption"), col("ior")
        emissive, intensity = col("emissive"), col("intensity")
        rough = np.array([np.float32(m["roughness"]) for m in scene.materials], np.float32)[mi]
        rough_t = np.array([np.float32(m["transmission_roughness"]) for m in scene.materials], np.float32)[mi]
        alpha, alpha_t = (rough * rough).astype(dt), (rough_t * rough_t).astype(dt)     # PackMaterial squares in float32
        is_light = np.array([bool(m["is_light"]) for m in scene.materials])[mi]

        light = act & is_light
        adds = light & ((not nee) | (depth == 0) | spec)
        energy = _w3(adds, energy + thr * emissive * intensity[:, None], energy)
        flags[light] = TERMINATE
        flags[adds] = TERMINATE | ENERGY
        act &= ~light

        # next event estimation: one sample or the reservoir of M candidates
        dw = np.maximum(0.0, 1.0 - specular - refr).astype(dt)
        result = np.zeros(n, np.uint32)
        lit = np.zeros(n, bool)
        if nl > 0 and nee:
            lit = act & ~ev.less(dw, np.full_like(dw, np.float32(0.001)), act) & (dw != np.float32(0.001).astype(dt))
        if ris:
            res = Reservoir(n, dt)
            for _ in range(candidates):
                tl, ln, em, dist, area = _sample_light(ev, scene, pos, lit)
                u = ev.uniform(lit)
                ndl, nldl = _dot(normal, tl), _dot(ln, -tl)
                c = _unshadowed(nl, albedo, thr, ndl, nldl, area, dist, em, dw, dt)
                up = ev.sign(ndl, _dot_scale(normal, tl, True), lit, True)
                up = up & ev.sign(nldl, _dot_scale(ln, tl, True), lit & up, True)
                res.update(ev, c, up, u, tl, dist, lit)
            wsum, w_y, dist_y, c_y, dir_y = res.wsum, res.w_y, res.dist_y, res.c_y, res.dir_y
            sh = lit & (wsum > 0.0)
            sh_o, sh_d = _w3(sh, pos + dir_y * K_NUDGE.astype(dt), sh_o), _w3(sh, dir_y, sh_d)
            sh_t = np.where(sh, dist_y - 2.0 * K_NUDGE.astype(dt), sh_t)
            pending = _w3(sh, res.pending(candidates), pending)
            result[sh] |= SHADOW
        elif lit.any():
            tl, ln, em, dist, area = _sample_light(ev, scene, pos, lit)
            ndl, nldl = _dot(normal, tl), _dot(ln, -tl)
            up = ev.sign(ndl, _dot_scale(normal, tl, True), lit, True)
            up = up & ev.sign(nldl, _dot_scale(ln, tl, True), lit & up, True)
            sh = lit & up
            sh_o, sh_d = _w3(sh, pos + tl * K_NUDGE.astype(dt), sh_o), _w3(sh, tl, sh_d)
            sh_t = np.where(sh, dist - 2.0 * K_NUDGE.astype(dt), sh_t)
            pending = _w3(sh, _unshadowed(nl, albedo, thr, ndl, nldl, area, dist, em, dw, dt), pending)
            result[sh] |= SHADOW

        # Russian roulette, the lobe draw
        p = np.clip(np.maximum(np.maximum(albedo[:, 0], albedo[:, 1]), albedo[:, 2]), np.float32(0.1).astype(dt), 1.0).astype(dt)

        def roulette(mask):
            nonlocal thr, act
            if not st["rr"]:
                return
            u = ev.uniform(mask)
            dead = mask & ev.less(p, u, mask, exact=True)
            flags[dead] = result[dead] | TERMINATE
            act = act & ~dead
            live = mask & ~dead
            thr = _w3(live, thr * (1.0 / p)[:, None], thr)
        roulette(act.copy())
        r = ev.uniform(act)
        sr = specular + refr
        lt_s = ev.less(r, specular, act, exact=True) & act
        lt_sr = ev.less(r, sr, act & ~lt_s) & act & ~lt_s                      # the dielectric range: !(r < specular) && r < specular + refractivity

        # the smooth dielectric's interface (glass_interface): a function of the ray and the hit alone
        cosi0 = np.clip(_dot(normal, d), -1.0, 1.0)
        front = np.zeros(n, bool); k_ge0 = np.zeros(n, bool); k_known = np.zeros(n, bool)
        etai, etat = np.ones(n, dt), ior.copy()

        def interface(mask):
            """decides the side and k >= 0 once for the samples in mask that have not been through it"""
            nonlocal front, k_ge0, k_known, etai, etat
            new = mask & ~k_known
            if not new.any():
                return
            f = ev.sign(cosi0, _dot_scale(normal, d, ncomp), new, False)
            front = np.where(new, f, front)
            etai = np.where(new & ~f, ior, etai); etat = np.where(new & ~f, 1.0, etat).astype(dt)
            eta = etai / etat
            cosi = np.abs(cosi0)
            k = 1.0 - eta * eta * (1.0 - cosi * cosi)
            ge = ~ev.sign(k, np.ones_like(k), new, False)
            k_ge0 = np.where(new, ge, k_ge0)
            k_known = k_known | new

        # stuck iterations
        rough_glass = (level >= 2) & (alpha_t > 0.0)
        absorbed = np.zeros(n, bool)
        cand = act & ~lit & ~rough_glass & ~lt_s & lt_sr
        interface(cand)
        stuck = cand & ~k_ge0
        while True:
            go = stuck & act & (depth + 1 <= maxd)
            if not go.any():
                break
            depth = np.where(go, depth + 1, depth)
            unwalked[go] += 1
            absorbed |= go
            roulette(go)
            go = go & act
            r = np.where(go, ev.uniform(go), r)
            new_s = ev.less(r, specular, go, exact=True)
            new_sr = ev.less(r, sr, go & ~new_s) & ~new_s
            lt_s, lt_sr = np.where(go, new_s, lt_s), np.where(go, new_sr, lt_sr)
            stuck = stuck & act & lt_sr

        # the lobes
        ggx = act & lt_s & (level >= 1) & (alpha > 0.0)
        mirror = act & lt_s & ~ggx
        rglass = act & lt_sr & rough_glass
        glass = act & lt_sr & ~rglass
        diffuse = act & ~lt_s & ~lt_sr
        nudge = K_NUDGE.astype(dt)

        def end(mask):
            nonlocal act
            flags[mask] = result[mask] | TERMINATE
            act = act & ~mask

        if ggx.any():
            u1, u2 = ev.uniform(ggx), ev.uniform(ggx)
            facing = ev.sign(_dot(d, normal), _dot_scale(d, normal, ncomp), ggx, False)
            ok, nn, oz, h = _visible_normal(ev, u1, u2, d, normal, facing, alpha, ggx, ncomp)
            end(ggx & ~ok)
            ggx = ggx & ok
            wi = _reflect(d, h)
            iz = _dot(wi, nn)
            up = ev.sign(iz, _dot_scale(wi, nn, True), ggx, True)
            ev.lost(iz, _dot_scale(wi, nn, True), ggx)
            end(ggx & ~up)
            ggx = ggx & up
            a2 = alpha * alpha
            lo, li = _lambda(a2, oz), _lambda(a2, iz)
            g = (1.0 + lo) / (1.0 + lo + li)
            ray_o, ray_d = _w3(ggx, pos + wi * nudge, ray_o), _w3(ggx, wi, ray_d)
            thr = _w3(ggx, thr * (albedo * g[:, None]), thr)
            spec = spec | ggx
        if mirror.any():
            rd = _reflect(d, normal)
            ray_o, ray_d = _w3(mirror, pos + rd * nudge, ray_o), _w3(mirror, rd, ray_d)
            thr = _w3(mirror, thr * albedo, thr)
            spec = spec | mirror
            result[mirror] |= CHAIN_REFLECT << CHAIN_SHIFT
        if rglass.any():
            u1, u2 = ev.uniform(rglass), ev.uniform(rglass)
            facing = ev.sign(_dot(normal, d), _dot_scale(normal, d, ncomp), rglass, False)
            inside = ~facing
            ei, et = np.where(inside, ior, 1.0).astype(dt), np.where(inside, 1.0, ior).astype(dt)
            eta = ei / et
            ok, nn, oz, h = _visible_normal(ev, u1, u2, d, normal, facing, alpha_t, rglass, ncomp)
            end(rglass & ~ok)
            rglass = rglass & ok
            dh = _dot(d, h)
            c = -dh
            k = 1.0 - eta * eta * (1.0 - c * c)
            kge = rglass & ~ev.sign(k, np.ones_like(k), rglass, False)
            wt = _normalize(d * eta[:, None] + ((eta * c - np.sqrt(np.maximum(k, 0.0)))[:, None] * h))
            Fr = RG.facet_fresnel(c, k, ei, et).astype(dt)
            u3 = ev.uniform(kge)
            refracts = kge & ev.less(Fr, u3, kge)
            w = _w3(refracts, wt, _reflect(d, h))
            wz = _dot(w, nn)
            right = np.where(refracts, ev.sign(wz, _dot_scale(w, nn, True), rglass & refracts, False), ev.sign(wz, _dot_scale(w, nn, True), rglass & ~refracts, True))
            ev.lost(wz, _dot_scale(w, nn, True), rglass)
            end(rglass & ~right)
            rglass = rglass & right
            a2 = alpha_t * alpha_t
            lo, lw = _lambda(a2, oz), _lambda(a2, np.abs(wz))
            g = (1.0 + lo) / (1.0 + lo + lw)
            thr = _w3(rglass, thr * (albedo * g[:, None]), thr)
            out = rglass & refracts & inside
            thr = _w3(out, thr * np.exp(-absorption * t[:, None]), thr)
            ray_o, ray_d = _w3(rglass, pos + w * nudge, ray_o), _w3(rglass, w, ray_d)
            spec = spec | rglass
        if glass.any():
            interface(glass)
            tir = glass & ~k_ge0
            result[tir] |= CHAIN_TIR << CHAIN_SHIFT                            # the ray is left as it is
            go = glass & k_ge0
            eta = etai / etat
            cosi = np.abs(cosi0)
            k = 1.0 - eta * eta * (1.0 - cosi * cosi)
            N = _w3(front, normal, -normal)
            rd = _normalize(d * eta[:, None] + ((eta * cosi - np.sqrt(np.maximum(k, 0.0)))[:, None] * N))
            Fr = RG.facet_fresnel(cosi, k, etai, etat).astype(dt)
            u = ev.uniform(go)
            refr_ = go & ev.less(Fr, u, go)
            refl_ = go & ~refr_
            thr = _w3(go, thr * albedo, thr)
            out = refr_ & ~front
            thr = _w3(out, thr * np.exp(-absorption * t[:, None]), thr)
            gd = _w3(refr_, rd, _reflect(d, normal))
            ray_o, ray_d = _w3(go, pos + gd * nudge, ray_o), _w3(go, gd, ray_d)
            spec = spec | go
            result[refr_] |= CHAIN_REFRACT << CHAIN_SHIFT
            result[refl_] |= CHAIN_REFLECT << CHAIN_SHIFT
        if diffuse.any():
            kpi = K_PI.astype(dt)
            if st["cosine"]:
                dd = _cosine_weighted(ev, normal, diffuse)
                ndr = _dot(dd, normal)
                pdf = np.full(n, 1.0 / (2.0 * kpi), dt)
            else:
                dd = _uniform_hemisphere(ev, normal, diffuse)
                ndr = _dot(dd, normal)
                pdf = ndr / kpi
            ray_o, ray_d = _w3(diffuse, pos + dd * nudge, ray_o), _w3(diffuse, dd, ray_d)
            thr = _w3(diffuse, thr * ((ndr / pdf)[:, None] * (albedo * K_INV_PI.astype(dt))), thr)
            spec = spec & ~diffuse

        result[absorbed] &= ~np.uint32(3 << CHAIN_SHIFT)
        depth = np.where(act, depth + 1, depth)
        over = act & (depth > maxd)
        result[over] |= TERMINATE
        flags[act] = result[act]

    no_sh = (flags & SHADOW) == 0
    sh_o[no_sh] = 0; sh_d[no_sh] = 0; sh_t[no_sh] = 0; pending[no_sh] = 0
    return dict(flags=flags, o=ray_o, d=ray_d, throughput=thr, energy=energy, rng=ev.s.astype(np.uint32), depth=depth.astype(np.uint32),
                is_specular=spec.astype(np.uint32), shadow_o=sh_o, shadow_d=sh_d, shadow_tmax=sh_t, pending=pending, unwalked=unwalked,
                margin=ev.margin, undecided=ev.margin < MARGIN, ill=ev.ill)


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------
FACTOR = 8.0
FLOOR_ULPS = 4.0
EPS32 = float(np.finfo(np.float32).eps)


def same_discrete(a, b):
    """Per sample: the discrete outputs of two evaluations (or of the device's records and an evaluation) are equal."""
    return np.all([np.asarray(a[k]) == np.asarray(b[k]) for k in DISCRETE], 0)


def deviation(a, ref, keep):
    """Per group: the largest |a - ref| over the samples in keep, and the largest |ref| there (the floor's magnitude)."""
    out = {}
    for g in GROUPS:
        dev = mag = 0.0
        for f in FLOATS[g]:
            x, y = np.asarray(a[f], np.float64)[keep], np.asarray(ref[f], np.float64)[keep]
            if x.size:
                dev = max(dev, float(np.max(np.abs(x - y))))
                mag = max(mag, float(np.max(np.abs(y))))
        out[g] = (dev, mag)
    return out


def tolerances(m32, m64):
    """Per group: FACTOR times the largest deviation of the float32 from the float64 evaluation over the decided samples, plus FLOOR_ULPS
    float32 ulps of the group's largest magnitude.  Returns ({group: tolerance}, keep): keep = decided in float64 and the same discrete
    outcome in both evaluations (test_shade_reference.py asserts that this is every decided sample)."""
    keep = ~m64["undecided"] & same_discrete(m32, m64)
    dev = deviation(m32, m64, keep)
    return {g: FACTOR * dev[g][0] + FLOOR_ULPS * EPS32 * dev[g][1] for g in GROUPS}, keep
