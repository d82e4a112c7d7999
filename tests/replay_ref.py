"""A whole render restated on the host as the chain of its two steps: every (pixel, sample) path of a frame advanced in lockstep through a
`trace` callable (IntersectScene on a ray batch) and a `shade` callable (one shade_bounce call per record), exactly as `megakernel`
(csrc/device/path_kernels.hip) chains intersect_scene and shade_bounce.  With the context's own probes (Renderer.intersect_rays,
Renderer.shade_samples) the replay is a second statement of a render whose accumulator can be compared word for word
(test_gpu_path_replay.py); with the numpy models (FlatSceneModel below, shade_ref.shade) it needs no GPU (test_replay_reference.py).

The loop.  A path (px, global row py, sample s) starts with rng = pcg_seed(py * W + px, s, seed), the primary ray of its pixel,
throughput 1, energy 0, depth 0, is_specular 0.  One step, for every live path at once:
  1. the extend rays are traced -- except a path whose last result carried chain choice TIR without the terminate bit: it keeps its ray
     and its hit record (megakernel's same_ray), which counts one ray and one unwalked re-trace;
  2. one shade call on the records (the traced ray, its hit, the path state);
  3. energy = energy + result.energy (float32; shade_bounce adds to the path's energy at most once per call, and 0 otherwise);
  4. the shadow rays of the results with the shadow bit are traced with shadow_tmax; where such a ray misses, energy = energy + pending,
     whether or not the terminate bit ended the path in the same call;
  5. o, d, throughput, rng, depth, is_specular are the result's; the path lives on unless the terminate bit is set.
Steps 3 and 4 are in the device's order; no result carries both a bounce energy and the shadow bit (a light hit ends the path before the
light is sampled), so at most one of the two adds is not + 0.
A finished path adds float64(float32((e.x + e.y) + e.z)) * 0.001 to the energy sum and, per pixel in sample order, acc.xyz += e, acc.w += 1
in float32.  Rays: every extend trace, every kept (TIR) ray, every shadow trace and every result's `unwalked` (the in-place iterations of a
stuck total internal reflection, each an IntersectScene call of the reference that the device answers without a walk).
"""
from __future__ import annotations

import numpy as np

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd.distributed import interleaved_rows
import shade_ref as S
import smooth_ref as SM
import tlas_ref as TL
import transform_ref as TR

MAX_CALL = 65536                                                               # cgpt_shade_samples takes no more
F = np.float32


# ---- the seed: rt_device.hpp wang_hash / pcg_seed, numpy integers ----------------------------------------------------------------------------
def wang_hash(x):
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x, np.uint64) & m
    x = (x ^ np.uint64(61)) ^ (x >> np.uint64(16))
    x = (x * np.uint64(9)) & m
    x = x ^ (x >> np.uint64(4))
    x = (x * np.uint64(0x27D4EB2D)) & m
    x = x ^ (x >> np.uint64(15))
    return x


def pcg_seed(pixel_index, sample_index, seed):
    """pcg_seed(global pixel index, sample index, seed) as uint32, elementwise."""
    h = wang_hash(np.uint64(seed & 0xFFFFFFFF))
    h = wang_hash(h ^ np.asarray(sample_index, np.uint64))
    h = wang_hash(h ^ np.asarray(pixel_index, np.uint64))
    return h.astype(np.uint32)


# ---- the primary ray: camera_ray with primary_ray's u, v (trace_steps.hpp), float32 in the device's operation order -------------------------
def camera_of(cam):
    """(pos, top_left, top_right, bottom_left) float32 from a cgpt_camera."""
    return tuple(np.array([float(x) for x in getattr(cam, k)], np.float32) for k in ("pos", "top_left", "top_right", "bottom_left"))


def camera_rays(cam, W, H):
    """(origins, dirs) (H, W, 3) float32: u = float32(px) * (float32(1) / float32(W)), v likewise from the row and H,
    pixel = (tl + u (tr - tl)) + v (bl - tl), d = (pixel - pos) * (1 / sqrt((x x + y y) + z z))."""
    pos, tl, tr, bl = camera_of(cam)
    u = (np.arange(W, dtype=np.float32) * (F(1.0) / F(W))).astype(np.float32)
    v = (np.arange(H, dtype=np.float32) * (F(1.0) / F(H))).astype(np.float32)
    right, down = (tr - tl).astype(np.float32), (bl - tl).astype(np.float32)
    pixel = ((tl[None, None] + u[None, :, None] * right[None, None]).astype(np.float32) + v[:, None, None] * down[None, None]).astype(np.float32)
    p = (pixel - pos[None, None]).astype(np.float32)
    dd = ((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]).astype(np.float32) + p[..., 2] * p[..., 2]).astype(np.float32)
    rcp = (F(1.0) / np.sqrt(dd).astype(np.float32)).astype(np.float32)
    d = (p * rcp[..., None]).astype(np.float32)
    return np.broadcast_to(pos, d.shape).copy(), d


def pack_pixels(acc, n):
    """vec4_to_uint(acc.xyz / n) per pixel (rt_device.hpp), n = float32(samples accumulated)."""
    with np.errstate(all="ignore"):
        c = (acc[..., :3].astype(np.float32) / F(n)).astype(np.float32)
        f = (F(255.0) * np.minimum(F(1.0), c)).astype(np.float32)
        w = np.where(f < 0, F(0.0), f).astype(np.int64).astype(np.uint32) & np.uint32(0xFF)
    return (np.uint32(255 << 24) + (w[..., 2] << np.uint32(16)) + (w[..., 1] << np.uint32(8)) + w[..., 0]).astype(np.uint32)


# ---- the model traversal for the dry run -------------------------------------------------------------------------------------------------------
class FlatSceneModel(TL.SceneModel):
    """tlas_ref.SceneModel with a mesh tested triangle by triangle in index order instead of through its tree, vectorised over the rays:
    the same float32 intersectors and the same strict t <, so the closest hit is the tree walk's except where two triangles tie to the
    bit.  The dry run needs a population, not the device's bits, and the per-ray tree walk of MeshModel is a Python loop."""

    def _test(self, k, idx, o, d, st):
        ob = self.spec[k]
        if ob["kind"] != "mesh":
            return super()._test(k, idx, o, d, st)
        oo, od = o[idx], d[idx]
        m = ob.get("transform")
        if m is not None and not TR.is_identity(m):
            oo, od = TR.ray_to_object(TR.invert(m), oo, od)
        mm = ob["model"]
        t = st["t"][idx].copy()
        tri = st["tri"][idx].copy()
        hit = np.zeros(idx.size, bool)
        for j in range(mm.v0.shape[0]):
            ok, tt = TL.hit_triangle(mm.v0[j], mm.e1[j], mm.e2[j], oo, od, t)
            t = np.where(ok, tt, t).astype(np.float32)
            tri = np.where(ok, j, tri)
            hit |= ok
        h = idx[hit]
        st["t"][h] = t[hit]; st["tri"][h] = tri[hit]; st["obj"][h] = k


def model_trace(model_scene, device_scene, level=None, tree=False):
    """A trace callable over a shade_ref.ModelScene: FlatSceneModel on the scene's objects, each mesh with the tree the host library built
    for it (device_scene: the cpugpupathtracing_amd.Scene of model_scene.device_scene()).  level: transforms are honoured from 4 up."""
    level = model_scene.lobe_level() if level is None else level
    spec = []
    for k, ob in enumerate(model_scene.objects):
        e = dict(kind=ob["kind"])
        if ob["kind"] == "plane":
            e.update(normal=ob["normal"], point=ob["point"])
        elif ob["kind"] == "sphere":
            e.update(center=ob["center"], radius=float(ob["radius"]))
        else:
            e["transform"] = ob.get("transform") if level >= 4 else None
            if ob["kind"] == "triangle":
                e["positions"] = ob["positions"]
            else:
                e["model"] = TL.MeshModel(ob["vertices"], ob["indices"], *device_scene.bvh_export(k))
        spec.append(e)
    model = FlatSceneModel(spec)

    def trace(o, d, tmax=None):
        return model.walk(o, d, tmax, tree=tree)[:4]
    return trace


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------------
def _chunks(n):
    return [slice(a, min(a + MAX_CALL, n)) for a in range(0, n, MAX_CALL)]


def _trace(trace, o, d, tmax=None):
    parts = [trace(o[c], d[c], None if tmax is None else tmax[c]) for c in _chunks(o.shape[0])]
    return tuple(np.concatenate([np.asarray(p[k]) for p in parts]) for k in range(4))


def _shade(shade, smp, settings):
    parts = [shade(smp[c], settings) for c in _chunks(smp.shape[0])]
    if not isinstance(parts[0], dict):
        return np.concatenate(parts)                                           # the device's records, kept as they are
    return {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in parts[0]}


def replay(trace, shade, camera_rays, W, H, rows, first_sample, n_samples, seed, settings, accumulator=None, max_steps=4096):
    """Advances the paths of the pixels (px, py) for py in rows (global row numbers, in the band's storage order), px in [0, W), samples
    first_sample .. first_sample + n_samples - 1.  trace(o, d, tmax or None) -> (t, obj, tri, bvh_depth); shade(samples, settings) ->
    cgpt_shade_result fields (a record array or a dict of arrays); camera_rays: (origins, dirs) (H, W, 3) of the whole frame.
    accumulator: the band's running sums before these samples (default zeros).
    Returns dict(accumulator (len(rows), W, 4) float32, rays, unwalked, energy_sum (float64), energy (path energies (rows, W, samples, 3)),
    path_rays, path_unwalked, path_energy_sum (the three counters per path, (rows, W, samples): paths are independent, so a band's
    counters are the sums over its rows), steps: per step dict(idx: the path numbers ((local row * W + px) * n_samples + s), samples, results))."""
    rows = np.asarray(rows, np.int64)
    R = rows.size
    N = R * W * n_samples
    path = np.arange(N)
    s_of = first_sample + path % n_samples
    px = (path // n_samples) % W
    py = rows[path // (n_samples * W)]
    cam_o, cam_d = camera_rays
    o = np.ascontiguousarray(cam_o[py, px], np.float32); d = np.ascontiguousarray(cam_d[py, px], np.float32)
    rng = pcg_seed(py * W + px, s_of, seed)
    thr = np.ones((N, 3), np.float32); energy = np.zeros((N, 3), np.float32)
    depth = np.zeros(N, np.uint32); spec = np.zeros(N, np.uint32)
    alive = np.ones(N, bool); same = np.zeros(N, bool)
    hit_t = np.zeros(N, np.float32); hit_obj = np.full(N, S.NO_HIT, np.uint32); hit_tri = np.zeros(N, np.uint32); hit_depth = np.zeros(N, np.uint32)
    rays, unwalked = np.zeros(N, np.int64), np.zeros(N, np.int64)
    steps = []
    for _ in range(max_steps):
        idx = np.nonzero(alive)[0]
        if not idx.size:
            break
        go = idx[~same[idx]]
        if go.size:
            hit_t[go], hit_obj[go], hit_tri[go], hit_depth[go] = _trace(trace, o[go], d[go])
        rays[idx] += 1                                                         # traced, or the same ray again: counted, not walked
        unwalked[idx[same[idx]]] += 1
        smp = S.samples(idx.size)
        smp["o"], smp["d"], smp["t"], smp["obj"], smp["tri"], smp["bvh_depth"] = o[idx], d[idx], hit_t[idx], hit_obj[idx], hit_tri[idx], hit_depth[idx]
        smp["throughput"], smp["rng"], smp["depth"], smp["is_specular"] = thr[idx], rng[idx], depth[idx], spec[idx]
        res = _shade(shade, smp, settings)
        flags = res["flags"].astype(np.uint32)
        rays[idx] += res["unwalked"].astype(np.int64)
        unwalked[idx] += res["unwalked"].astype(np.int64)
        energy[idx] = (energy[idx] + res["energy"].astype(np.float32)).astype(np.float32)
        sh = (flags & S.SHADOW) != 0
        if sh.any():
            so, sd = np.ascontiguousarray(res["shadow_o"][sh], np.float32), np.ascontiguousarray(res["shadow_d"][sh], np.float32)
            _, sobj, _, _ = _trace(trace, so, sd, np.ascontiguousarray(res["shadow_tmax"][sh], np.float32))
            rays[idx[sh]] += 1
            free = idx[sh][sobj == S.NO_HIT]
            energy[free] = (energy[free] + res["pending"][sh][sobj == S.NO_HIT].astype(np.float32)).astype(np.float32)
        o[idx], d[idx], thr[idx] = res["o"], res["d"], res["throughput"]
        rng[idx], depth[idx], spec[idx] = res["rng"], res["depth"], res["is_specular"]
        ended = (flags & S.TERMINATE) != 0
        alive[idx] = ~ended
        same[idx] = ~ended & (((flags >> S.CHAIN_SHIFT) & 3) == S.CHAIN_TIR)
        steps.append(dict(idx=idx, samples=smp, results=res))
    assert not alive.any(), "a path outlived max_steps"
    acc = np.zeros((R, W, 4), np.float32) if accumulator is None else np.array(accumulator, np.float32).reshape(R, W, 4)
    e = energy.reshape(R, W, n_samples, 3)
    for k in range(n_samples):
        acc[..., :3] = (acc[..., :3] + e[:, :, k]).astype(np.float32)
        acc[..., 3] = (acc[..., 3] + F(1.0)).astype(np.float32)
    total = ((energy[:, 0] + energy[:, 1]).astype(np.float32) + energy[:, 2]).astype(np.float32).astype(np.float64) * 0.001
    shape = (R, W, n_samples)
    return dict(accumulator=acc, rays=int(rays.sum()), unwalked=int(unwalked.sum()), energy_sum=float(total.sum()), energy=e, steps=steps,
                path_rays=rays.reshape(shape), path_unwalked=unwalked.reshape(shape), path_energy_sum=total.reshape(shape))


# ---- the scene, the views and the configurations of test_replay_reference.py and test_gpu_path_replay.py ----------------------------------------
W, H, SEED = 40, 28, 0x13579BDF                                                 # padded 8 x 8 and 16 x 16 tiles, W / 2 = 20
LEVELS, CANDIDATES = (0, 1, 2, 3, 4), (1, 4)
ROUGHNESS, TRANSMISSION_ROUGHNESS = 0.3, 0.2
GLASS_CENTER, GLASS_RADIUS = (0.1, 0.9, -2.0), 0.9
MESH_CENTER, MESH_RADIUS = (1.9, 0.85, -3.1), 0.8
# of the mesh at level 4: a rotation and a non-uniform scale about the mesh's own centre
_A = TR.rotation((0.3, 1.0, -0.2), 0.7) @ np.diag([1.2, 0.8, 1.0])
MOVED = TR.affine(_A, np.asarray(MESH_CENTER) - _A @ np.asarray(MESH_CENTER))
# first view: 3 samples after 2 earlier ones, NEE on; second view: from inside the glass sphere, off its centre, up at the lamp through the far wall (a third of the pixels beyond the critical angle), NEE off
VIEWS = (dict(name="outside", camera=((0.0, 4.0, 1.6), (0.0, -0.9, -1.0), 60.0, W / H), first_sample=2, n_samples=3, nee=True),
         dict(name="inside_glass", camera=((GLASS_CENTER[0] + 0.5, GLASS_CENTER[1] - 0.5, GLASS_CENTER[2]), (0.0, 1.0, -0.1), 70.0, W / H),
              first_sample=0, n_samples=2, nee=False))


def view_settings(view):
    return S.settings(max_ray_depth=5, nee=view["nee"], cosine=True, rr=True)


def build_scene():
    """(ModelScene at level 0, names): a diffuse ground, a half-specular sphere, a polished glass sphere (ior 1.517, absorbing), a level-1
    icosphere (80 triangles) that mixes specular, dielectric and diffuse, a stand-alone triangle of polished, partly dielectric material seen from its back, a sphere light and a two-triangle mesh
    light of a fiftieth of its radiance."""
    sc = S.ModelScene()
    mats = dict(ground=sc.material(albedo=(0.8, 0.7, 0.6)), half=sc.material(albedo=(0.7, 0.7, 0.2), specular=0.5),
                glass=sc.material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517),
                mixed=sc.material(albedo=(0.6, 0.8, 0.7), specular=0.3, refractivity=0.4, absorption=(0.1, 0.2, 0.3), ior=1.517),
                pane=sc.material(albedo=(0.8, 0.3, 0.3), specular=0.1, refractivity=0.5, absorption=(0.1, 0.1, 0.1), ior=2.0),
                lamp=sc.material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True),
                panel=sc.material(emissive=(0.2, 0.5, 1.0), intensity=0.2, is_light=True))
    objs = dict(ground=sc.plane((0, 1, 0), (0, 0, 0), mats["ground"]),
                half=sc.sphere((-1.7, 0.8, -3.0), 0.8, mats["half"]),
                glass=sc.sphere(GLASS_CENTER, GLASS_RADIUS, mats["glass"]))
    objs["mesh"] = sc.mesh(*SM.icosphere(1, MESH_CENTER, MESH_RADIUS), mats["mixed"])
    # its normal points away from the first camera: the primary rays meet it from "inside" beyond the critical angle of ior 2 (cosines below 0.866), so
    # those that draw the dielectric lobe are totally reflected with the diffuse lobe's NEE pending -- the kept ray (same_ray) at every level, since no edit roughens it
    objs["triangle"] = sc.triangle([[-3.5, 0.0, -5.5], [3.5, 0.0, -5.5], [0.0, 4.5, -5.5]], (0, 0, -1), mats["pane"])
    objs["lamp"] = sc.sphere((0.0, 5.0, -2.5), 1.0, mats["lamp"], light=True)
    quad = np.array([[-3.4, 3.0, -4.2, 0, -1, 0], [-1.6, 3.0, -4.2, 0, -1, 0], [-1.6, 3.0, -2.4, 0, -1, 0], [-3.4, 3.0, -2.4, 0, -1, 0]], np.float32)
    objs["panel"] = sc.mesh(quad, [0, 1, 2, 2, 3, 0], mats["panel"], light=True)
    return sc, dict(mats=mats, objs=objs)


def ladder(names):
    """Per level 1..4: (the edit of the ModelScene, the edit of a Renderer that holds it) -- roughness on the half-specular and the mixed
    material, transmission roughness on the mixed one (the glass sphere stays polished), smooth normals and then the transform on the mesh."""
    mats, objs = names["mats"], names["objs"]
    n_mat, n_obj, mesh = len(mats), len(objs), objs["mesh"]
    rough = np.zeros(n_mat, np.float32); rough[[mats["half"], mats["mixed"]]] = ROUGHNESS
    rough_t = np.zeros(n_mat, np.float32); rough_t[mats["mixed"]] = TRANSMISSION_ROUGHNESS
    smooth = np.zeros(n_obj, np.uint32); smooth[mesh] = 1
    matrices = np.tile(np.asarray(TR.IDENTITY, np.float32).reshape(1, 3, 4), (n_obj, 1, 1)); matrices[mesh] = MOVED

    def set_all(sc, key, values):
        for m, v in zip(sc.materials, values):
            m[key] = float(v)
    return {1: (lambda sc: set_all(sc, "roughness", rough), lambda r: r.update_roughness(rough)),
            2: (lambda sc: set_all(sc, "transmission_roughness", rough_t), lambda r: r.update_transmission_roughness(rough_t)),
            3: (lambda sc: sc.objects[mesh].update(smooth=True), lambda r: r.update_smooth_normals(smooth)),
            4: (lambda sc: sc.objects[mesh].update(transform=np.asarray(MOVED, np.float32).reshape(3, 4)), lambda r: r.update_transforms(matrices))}


def view_camera(device_scene, view):
    """The cgpt_camera of a view, from the host library."""
    device_scene.set_camera(*view["camera"])
    return device_scene.camera()


# ---- a render of a view on a context, and what a replay expects of it (test_gpu_path_replay.py, test_gpu_trace_probe.py) -------------------------
KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render_view(r, view, cam, st, kernel, counters, rows=None, interleave=None):
    """(accumulator, pixels, stats) of the view's samples on a band whose earlier samples summed to zero."""
    n_rows = H if rows is None and interleave is None else (rows[1] - rows[0] if rows else len(interleaved_rows(H, interleave[2], interleave[1], interleave[0])))
    r.reset_accumulator()
    if view["first_sample"]:
        r.load_accumulator(np.zeros((n_rows, W, 4), np.float32), view["first_sample"], W, H, rows=rows, interleave=interleave)
    r.reset_stats()
    r.render(W, H, view["n_samples"], seed=SEED, rows=rows, interleave=interleave, kernel=kernel, counters=counters, settings=st, camera=cam)
    return r.accumulator().copy(), r.pixels().copy(), r.stats()


def expected(rep, view, local_rows):
    """The replay's accumulator (the w of the earlier samples is not in it: they were loaded as zeros), pixels and counters on some rows."""
    acc = rep["accumulator"][local_rows].copy()
    return dict(acc=acc, pixels=pack_pixels(acc, view["first_sample"] + view["n_samples"]), rays=int(rep["path_rays"][local_rows].sum()),
                unwalked=int(rep["path_unwalked"][local_rows].sum()), energy=float(rep["path_energy_sum"][local_rows].sum()))


def assert_render_is(got, exp, counters, what, columns=slice(None), count=True):
    acc, pixels, stats = got
    differ = _bits(acc[:, columns]) != _bits(exp["acc"][:, columns])
    assert not differ.any(), (what, "accumulator words differ at (row, px, channel)", np.argwhere(differ)[:8].tolist(),
                              acc[:, columns][differ][:4], exp["acc"][:, columns][differ][:4])
    assert np.array_equal(pixels[:, columns], exp["pixels"][:, columns]), (what, "packed pixels")
    if count:
        assert stats.traced_rays == exp["rays"], (what, "traced_rays", stats.traced_rays, exp["rays"])
        assert stats.retrace_unwalked == (0 if counters else exp["unwalked"]), (what, "retrace_unwalked", stats.retrace_unwalked, exp["unwalked"])
        assert abs(stats.total_energy_received - exp["energy"]) <= 1e-12 * abs(exp["energy"]), (what, "total_energy_received", stats.total_energy_received, exp["energy"])
