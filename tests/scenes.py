"""Paired scene builders: the same scene in the oracle (checker) and in the product's host mirror."""
from __future__ import annotations

import numpy as np

import oracle as O
import cpugpupathtracing_amd as P

GROUND_V = np.array([[-1000, -3, 1000, 0, 1, 0], [-1000, -3, -1000, 0, 1, 0],
                     [1000, -3, -1000, 0, 1, 0], [1000, -3, 1000, 0, 1, 0]], np.float32)
GROUND_I = np.array([0, 1, 2, 2, 3, 0], np.uint32)

# C2 material of SURVEY 8d
MAT_SPEC_DIFFUSE = P.Material(albedo=(0.8, 0.6, 0.2), specular=0.5)


def _add_materials(o: O.OracleScene, s: P.Scene, mats):
    for m in mats:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light)
        s.add_material(m)


def reference_layout_pair(vertices, indices, mesh_material=3, aspect=1.0, build_option=O.BUILD_SAH_INTERVALS,
                          extra_materials=(), settings: P.Settings | None = None):
    """The shipped scene (ref: Main.cpp:777-819) around the given mesh, built twice."""
    o = O.OracleScene()
    s = P.Scene()
    _add_materials(o, s, list(P.REFERENCE_MATERIALS) + list(extra_materials))
    mesh = P.Mesh.from_arrays(vertices, indices)
    ground = P.Mesh.from_arrays(GROUND_V, GROUND_I)
    o.add_mesh(vertices, indices, mesh_material, build_option); s.add_mesh(mesh, mesh_material, build_option)
    o.add_mesh(GROUND_V, GROUND_I, 1, O.BUILD_SAH_INTERVALS); s.add_mesh(ground, 1, P.BUILD_SAH_INTERVALS)
    for c in ((10.0, 10.0, 10.0), (-10.0, 10.0, -10.0)):
        li = o.add_sphere(c, 5.0, 2); o.add_light(li)
        li2 = s.add_sphere(c, 5.0, 2); s.add_light(li2)
        assert li == li2
    o.set_camera((0, 0, 8), (0, 0, -1), 60.0, aspect); s.set_camera((0, 0, 8), (0, 0, -1), 60.0, aspect)
    st = settings or P.Settings()
    o.set_settings(st.max_ray_depth, st.next_event_estimation_enabled, st.cosine_weighted_diffuse_reflection_enabled,
                   st.russian_roulette_enabled)
    s.set_settings(st)
    return o, s


def standin_mesh(level: int):
    m = P.Mesh.dragon_standin(level)
    return m.vertices, m.indices


def rmse(a: np.ndarray, b: np.ndarray) -> float:
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def pair_from(objects, mats, lights, camera=((0, 0, 8), (0, 0, -1), 60.0, 1.0), settings=None):
    """The scene of `objects` -- ("mesh", vertices, indices, material, build option), ("sphere", centre, radius, material) or ("plane", normal,
    point, material) -- built twice, with `lights` the object indices of its lights."""
    o = O.OracleScene(); s = P.Scene()
    for m in mats:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light); s.add_material(m)
    for kind, *a in objects:
        if kind == "mesh":
            v, i, mat, opt = a
            o.add_mesh(v, i, mat, opt); s.add_mesh(P.Mesh.from_arrays(v, i), mat, opt)
        elif kind == "sphere":
            c, r, mat = a
            o.add_sphere(c, r, mat); s.add_sphere(c, r, mat)
        else:
            n, p, mat = a
            o.add_plane(n, p, mat); s.add_plane(n, p, mat)
    for li in lights:
        o.add_light(li); s.add_light(li)
    o.set_camera(*camera); s.set_camera(*camera)
    st = settings or P.Settings()
    o.set_settings(st.max_ray_depth, st.next_event_estimation_enabled, st.cosine_weighted_diffuse_reflection_enabled, st.russian_roulette_enabled)
    s.set_settings(st)
    return o, s


def quad_stack(n_quads, spacing=0.01, half=1.0):
    """n_quads camera-facing quads behind each other along -z: a ray down the axis crosses every node's bounds, so the ordered
    traversal pushes a far child at every level and the stack gets as deep as the tree."""
    z = -(np.arange(n_quads, dtype=np.float32) * np.float32(spacing))
    corners = np.array([[-half, -half], [half, -half], [half, half], [-half, half]], np.float32)
    v = np.zeros((n_quads, 4, 6), np.float32)
    v[:, :, 0:2] = corners[None]
    v[:, :, 2] = z[:, None]
    v[:, :, 5] = 1.0
    base = (np.arange(n_quads, dtype=np.uint32) * 4)[:, None]
    idx = (base + np.array([0, 1, 2, 2, 3, 0], np.uint32)[None]).reshape(-1)
    return v.reshape(-1, 6), idx.astype(np.uint32)


def forty_object_pair():
    """40 objects (small meshes, spheres, a plane, in mixed order): beyond the 31 object records the trace kernels mirror in LDS."""
    v, i = standin_mesh(1)
    grey, light, mirror = P.Material(albedo=(0.6, 0.6, 0.6)), P.Material(emissive=(1, 1, 1), intensity=4.0, is_light=True), P.Material(albedo=(0.9, 0.9, 0.9), specular=0.7)
    objs = []
    rng = np.random.default_rng(5)
    for k in range(38):
        c = (float(rng.uniform(-9, 9)), float(rng.uniform(-2, 6)), float(rng.uniform(-12, 0)))
        if k % 3 == 0:
            vv = v.copy(); vv[:, :3] = vv[:, :3] * np.float32(0.15) + np.array(c, np.float32)
            objs.append(("mesh", vv, i, 2 if k % 2 else 0, O.BUILD_SAH_INTERVALS))
        else:
            objs.append(("sphere", c, float(rng.uniform(0.3, 0.9)), 2 if k % 4 == 1 else 0))
    objs.append(("plane", (0, 1, 0), (0, -3, 0), 0))
    objs.append(("sphere", (0, 14, 2), 4.0, 1))
    return pair_from(objs, [grey, light, mirror], [39])
