"""Scenes shared by the transform tests (tests/test_host_transforms.py on the CPU, tests/test_gpu_transforms.py on the device): the
axis-aligned box world S0 of the exact comparison and its stored-flipped twin S1, as editable flattened scenes."""
from __future__ import annotations

import ctypes as C

import numpy as np

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import transform_ref as T

IDENTITY12 = T.IDENTITY.reshape(12)


def box_mesh(lo, hi):
    """(vertices 24 x 6, indices 36): an axis-aligned box, outward winding, every vertex normal its face's normal (zeros stored as +0)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v, idx = [], []
    for ax in range(3):
        for side in (0, 1):
            n = np.zeros(3); n[ax] = 1.0 if side else -1.0
            a, b = (ax + 1) % 3, (ax + 2) % 3
            corners = []
            for ca, cb in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = np.zeros(3)
                p[ax] = hi[ax] if side else lo[ax]
                p[a] = hi[a] if ca else lo[a]
                p[b] = hi[b] if cb else lo[b]
                corners.append(p)
            if not side:
                corners.reverse()
            base = len(v)
            v += [np.concatenate([p, n + 0.0]) for p in corners]
            idx += [base, base + 1, base + 2, base + 2, base + 3, base]
    return np.array(v, np.float32), np.array(idx, np.uint32)


def merge(meshes):
    vs, is_, base = [], [], 0
    for v, i in meshes:
        vs.append(v); is_.append(i + base); base += v.shape[0]
    return np.concatenate(vs), np.concatenate(is_).astype(np.uint32)


def terrain(n=8, seed=3):
    """n x n box columns of seeded heights over [-2, 2]^2, their feet at y = -1: 12 n^2 triangles."""
    rng = np.random.default_rng(seed)
    step = 4.0 / n
    cols = []
    for ix in range(n):
        for iz in range(n):
            h = -0.9 + 0.05 * rng.integers(0, 12)
            cols.append(box_mesh((-2.0 + ix * step, -1.0, -2.0 + iz * step), (-2.0 + (ix + 1) * step, h, -2.0 + (iz + 1) * step)))
    return merge(cols)


BOX_MESHES = 3                                                                # objects 2, 3, 4 of box_world


def box_world(settings=None, size=64):
    """S0: a plane under a sphere light, the diffuse terrain, a mirror box and a glass box.  Returns (scene, [mesh object indices])."""
    s = P.Scene()
    ground = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=14.0, is_light=True))
    diffuse = s.add_material(P.Material(albedo=(0.8, 0.6, 0.3)))
    mirror = s.add_material(P.Material(albedo=(0.9, 0.9, 0.9), specular=1.0))
    glass = s.add_material(P.Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -1.5, 0.0), ground)
    lamp = s.add_sphere((0.5, 5.0, 2.0), 1.5, emitter)
    s.add_light(lamp)
    meshes = [s.add_mesh(P.Mesh.from_arrays(*terrain()), diffuse),
              s.add_mesh(P.Mesh.from_arrays(*box_mesh((-1.7, -0.2, -0.9), (-0.6, 0.9, 0.1))), mirror),
              s.add_mesh(P.Mesh.from_arrays(*box_mesh((0.5, -0.1, -0.4), (1.6, 1.0, 0.7))), glass)]
    s.set_camera((0.37, 2.3, 5.9), (0.02, -0.33, -1.0), 60.0, 1.0)             # off every axis: no primary ray has a zero component
    if settings is not None:
        s.set_settings(settings)
    return s, meshes


class Flat:
    """An owned, editable copy of a flattened scene (cgpt_scene_desc)."""

    def __init__(self, desc):
        u32 = lambda p, n, w: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n, w)).copy()
        self.objects = [N.Object.from_buffer_copy(desc.objects[i]) for i in range(desc.n_objects)]
        self.nodes = u32(desc.nodes, desc.n_nodes, 8)
        self.tris = u32(desc.triangles, desc.n_triangles, 18).view(np.float32)
        self.tidx = u32(desc.tri_indices, desc.n_triangles, 1).ravel()
        self.materials = [N.Material.from_buffer_copy(desc.materials[i]) for i in range(desc.n_materials)]
        self.lights = np.array([desc.light_indices[i] for i in range(desc.n_lights)], np.uint32)

    def desc(self):
        """(cgpt_scene_desc, the arrays it points into: keep them alive while it is used)"""
        objs = (N.Object * len(self.objects))(*self.objects)
        mats = (N.Material * len(self.materials))(*self.materials)
        nodes, tris, tidx, lights = (np.ascontiguousarray(a) for a in (self.nodes, self.tris, self.tidx, self.lights))
        d = N.SceneDesc()
        d.objects = objs; d.n_objects = len(self.objects)
        d.nodes = nodes.ctypes.data_as(C.POINTER(N.BvhNode)); d.n_nodes = nodes.shape[0]
        d.triangles = tris.ctypes.data_as(C.POINTER(N.Triangle)); d.n_triangles = tris.shape[0]
        d.tri_indices = tidx.ctypes.data_as(C.POINTER(C.c_uint32))
        d.materials = mats; d.n_materials = len(self.materials)
        d.light_indices = lights.ctypes.data_as(C.POINTER(C.c_uint32)); d.n_lights = lights.size
        return d, (objs, mats, nodes, tris, tidx, lights)


def stored_flipped(scene, meshes, flip):
    """S1's geometry: the flattened `scene` with the triangles and trees of `meshes` under the sign flip `flip` (its own inverse), and the
    transforms that bring them back: (Flat, (n_objects, 12) float32)."""
    f = Flat(scene.flatten())
    s = np.diag(np.asarray(flip, np.float32).reshape(3, 4)[:, :3]).astype(np.float32)
    m = np.tile(IDENTITY12, (len(f.objects), 1))
    for oi in meshes:
        o = f.objects[oi]
        t = f.tris[o.tri_offset:o.tri_offset + o.tri_count].reshape(-1, 6, 3)
        t *= s
        t += np.float32(0.0)                                                  # a flipped zero is +0
        f.nodes[o.node_offset:o.node_offset + o.node_count] = T.flip_nodes(f.nodes[o.node_offset:o.node_offset + o.node_count], flip).view(np.uint32)
        m[oi] = np.asarray(flip, np.float32).reshape(12)
    return f, m
