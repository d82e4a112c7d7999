"""Scenes shared by the instancing tests (tests/test_host_instancing.py on the CPU, tests/test_gpu_instancing.py on the device): the
"grove", one cgpt_scene_desc in which several objects name the same node and triangle slices, as an editable flattened scene
(transform_scenes.Flat), with the edits both uploads of it receive."""
from __future__ import annotations

import numpy as np

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.scene import triangles_from_arrays
import smooth_ref as S
import transform_ref as T
import transform_scenes as TS

N_ICOS, N_QUADS = 6, 10                                       # 10 quads of 2 triangles: more than the 8 the 16 LDS records hold per object
ICO_TRIS = 80                                                 # a level-1 icosphere

DIFFUSE = dict(albedo=(0.8, 0.6, 0.3))
MIRROR = dict(albedo=(0.9, 0.9, 0.9), specular=1.0)
GGX = dict(albedo=(0.9, 0.8, 0.6), specular=0.8, roughness=0.3)
GLASS = dict(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517)
ROUGH_GLASS = dict(GLASS, transmission_roughness=0.3)


def quad_mesh(half=0.3):
    """(vertices 4 x 6, indices 6): a square in the plane z = 0 around the origin, facing +z: 2 triangles, a leaf-rooted tree."""
    v = np.array([[-half, -half, 0, 0, 0, 1], [half, -half, 0, 0, 0, 1], [half, half, 0, 0, 0, 1], [-half, half, 0, 0, 0, 1]], np.float32)
    return v, np.array([0, 1, 2, 2, 3, 0], np.uint32)


def _affine(a, b):
    return np.hstack([np.asarray(a, np.float64), np.asarray(b, np.float64).reshape(3, 1)]).astype(np.float32)


def _rot(axis, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


class Grove:
    """flat: the scene, objects in `order`; base: the P.Scene it was flattened from, one object per mesh (camera, settings and the
    materials' roughnesses); icos / quads / box / emitter / twin / tri / plane / lamp: object indices in flat."""

    def __init__(self):
        s = P.Scene()
        mats = {}
        mats["ground"] = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
        mats["emitter"] = s.add_material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=14.0, is_light=True))
        for name, m in (("diffuse", DIFFUSE), ("mirror", MIRROR), ("ggx", GGX), ("glass", GLASS), ("rough_glass", ROUGH_GLASS)):
            mats[name] = s.add_material(P.Material(**m))
        self.mats = mats
        plane = s.add_plane((0.0, 1.0, 0.0), (0.0, -1.5, 0.0), mats["ground"])
        lamp = s.add_sphere((0.5, 5.0, 2.0), 1.5, mats["emitter"])
        s.add_light(lamp)
        self.ico_mesh = S.icosphere(1, (0.0, 0.0, 0.0), 0.45)
        ico = s.add_mesh(P.Mesh.from_arrays(*self.ico_mesh), mats["diffuse"])
        quad = s.add_mesh(P.Mesh.from_arrays(*quad_mesh()), mats["diffuse"])
        box = s.add_mesh(P.Mesh.from_arrays(*TS.box_mesh((-0.4, -1.5, 1.2), (0.2, -0.9, 1.8))), mats["mirror"])
        emitter = s.add_mesh(P.Mesh.from_arrays(*TS.box_mesh((1.8, 0.8, -0.5), (2.2, 1.2, -0.1))), mats["emitter"])
        tri = s.add_triangle([[-2.6, -1.4, 0.8], [-1.7, -1.4, 0.9], [-2.2, -0.5, 0.6]], [[0.0, 0.3, 0.95], [0.3, 0.0, 0.95], [0.0, 0.0, 1.0]], mats["ggx"])
        s.set_camera((0.37, 2.3, 5.9), (0.02, -0.33, -1.0), 60.0, 1.0)         # off every axis: no primary ray has a zero component
        self.base = s
        f = TS.Flat(s.flatten())
        assert f.objects[ico].tri_count == ICO_TRIS and f.objects[quad].tri_count == 2 and f.objects[quad].node_count == 1
        # the instances interleaved, so that a group's members are no run of indices and a member may come long after its first
        order = [plane, lamp, ico, quad, ico, quad, ico, quad, box, ico, quad, emitter, ico, quad, quad, ico, emitter, quad, quad, quad, quad, tri]
        assert order.count(ico) == N_ICOS and order.count(quad) == N_QUADS
        base_objects = f.objects
        f.objects = [N.Object.from_buffer_copy(base_objects[k]) for k in order]
        where = lambda k: [i for i, b in enumerate(order) if b == k]
        self.icos, self.quads = where(ico), where(quad)
        self.plane, self.lamp, self.box, self.tri = where(plane)[0], where(lamp)[0], where(box)[0], where(tri)[0]
        self.emitter, self.twin = where(emitter)                               # the light, and a second object that names its slices and is no light
        f.lights = np.array([self.lamp, self.emitter], np.uint32)
        ico_mats = ["diffuse", "mirror", "glass", "ggx", "rough_glass", "diffuse"]
        for i, m in zip(self.icos, ico_mats):
            f.objects[i].mat_index = mats[m]
        for n, i in enumerate(self.quads):
            f.objects[i].mat_index = mats[("diffuse", "mirror", "ggx")[n % 3]]
        f.objects[self.twin].mat_index = mats["glass"]
        # as given: a member's total_area is its own word (the twin is no light, nothing reads it)
        f.objects[self.twin].total_area = 0.5
        self.flat = f
        self.order = order
        self.first_of_group = [order.index(b) for b in order]                 # per object: the first object naming the same base object
        self.n_groups = 4                                                      # ico, quad, box, emitter

    def unique(self):
        """The grove with one object per group (every later sharer dropped), lights renamed: what the instanced layout's array sizes
        are compared to."""
        f = TS.Flat(self.flat.desc()[0])
        keep = [i for i, first in enumerate(self.first_of_group) if first == i]
        f.objects = [f.objects[i] for i in keep]
        f.lights = np.array([keep.index(int(li)) for li in self.flat.lights], np.uint32)
        return f, keep

    def transforms(self):
        """(n_objects, 3, 4) float32: six distinct placements of the icosphere -- rotations, non-uniform scales, one mirror -- and a shift
        per quad; the twin of the emitter is moved away from it.  Planes, spheres, the light and the rest keep the identity."""
        m = np.tile(T.IDENTITY, (len(self.flat.objects), 1, 1)).astype(np.float32)
        spots = [(-2.1, -0.6, -0.4), (-1.0, -0.9, 0.9), (0.1, -0.2, -0.9), (1.2, -1.0, 0.7), (2.0, -0.3, -0.8), (0.9, 0.5, -2.2)]
        lin = [_rot(1, 30.0),
               _rot(0, 50.0) @ np.diag([1.3, 0.7, 1.0]),
               np.diag([1.0, 1.0, -1.0]),                                      # the mirror: det < 0
               _rot(2, -40.0) @ np.diag([0.8, 1.4, 1.1]),
               _rot(1, 115.0) @ _rot(0, 20.0),
               np.diag([1.5, 1.5, 0.6]) @ _rot(2, 10.0)]
        assert sum(np.linalg.det(a) < 0 for a in lin) == 1
        for i, a, b in zip(self.icos, lin, spots):
            m[i] = _affine(a, b)
        for n, i in enumerate(self.quads):
            m[i] = _affine(np.eye(3), (-2.7 + 0.6 * n, -1.1 + 0.15 * (n % 3), -2.0 + 0.1 * n))
        m[self.twin] = _affine(np.eye(3), (-4.0, -0.9, 0.4))
        return m

    def smooth(self):
        """(n_objects,) uint32: interpolated normals on two of the icosphere instances."""
        flags = np.zeros(len(self.flat.objects), np.uint32)
        flags[[self.icos[1], self.icos[4]]] = 1
        return flags

    def refit_triangles(self):
        """T': the icosphere's triangles, original order, deformed -- squashed in y, bulged in x -- with its normals kept."""
        rows = triangles_from_arrays(*self.ico_mesh).copy().reshape(-1, 3, 6)
        p = rows[:, :, 0:3]
        p[..., 0] *= np.float32(1.0) + np.float32(0.5) * p[..., 1]
        p[..., 1] *= np.float32(0.6)
        return rows.reshape(-1, 18)

    def close(self):
        self.base.close()
