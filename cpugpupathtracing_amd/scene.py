"""Python handles on the host mirror (include/cpugpupt_host.h): Mesh, Scene, materials, camera, settings.

Names follow the reference (ref: Source/Main.cpp:51-69 Material, :94-170 Camera, :228-235 Settings, :245-275 Object;
Include/Primitives.h:24-28 Mesh).  All work (glTF parsing, BVH build, flattening) happens in the C++ library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Sequence, Tuple

import numpy as np

from . import _native as N


class HostError(RuntimeError):
    pass


def _host_check(rc: int, what: str):
    if rc != 0:
        raise HostError(f"{what}: {N.lib().cgpth_last_error().decode()}")


def _f3(v: Sequence[float]):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


@dataclass
class Material:
    """ref: Source/Main.cpp:51-69, plus the specular lobe's roughness in [0, 1] (0: the reference's mirror; > 0: GGX reflection with
    alpha = roughness^2, cgpt_scene_update_roughness) and the dielectric lobe's transmission roughness in [0, 1] (0: the reference's
    polished glass; > 0: GGX refraction with alpha_t = transmission_roughness^2, cgpt_scene_update_transmission_roughness).  to_abi()
    carries neither: the Scene forwards them through the host mirror."""
    albedo: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    specular: float = 0.0
    refractivity: float = 0.0
    absorption: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    ior: float = 1.0
    emissive: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    intensity: float = 0.0
    is_light: bool = False
    roughness: float = 0.0
    transmission_roughness: float = 0.0

    def to_abi(self) -> N.Material:
        m = N.Material()
        m.albedo = _f3(self.albedo); m.specular = self.specular; m.refractivity = self.refractivity
        m.absorption = _f3(self.absorption); m.ior = self.ior; m.emissive = _f3(self.emissive)
        m.intensity = self.intensity; m.is_light = 1 if self.is_light else 0
        return m


@dataclass
class Settings:
    """ref: Source/Main.cpp:228-235 plus render_mode / debug_render_mode (:215-216)"""
    max_ray_depth: int = 5
    next_event_estimation_enabled: bool = True
    cosine_weighted_diffuse_reflection_enabled: bool = True
    russian_roulette_enabled: bool = True
    render_mode: int = N.MODE_ADVANCED
    debug_render_mode: int = N.DEBUG_NONE

    def to_abi(self) -> N.Settings:
        return N.Settings(self.max_ray_depth, int(self.next_event_estimation_enabled),
                          int(self.cosine_weighted_diffuse_reflection_enabled), int(self.russian_roulette_enabled),
                          self.render_mode, self.debug_render_mode)


# the four materials of the shipped scene (ref: Main.cpp:779-782)
REFERENCE_MATERIALS = (
    Material(albedo=(0.2, 0.2, 0.8)),
    Material(albedo=(1.0, 1.0, 1.0)),
    Material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True),
    Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517),
)


def triangles_from_arrays(vertices, indices) -> np.ndarray:
    """The cgpt_triangle array (n x 18 float32: v0, v1, v2, each pos.xyz + normal.xyz, 72 bytes a row) of a mesh given as vertices
    (m x 6: pos.xyz, normal.xyz) and indices (3n), in the mesh's original triangle order -- what Mesh + BVH::Build turn into
    m_triangles (ref: Source/BVH.cpp:15-20) and what refit_mesh takes."""
    v = np.ascontiguousarray(vertices, dtype=np.float32)
    i = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
    if v.ndim != 2 or v.shape[1] != 6 or i.size % 3:
        raise ValueError("vertices must be m x 6 (pos, normal) and indices a multiple of 3")
    if i.size and int(i.max()) >= v.shape[0]:
        raise ValueError("index out of range")
    return np.ascontiguousarray(v[i].reshape(-1, 18))


def _triangle_rows(triangles) -> np.ndarray:
    t = np.ascontiguousarray(triangles, dtype=np.float32)
    if t.ndim < 1 or t.size % 18:
        raise ValueError("triangles must hold 18 floats per triangle (see triangles_from_arrays)")
    return t.reshape(-1, 18)


def _triangle_ptr(rows: np.ndarray):
    return rows.ctypes.data_as(C.POINTER(N.Triangle))


def _skin_arrays(bind_triangles, joints, weights):
    """A skin as the library takes it: (n, 18) float32 bind triangles, 12 n uint16 joint indices, 12 n float32 weights."""
    rows = _triangle_rows(bind_triangles)
    j = np.ascontiguousarray(joints)
    if j.dtype != np.uint16:
        if j.size and (j.min() < 0 or j.max() > 0xFFFF):
            raise ValueError("joint indices must fit uint16")
        j = j.astype(np.uint16)
    j = np.ascontiguousarray(j.ravel())
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if j.size != 12 * rows.shape[0] or w.size != 12 * rows.shape[0]:
        raise ValueError("joints and weights hold 12 entries per triangle: four per corner")
    return rows, j, w


def _joint_matrices(matrices) -> np.ndarray:
    m = np.ascontiguousarray(matrices, dtype=np.float32)
    if m.size % 12:
        raise ValueError("joint matrices are (n_joints, 3, 4) or (n_joints, 12)")
    return m.reshape(-1, 12)


def skin_triangles(bind_triangles, joints, weights, matrices) -> np.ndarray:
    """Linear blend skinning on the host (cgpth_skin_triangles): the (n, 18) float32 triangles of the pose.
    bind_triangles: (n, 18) as triangles_from_arrays returns them; joints / weights: (n, 3, 4) -- four influences per corner;
    matrices: (n_joints, 3, 4) or (n_joints, 12) float32, the rows of [A | b] of each joint's object-space skinning matrix.
    It is what Renderer.skin_mesh computes on the device, to the bit."""
    rows, j, w = _skin_arrays(bind_triangles, joints, weights)
    m = _joint_matrices(matrices)
    out = np.empty_like(rows)
    _host_check(N.lib().cgpth_skin_triangles(_triangle_ptr(rows), j.ctypes.data_as(C.POINTER(C.c_uint16)), w.ctypes.data_as(C.POINTER(C.c_float)),
                                             rows.shape[0], m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], _triangle_ptr(out)), "skin_triangles")
    return out


def _morph_arrays(base_triangles, deltas, weights=None):
    """Morph targets as the library takes them: (n, 18) float32 base triangles, (n_targets, n, 18) float32 deltas, n_targets weights."""
    rows = _triangle_rows(base_triangles)
    d = np.ascontiguousarray(deltas, dtype=np.float32)
    if rows.shape[0] == 0 or d.size % rows.size:
        raise ValueError("deltas are (n_targets, n_tris, 18): one record per base triangle and target")
    d = d.reshape(d.size // rows.size, rows.shape[0], 18)
    if weights is None:
        return rows, d
    return rows, d, _morph_weights(weights, d.shape[0])


def _morph_weights(weights, n_targets=None) -> np.ndarray:
    w = np.ascontiguousarray(weights, dtype=np.float32).ravel()
    if n_targets is not None and w.size != n_targets:
        raise ValueError(f"{n_targets} targets take {n_targets} weights, got {w.size}")
    return w


def morph_triangles(base_triangles, deltas, weights) -> np.ndarray:
    """Morph targets on the host (cgpth_morph_triangles): the (n, 18) float32 triangles of the pose.
    base_triangles: (n, 18) as triangles_from_arrays returns them; deltas: (n_targets, n, 18) displacements in the same layout (per corner
    a position delta and a normal delta); weights: n_targets float32, used as given, a zero of either sign skipped.
    It is what Renderer.morph_mesh computes on the device, to the bit; the bind pose of a skin that follows it."""
    rows, d, w = _morph_arrays(base_triangles, deltas, weights)
    out = np.empty_like(rows)
    _host_check(N.lib().cgpth_morph_triangles(_triangle_ptr(rows), _triangle_ptr(d), rows.shape[0], d.shape[0], w.ctypes.data_as(C.POINTER(C.c_float)),
                                              _triangle_ptr(out)), "morph_triangles")
    return out


def _skeleton_desc(parents, inverse_bind, rest, root=None):
    """cgpt_skeleton_desc and the arrays it points into: parents n int32, inverse_bind (n, 12) or (n, 3, 4), rest (n, 10) float32
    {T.xyz, R.xyzw, S.xyz}, root None or 12 floats."""
    par = np.ascontiguousarray(parents, np.int32).ravel()
    ib = np.ascontiguousarray(inverse_bind, np.float32).reshape(-1, 12)
    rs = np.ascontiguousarray(rest, np.float32).reshape(-1, 10)
    if ib.shape[0] != par.size or rs.shape[0] != par.size:
        raise ValueError("a skeleton has one parent, 12 inverse bind floats and 10 rest floats per joint")
    rt = None if root is None else np.ascontiguousarray(root, np.float32).reshape(12)
    fp = C.POINTER(C.c_float)
    desc = N.SkeletonDesc(par.ctypes.data_as(C.POINTER(C.c_int32)), ib.ctypes.data_as(fp), rs.ctypes.data_as(fp),
                          None if rt is None else rt.ctypes.data_as(fp), par.size)
    return desc, (par, ib, rs, rt)


def _clip_desc(n_joints, channels, times, values):
    """cgpt_clip_desc and the arrays it points into: channels rows of six words {joint, path, interpolation, n_keys, first_time,
    first_value} (N.ANIM_*), times and values float32."""
    ch = np.ascontiguousarray(channels, np.uint32).reshape(-1, 6)
    t = np.ascontiguousarray(times, np.float32).ravel()
    v = np.ascontiguousarray(values, np.float32).ravel()
    fp = C.POINTER(C.c_float)
    desc = N.ClipDesc(int(n_joints), ch.shape[0], ch.ctypes.data_as(C.POINTER(N.ClipChannel)), t.ctypes.data_as(fp), t.size, v.ctypes.data_as(fp), v.size)
    return desc, (ch, t, v)


def animate_joints(skeleton, clip, time) -> np.ndarray:
    """Joint matrices from an animation clip on the host (cgpth_animate_joints): the (n_joints, 12) float32 matrices
    of skeleton = (parents, inverse_bind, rest[, root]) under clip = (n_joints, channels, times, values) at `time` -- sampled (STEP,
    LINEAR; rotations by normalised lerp), composed up the hierarchy, times the inverse bind matrices.  It is what
    Renderer.animate_objects computes on the device, to the bit, and what Renderer.pose_objects takes."""
    sd, keep_s = _skeleton_desc(*skeleton)
    cd, keep_c = _clip_desc(*clip)
    out = np.empty((sd.n_joints, 12), np.float32)
    rc = N.lib().cgpth_animate_joints(C.byref(sd), C.byref(cd), float(time), out.ctypes.data_as(C.POINTER(C.c_float)), sd.n_joints)
    if rc != 0:
        e = HostError(f"animate_joints: {N.lib().cgpth_last_error().decode()}")
        e.code = rc
        raise e
    return out


def _host_error(rc, what):
    e = HostError(f"{what}: {N.lib().cgpth_last_error().decode()}")
    e.code = rc
    return e


def animate_layers(skeleton, layers) -> np.ndarray:
    """Joint matrices from a blend of clips on the host (cgpth_animate_layers): `layers` is a sequence of 1 .. 4
    (clip, time, weight, wrap) with clip = (n_joints, channels, times, values) and wrap one of N.ANIM_WRAP_*.  Each layer's time is
    wrapped over its clip's range, layers of weight 0 are left out, the others' T / R / S are blended by their weights over the
    weights' sum before the hierarchy is walked.  It is what Renderer.animate_layers computes on the device, to the bit."""
    sd, keep_s = _skeleton_desc(*skeleton)
    layers = list(layers)
    descs, keep = [], []
    for clip, _, _, _ in layers:
        cd, keep_c = _clip_desc(*clip)
        descs.append(cd); keep.append(keep_c)
    clips = (N.ClipDesc * max(1, len(descs)))(*descs)
    rows = (N.ClipLayer * max(1, len(layers)))(*[N.ClipLayer(0, float(t), float(w), int(wrap)) for _, t, w, wrap in layers])
    out = np.empty((sd.n_joints, 12), np.float32)
    rc = N.lib().cgpth_animate_layers(C.byref(sd), clips, rows, len(layers), out.ctypes.data_as(C.POINTER(C.c_float)), sd.n_joints)
    if rc != 0:
        raise _host_error(rc, "animate_layers")
    return out


def clip_range(clip):
    """(begin, end) of clip = (n_joints, channels, times, values) as float32: the smallest first-key and the largest last-key time of
    its channels, (0, 0) without channels (cgpth_clip_range) -- what a layer's LOOP or PINGPONG wraps its time over."""
    cd, keep = _clip_desc(*clip)
    b, e = C.c_float(), C.c_float()
    rc = N.lib().cgpth_clip_range(C.byref(cd), C.byref(b), C.byref(e))
    if rc != 0:
        raise _host_error(rc, "clip_range")
    return np.float32(b.value), np.float32(e.value)


def wrap_time(t, begin, end, wrap):
    """cgpth_wrap_time: `t` over [begin, end] by N.ANIM_WRAP_CLAMP (as given), _LOOP or _PINGPONG, in float32 as the device call wraps it."""
    out = C.c_float()
    rc = N.lib().cgpth_wrap_time(float(t), float(begin), float(end), int(wrap), C.byref(out))
    if rc != 0:
        raise _host_error(rc, "wrap_time")
    return np.float32(out.value)


def tree_cost(nodes, c_inner: float = 1.0, c_tri: float = 1.0) -> N.TreeCost:
    """cgpth_tree_cost: the surface-area cost of the tree in `nodes`, (n, 8) uint32 words as Scene.bvh_export and Renderer.export_bvh
    return them: .cost, .root_half_area, .n_inner, .n_leaves, .max_leaf_tris.  It is what Renderer.tree_costs sums
    on the device, to rounding."""
    n = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    out = N.TreeCost()
    rc = N.lib().cgpth_tree_cost(n.ctypes.data_as(C.POINTER(N.BvhNode)), n.shape[0], float(c_inner), float(c_tri), C.byref(out))
    if rc != 0:
        raise _host_error(rc, "tree_cost")
    return out


def primitive_abi(kind: int, mat_index: int, center=None, radius=None, normal=None, point=None) -> N.Object:
    """A cgpt_object for update_primitive: a sphere (center, radius) or a plane (normal, point)."""
    o = N.Object()
    o.kind, o.mat_index = kind, mat_index
    if kind == N.OBJECT_SPHERE:
        if center is None or radius is None:
            raise ValueError("a sphere takes center and radius")
        o.sphere_center = _f3(center); o.sphere_radius = float(radius)
    elif kind == N.OBJECT_PLANE:
        if normal is None or point is None:
            raise ValueError("a plane takes normal and point")
        o.plane_normal = _f3(normal); o.plane_point = _f3(point)
    else:
        raise ValueError(f"update_primitive edits spheres and planes, not kind {kind}")
    return o


class Mesh:
    """ref: Include/Primitives.h:24-28; vertices = n x (pos.xyz, normal.xyz) float32, indices uint32"""

    def __init__(self, handle):
        if not handle:
            raise HostError(N.lib().cgpth_last_error().decode())
        self._h = C.c_void_p(handle)

    @classmethod
    def load_gltf(cls, path: str) -> "Mesh":
        """GLTFLoader::Load (ref: Source/GLTFLoader.cpp:19-89)"""
        return cls(N.lib().cgpth_mesh_load_gltf(path.encode()))

    @classmethod
    def from_arrays(cls, vertices, indices) -> "Mesh":
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        i = np.ascontiguousarray(indices, dtype=np.uint32).ravel()
        assert v.ndim == 2 and v.shape[1] == 6
        return cls(N.lib().cgpth_mesh_from_arrays(v.ctypes.data_as(C.POINTER(N.Vertex)), v.shape[0],
                                                  i.ctypes.data_as(C.POINTER(C.c_uint32)), i.size))

    @classmethod
    def dragon_standin(cls, level: int) -> "Mesh":
        return cls(N.lib().cgpth_mesh_dragon_standin(level))

    @classmethod
    def bumpy_icosphere(cls, level: int, center, radii, bump: float) -> "Mesh":
        return cls(N.lib().cgpth_mesh_bumpy_icosphere(level, _f3(center), _f3(radii), bump))

    def save_gltf(self, path: str):
        _host_check(N.lib().cgpth_mesh_save_gltf(self._h, path.encode()), "save_gltf")

    @property
    def vertices(self) -> np.ndarray:
        L = N.lib()
        n = L.cgpth_mesh_num_vertices(self._h)
        if n == 0:
            return np.zeros((0, 6), np.float32)
        p = C.cast(L.cgpth_mesh_vertices(self._h), C.POINTER(C.c_float))
        return np.ctypeslib.as_array(p, shape=(n, 6)).copy()

    @property
    def indices(self) -> np.ndarray:
        L = N.lib()
        n = L.cgpth_mesh_num_indices(self._h)
        if n == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(L.cgpth_mesh_indices(self._h), shape=(n,)).copy()

    @property
    def num_triangles(self) -> int:
        return N.lib().cgpth_mesh_num_indices(self._h) // 3

    def close(self):
        if self._h:
            N.lib().cgpth_mesh_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """The parts of the reference's `data` that Render() reads (ref: Main.cpp:209-216,228-235)."""

    def __init__(self, handle=None):
        L = N.lib()
        self._h = C.c_void_p(handle if handle else L.cgpth_scene_new())
        if not self._h:
            raise HostError(L.cgpth_last_error().decode())

    @classmethod
    def reference_layout(cls, mesh: Mesh, mesh_material: int = 3, aspect: float = 16.0 / 9.0,
                         build_option: int = N.BUILD_SAH_INTERVALS) -> "Scene":
        """The shipped scene (ref: Main.cpp:777-819) with `mesh` in place of the dragon."""
        h = N.lib().cgpth_scene_reference_layout(mesh._h, mesh_material, aspect, build_option)
        if not h:
            raise HostError(N.lib().cgpth_last_error().decode())
        return cls(h)

    def add_material(self, m: Material) -> int:
        if not 0.0 <= m.roughness <= 1.0:               # (NaN fails too) refused before the material is added
            raise HostError(f"add_material: roughness {m.roughness} outside [0, 1]")
        if not 0.0 <= m.transmission_roughness <= 1.0:
            raise HostError(f"add_material: transmission_roughness {m.transmission_roughness} outside [0, 1]")
        abi = m.to_abi()
        rc = N.lib().cgpth_scene_add_material(self._h, C.byref(abi))
        if rc < 0:
            raise HostError(N.lib().cgpth_last_error().decode())
        if m.roughness != 0.0:
            self.set_roughness(rc, m.roughness)
        if m.transmission_roughness != 0.0:
            self.set_transmission_roughness(rc, m.transmission_roughness)
        return rc

    def set_material(self, index: int, m: Material):
        """The whole material, both roughnesses included."""
        if not 0.0 <= m.roughness <= 1.0:
            raise HostError(f"set_material: roughness {m.roughness} outside [0, 1]")
        if not 0.0 <= m.transmission_roughness <= 1.0:
            raise HostError(f"set_material: transmission_roughness {m.transmission_roughness} outside [0, 1]")
        abi = m.to_abi()
        _host_check(N.lib().cgpth_scene_set_material(self._h, index, C.byref(abi)), "set_material")
        self.set_roughness(index, m.roughness)
        self.set_transmission_roughness(index, m.transmission_roughness)

    def set_roughness(self, index: int, roughness: float):
        """The specular lobe's roughness of material `index` (cgpth_scene_set_roughness)."""
        _host_check(N.lib().cgpth_scene_set_roughness(self._h, index, float(roughness)), "set_roughness")

    def roughness(self, n_materials=None) -> np.ndarray:
        """Every material's roughness, float32 (cgpth_scene_get_roughness).  n_materials: the scene's count when the caller has it."""
        n = self.flatten().n_materials if n_materials is None else n_materials
        out = np.zeros(n, np.float32)
        _host_check(N.lib().cgpth_scene_get_roughness(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n), "get_roughness")
        return out

    def set_transmission_roughness(self, index: int, transmission_roughness: float):
        """The dielectric lobe's transmission roughness of material `index` (cgpth_scene_set_transmission_roughness)."""
        _host_check(N.lib().cgpth_scene_set_transmission_roughness(self._h, index, float(transmission_roughness)), "set_transmission_roughness")

    def transmission_roughness(self, n_materials=None) -> np.ndarray:
        """Every material's transmission roughness, float32 (cgpth_scene_get_transmission_roughness)."""
        n = self.flatten().n_materials if n_materials is None else n_materials
        out = np.zeros(n, np.float32)
        _host_check(N.lib().cgpth_scene_get_transmission_roughness(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n), "get_transmission_roughness")
        return out

    def set_smooth_normals(self, obj_index: int, smooth: bool):
        """Smooth shading of object `obj_index` (cgpth_scene_set_smooth_normals): True interpolates the hit triangle's three vertex
        normals, False is the reference's flat v0.normal.  Spheres and planes ignore it; a light refuses True."""
        _host_check(N.lib().cgpth_scene_set_smooth_normals(self._h, obj_index, 1 if smooth else 0), "set_smooth_normals")

    def smooth_normals(self, n_objects=None) -> np.ndarray:
        """Every object's smooth-normal flag, uint32 (cgpth_scene_get_smooth_normals).  n_objects: the scene's count when the caller has it."""
        n = self.flatten().n_objects if n_objects is None else n_objects
        out = np.zeros(n, np.uint32)
        _host_check(N.lib().cgpth_scene_get_smooth_normals(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n), "get_smooth_normals")
        return out

    def set_transform(self, obj_index: int, m):
        """The object-to-world matrix of object `obj_index` (cgpth_scene_set_transform): 12 floats, the rows of [A | b]
        (a 3x4 array), so that world = A p + b.  Meshes and triangle objects; a sphere, a plane or a light takes the identity only."""
        v = np.ascontiguousarray(m, np.float32).reshape(12)
        _host_check(N.lib().cgpth_scene_set_transform(self._h, obj_index, v.ctypes.data_as(C.POINTER(C.c_float))), "set_transform")

    def transforms(self, n_objects=None) -> np.ndarray:
        """Every object's object-to-world matrix, float32 (n, 3, 4) (cgpth_scene_get_transforms)."""
        n = self.flatten().n_objects if n_objects is None else n_objects
        out = np.zeros((n, 3, 4), np.float32)
        _host_check(N.lib().cgpth_scene_get_transforms(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), n), "get_transforms")
        return out

    def top_level(self, transforms=None):
        """The top-level tree an upload of this scene builds (cgpth_top_level), with the scene's own transforms or the
        given ones: (nodes (2 n - 1, 8) float32 in preorder, {lo.xyz, bits(skip) | hi.xyz, bits(object or 0xFFFFFFFF)}, entry (n + 1,)
        uint32).  Host only."""
        L = N.lib()
        desc = self.flatten()
        view = N.TopLevelView()
        _host_check(L.cgpth_top_level(C.byref(desc), C.byref(view)), "top_level")
        m = np.ascontiguousarray(self.transforms(desc.n_objects) if transforms is None else transforms, np.float32).reshape(-1, 12)
        _host_check(L.cgpth_top_level_transforms(m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0], C.byref(view)), "top_level")
        nodes = np.ctypeslib.as_array(view.nodes, shape=(view.n_nodes, 8)).copy()
        entry = np.ctypeslib.as_array(view.entry, shape=(view.n_entry,)).copy()
        return nodes, entry

    def world_boxes(self) -> np.ndarray:
        """Every object's padded world box (n, 6) float32 {lo.xyz, hi.xyz}: the leaves of top_level().  A plane's is (-inf, +inf)."""
        nodes, _ = self.top_level()
        obj = nodes[:, 7].view(np.uint32)
        leaf = obj != 0xFFFFFFFF
        out = np.zeros((int(leaf.sum()), 6), np.float32)
        out[obj[leaf]] = nodes[leaf][:, [0, 1, 2, 4, 5, 6]]
        return out

    def sort_objects_spatially(self) -> np.ndarray:
        """Reorders the objects along a Morton curve through their world-box centres (10 bits per axis over the centres' bounds;
        planes and other unbounded objects first, ties in the old order), so that the index ranges of the top-level tree
        (Renderer.set_top_level) are compact in space.  Light indices, smooth flags and transforms follow their objects.
        Returns `order`: the new object k is the old object order[k] -- indices the caller holds must be renamed.
        It is the caller's choice because it CHANGES THE TIE ORDER: where two objects' surfaces lie at exactly the same distance along
        a ray, the lower object index wins, so coincident surfaces may render with the other object's material afterwards."""
        boxes = self.world_boxes().astype(np.float64)
        n = boxes.shape[0]
        finite = np.isfinite(boxes).all(-1)
        key = np.zeros(n, np.uint64)                                  # unbounded objects keep key 0 and come first
        if finite.any():
            c = 0.5 * (boxes[finite, :3] + boxes[finite, 3:])
            lo, hi = c.min(0), c.max(0)
            q = np.floor((c - lo) / np.where(hi > lo, hi - lo, 1.0) * 1023.0 + 0.5).astype(np.uint64)
            code = np.zeros(q.shape[0], np.uint64)
            for bit in range(10):
                for axis in range(3):
                    code |= ((q[:, axis] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + axis)
            key[finite] = code + np.uint64(1)
        order = np.argsort(key, kind="stable").astype(np.uint32)
        _host_check(N.lib().cgpth_scene_permute_objects(self._h, order.ctypes.data_as(C.POINTER(C.c_uint32)), n), "sort_objects_spatially")
        return order

    def add_mesh(self, mesh: Mesh, mat_index: int, build_option: int = N.BUILD_SAH_INTERVALS, device_builder=None, smooth: bool = False,
                 transform=None) -> int:
        """Object ctor (ref: Main.cpp:247-251).  device_builder: a Renderer whose GPU builds the (bit-identical) tree, any option.
        build_option: BUILD_NAIVE, BUILD_SAH_INTERVALS (the reference's default), BUILD_SAH_PRIMITIVES or BUILD_SAH_BINNED.
        smooth: shade with interpolated vertex normals (set_smooth_normals).  transform: the object-to-world matrix (set_transform)."""
        if device_builder is not None:
            rc = N.lib().cgpth_scene_add_mesh_device_built_ex(self._h, mesh._h, mat_index, device_builder._ctx, build_option)
        else:
            rc = N.lib().cgpth_scene_add_mesh(self._h, mesh._h, mat_index, build_option)
        if rc < 0:
            raise HostError(N.lib().cgpth_last_error().decode())
        if smooth:
            self.set_smooth_normals(rc, True)
        if transform is not None:
            self.set_transform(rc, transform)
        return rc

    def add_instance(self, obj_index: int, mat_index: int, transform=None, smooth: bool = False) -> int:
        """An instance of mesh object `obj_index` (cgpth_scene_add_instance): a new mesh object that shares that object's
        triangles and BVH -- one device copy under Renderer.upload(instanced=True) -- with its own material, transform and smooth flag.
        refit_mesh and rebuild_bvh through either index act on the shared tree.  Spheres, planes and triangle objects are refused.
        Returns the object index."""
        rc = N.lib().cgpth_scene_add_instance(self._h, obj_index, mat_index)
        if rc < 0:
            raise HostError(N.lib().cgpth_last_error().decode())
        if smooth:
            self.set_smooth_normals(rc, True)
        if transform is not None:
            self.set_transform(rc, transform)
        return rc

    def has_instances(self, desc=None) -> bool:
        """Two mesh objects of the flattened scene name the same node and triangle slices (add_instance makes such objects)."""
        desc = self.flatten() if desc is None else desc
        seen = set()
        for k in range(desc.n_objects):
            o = desc.objects[k]
            if o.kind == N.OBJECT_MESH:
                key = (o.node_offset, o.node_count, o.tri_offset, o.tri_count)
                if key in seen:
                    return True
                seen.add(key)
        return False

    def add_sphere(self, center, radius: float, mat_index: int) -> int:
        return N.lib().cgpth_scene_add_sphere(self._h, _f3(center), radius, mat_index)

    def add_plane(self, normal, point, mat_index: int) -> int:
        return N.lib().cgpth_scene_add_plane(self._h, _f3(normal), _f3(point), mat_index)

    def add_triangle(self, positions, normals, mat_index: int, smooth: bool = False) -> int:
        """Primitive(const Triangle&) (ref: Include/Primitives.h:84-89): a stand-alone triangle object without a BVH.
        positions: 3x3 (v0, v1, v2); normals: 3x3 per vertex, or one normal for all three.  The shading normal is v0's
        (ref: Primitives.cpp:148-151), or with smooth=True the three interpolated (set_smooth_normals).  Returns the object index."""
        p = np.asarray(positions, dtype=np.float32).reshape(3, 3)
        n = np.asarray(normals, dtype=np.float32)
        n = np.broadcast_to(n.reshape(3), (3, 3)) if n.size == 3 else n.reshape(3, 3)
        tri = N.Triangle()
        for k, v in enumerate((tri.v0, tri.v1, tri.v2)):
            v.pos = _f3(p[k]); v.normal = _f3(n[k])
        rc = N.lib().cgpth_scene_add_triangle(self._h, C.byref(tri), mat_index)
        if rc < 0:
            raise HostError(N.lib().cgpth_last_error().decode())
        if smooth:
            self.set_smooth_normals(rc, True)
        return rc

    def add_light(self, obj_index: int):
        _host_check(N.lib().cgpth_scene_add_light(self._h, obj_index), "add_light")

    def set_camera(self, pos, view_dir, fov_deg: float, aspect: float):
        _host_check(N.lib().cgpth_scene_set_camera(self._h, _f3(pos), _f3(view_dir), fov_deg, aspect), "set_camera")

    def set_settings(self, s: Settings):
        abi = s.to_abi()
        _host_check(N.lib().cgpth_scene_set_settings(self._h, C.byref(abi)), "set_settings")

    def rebuild_bvh(self, obj_index: int, build_option: int, device_builder=None):
        """BVH::Rebuild (ref: BVH.cpp:47-59): re-split over the CURRENT triangle order; device_builder: a Renderer whose GPU does it."""
        if device_builder is not None:
            _host_check(N.lib().cgpth_scene_rebuild_bvh_device(self._h, obj_index, build_option, device_builder._ctx), "rebuild_bvh")
        else:
            _host_check(N.lib().cgpth_scene_rebuild_bvh(self._h, obj_index, build_option), "rebuild_bvh")

    def refit_mesh(self, obj_index: int, triangles):
        """BVH refit of a mesh (or the replacement of a triangle object): triangles in the object's original order, as many as it has
        (triangles_from_arrays).  The tree is kept; node bounds, total_area, centroids follow the new triangles (cgpth_scene_refit_mesh)."""
        rows = _triangle_rows(triangles)
        _host_check(N.lib().cgpth_scene_refit_mesh(self._h, obj_index, _triangle_ptr(rows), rows.shape[0]), "refit_mesh")

    def skin_mesh(self, obj_index: int, bind_triangles, joints, weights, matrices):
        """The host mirror of Renderer.set_skin + Renderer.skin_mesh (cgpth_scene_skin_mesh): refit_mesh of
        skin_triangles(bind_triangles, joints, weights, matrices).  The host scene keeps no skin: every call takes it whole.  A light, a
        sphere or a plane is refused, as on the device."""
        rows, j, w = _skin_arrays(bind_triangles, joints, weights)
        m = _joint_matrices(matrices)
        _host_check(N.lib().cgpth_scene_skin_mesh(self._h, obj_index, _triangle_ptr(rows), j.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                  w.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], m.ctypes.data_as(C.POINTER(C.c_float)),
                                                  m.shape[0]), "skin_mesh")

    def morph_mesh(self, obj_index: int, base_triangles, deltas, weights):
        """The host mirror of Renderer.set_morph_targets + Renderer.morph_mesh (cgpth_scene_morph_mesh): refit_mesh of
        morph_triangles(base_triangles, deltas, weights).  The host scene keeps no targets: every call takes them whole.  A light, a
        sphere or a plane is refused, as on the device."""
        rows, d, w = _morph_arrays(base_triangles, deltas, weights)
        _host_check(N.lib().cgpth_scene_morph_mesh(self._h, obj_index, _triangle_ptr(rows), _triangle_ptr(d), rows.shape[0], d.shape[0],
                                                   w.ctypes.data_as(C.POINTER(C.c_float))), "morph_mesh")

    def update_primitive(self, obj_index: int, center=None, radius=None, normal=None, point=None):
        """Primitive::RenderImGui's sliders (ref: Primitives.cpp:385-410): a sphere's center / radius or a plane's normal / point;
        what is not given keeps its current value."""
        desc = self.flatten()
        if not 0 <= obj_index < desc.n_objects:
            raise HostError(f"update_primitive: object {obj_index} out of range ({desc.n_objects} objects)")
        cur = desc.objects[obj_index]
        if cur.kind == N.OBJECT_SPHERE:
            center = tuple(cur.sphere_center) if center is None else center
            radius = cur.sphere_radius if radius is None else radius
        elif cur.kind == N.OBJECT_PLANE:
            normal = tuple(cur.plane_normal) if normal is None else normal
            point = tuple(cur.plane_point) if point is None else point
        if cur.kind in (N.OBJECT_SPHERE, N.OBJECT_PLANE):
            abi = primitive_abi(cur.kind, cur.mat_index, center, radius, normal, point)
        else:
            abi = N.Object(kind=cur.kind, mat_index=cur.mat_index)      # refused by the library, with its message
        _host_check(N.lib().cgpth_scene_update_primitive(self._h, obj_index, C.byref(abi)), "update_primitive")

    def bvh_info(self, obj_index: int) -> N.BvhInfo:
        info = N.BvhInfo()
        _host_check(N.lib().cgpth_scene_bvh_info(self._h, obj_index, C.byref(info)), "bvh_info")
        return info

    def bvh_export(self, obj_index: int):
        """(nodes[n,8] uint32 words in the reference's 32-byte layout, tri_indices[m] uint32)"""
        info = self.bvh_info(obj_index)
        nodes = np.zeros((info.nodes_used, 8), np.uint32)
        tri = np.zeros(info.num_triangles, np.uint32)
        _host_check(N.lib().cgpth_scene_bvh_export(self._h, obj_index, nodes.ctypes.data_as(C.POINTER(N.BvhNode)),
                                                   tri.ctypes.data_as(C.POINTER(C.c_uint32))), "bvh_export")
        return nodes, tri

    def tree_cost(self, obj_index: int, c_inner: float = 1.0, c_tri: float = 1.0) -> N.TreeCost:
        """The surface-area cost of mesh `obj_index`'s tree as the host holds it (tree_cost of its bvh_export)."""
        return tree_cost(self.bvh_export(obj_index)[0], c_inner, c_tri)

    def flatten(self) -> N.SceneDesc:
        desc = N.SceneDesc()
        _host_check(N.lib().cgpth_scene_flatten(self._h, C.byref(desc)), "flatten")
        return desc

    def camera(self) -> N.Camera:
        cam = N.Camera()
        _host_check(N.lib().cgpth_scene_get_camera(self._h, C.byref(cam)), "get_camera")
        return cam

    def settings(self) -> N.Settings:
        s = N.Settings()
        _host_check(N.lib().cgpth_scene_get_settings(self._h, C.byref(s)), "get_settings")
        return s

    def close(self):
        if self._h:
            N.lib().cgpth_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_ppm(path: str, pixels: np.ndarray):
    p = np.ascontiguousarray(pixels, dtype=np.uint32)
    _host_check(N.lib().cgpth_write_ppm(path.encode(), p.ctypes.data_as(C.POINTER(C.c_uint32)), p.shape[1], p.shape[0]), "write_ppm")


def write_pfm(path: str, accumulator: np.ndarray, num_accumulated: int):
    a = np.ascontiguousarray(accumulator, dtype=np.float32)
    _host_check(N.lib().cgpth_write_pfm(path.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), num_accumulated,
                                        a.shape[1], a.shape[0]), "write_pfm")


def write_accumulator(path: str, accumulator: np.ndarray, num_accumulated: int):
    a = np.ascontiguousarray(accumulator, dtype=np.float32)
    _host_check(N.lib().cgpth_write_accumulator(path.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), num_accumulated,
                                                a.shape[1], a.shape[0]), "write_accumulator")


def read_accumulator(path: str, width: int, height: int):
    a = np.zeros((height, width, 4), np.float32)
    n = C.c_uint32(0)
    _host_check(N.lib().cgpth_read_accumulator(path.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n), width, height),
                "read_accumulator")
    return a, n.value
