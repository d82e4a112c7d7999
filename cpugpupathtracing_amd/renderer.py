"""Renderer: the reference's Render() / ResetAccumulator() / data.accumulator / data.pixels / data.stats surface
(ref: Source/Main.cpp:200-243,691-755) on top of the HIP library's C ABI (include/cpugpupt_abi.h).

No CPU path: constructing a Renderer without a gfx950 device raises DeviceError.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _native as N
from .scene import Scene, Settings, _clip_desc, _joint_matrices, _skeleton_desc, _morph_arrays, _morph_weights, _skin_arrays, _triangle_ptr, _triangle_rows, primitive_abi


_IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def _all_identity(matrices) -> bool:
    """Every matrix is the identity bit for bit (-0 is not 0): what cgpt_scene_update_transforms calls untransformed."""
    v = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
    return bool(np.array_equal(v.view(np.uint32), np.broadcast_to(_IDENTITY.view(np.uint32), v.shape)))


# cgpt_shade_sample / cgpt_shade_result as numpy records (Renderer.shade_samples)
SHADE_SAMPLE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("t", np.float32), ("obj", np.uint32), ("tri", np.uint32),
                         ("bvh_depth", np.uint32), ("throughput", np.float32, 3), ("rng", np.uint32), ("depth", np.uint32),
                         ("is_specular", np.uint32)])
SHADE_RESULT = np.dtype([("flags", np.uint32), ("o", np.float32, 3), ("d", np.float32, 3), ("throughput", np.float32, 3),
                         ("energy", np.float32, 3), ("rng", np.uint32), ("depth", np.uint32), ("is_specular", np.uint32),
                         ("shadow_o", np.float32, 3), ("shadow_d", np.float32, 3), ("shadow_tmax", np.float32),
                         ("pending", np.float32, 3), ("unwalked", np.uint32), ("reserved", np.uint32)])
assert SHADE_SAMPLE.itemsize == C.sizeof(N.ShadeSample) and SHADE_RESULT.itemsize == C.sizeof(N.ShadeResult)


# cgpt_tree_cost / cgpt_rebuild_result as numpy records (Renderer.tree_costs, Renderer.rebuild_degraded)
TREE_COST_DTYPE = np.dtype([("cost", np.float64), ("root_half_area", np.float64), ("n_inner", np.uint32), ("n_leaves", np.uint32),
                            ("max_leaf_tris", np.uint32), ("reserved", np.uint32)])
REBUILD_RESULT_DTYPE = np.dtype([("cost_before", np.float64), ("cost_after", np.float64), ("rebuilt", np.uint32), ("reserved", np.uint32)])
assert TREE_COST_DTYPE.itemsize == C.sizeof(N.TreeCost) and REBUILD_RESULT_DTYPE.itemsize == C.sizeof(N.RebuildResult)


class DeviceError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[cgpt status {code}] {message}")
        self.code = code


_CLIP_LAYER = np.dtype([("clip", np.uint32), ("time", np.float32), ("weight", np.float32), ("wrap", np.uint32)])
_LAYERED_ANIMATION = np.dtype({"names": ["obj_index", "n_layers", "layers", "n_targets", "weights"],
                               "formats": [np.uint32, np.uint32, np.uint64, np.uint32, np.uint64], "offsets": [0, 4, 8, 16, 24], "itemsize": 32})


def _layer_tables(entries):
    """(cgpt_layered_animation table, its length, the arrays it points into) of animate_layers' entries.  Both tables are filled as
    numpy arrays -- every entry's layers in one array of cgpt_clip_layer rows, an entry pointing at its first -- since a ctypes object
    per layer and per entry costs more than the device call itself for a crowd."""
    assert C.sizeof(N.ClipLayer) == _CLIP_LAYER.itemsize and C.sizeof(N.LayeredAnimation) == _LAYERED_ANIMATION.itemsize
    assert (N.LayeredAnimation.layers.offset, N.LayeredAnimation.n_targets.offset, N.LayeredAnimation.weights.offset) == (8, 16, 24)
    entries = [(obj_index, None if layers is None else list(layers), None if weights is None else _morph_weights(weights)) for obj_index, layers, weights in entries]
    n = len(entries)
    flat = [row for _, layers, _ in entries if layers is not None for row in layers]
    rows = np.zeros(max(1, len(flat)), _CLIP_LAYER)
    if flat:
        rows[:len(flat)] = flat
    table = np.zeros(max(1, n), _LAYERED_ANIMATION)
    if n:
        counts = np.array([0 if layers is None else len(layers) for _, layers, _ in entries], np.uint32)
        first = np.concatenate([[0], np.cumsum(counts[:-1], dtype=np.uint64)]).astype(np.uint64)
        table["obj_index"][:n] = [obj_index for obj_index, _, _ in entries]
        table["n_layers"][:n] = counts
        table["layers"][:n] = [0 if layers is None else rows.ctypes.data + 16 * int(at) for (_, layers, _), at in zip(entries, first)]
        table["n_targets"][:n] = [0 if w is None else w.size for _, _, w in entries]
        table["weights"][:n] = [0 if w is None else w.ctypes.data for _, _, w in entries]
    return table.ctypes.data_as(C.POINTER(N.LayeredAnimation)), n, (table, rows, entries)


class Renderer:
    def __init__(self, device=0, flags: int = 0):
        """device: one HIP device id, or a sequence of up to 8 ids for ONE context that spreads every frame over those GPUs
        (interleaved row bands, one RCCL exchange of the float4 bands per read-back; cgpt_ctx_create).  flags: N.CTX_*."""
        self.L = N.lib()
        self._ctx = C.c_void_p()
        devices = [int(device)] if isinstance(device, (int, np.integer)) else [int(d) for d in device]
        ids = (C.c_int * len(devices))(*devices)
        rc = self.L.cgpt_ctx_create(ids, len(devices), flags, C.byref(self._ctx))
        if rc != 0:
            raise DeviceError(rc, self.L.cgpt_last_error(None).decode())
        self.devices = devices
        self.is_group = len(devices) > 1 or bool(flags & N.CTX_FORCE_COLLECTIVE)
        self.scene: Optional[Scene] = None
        self._node_counts = []
        self._copy_of = []
        self.width = self.height = 0
        self.rows: Tuple[int, int] = (0, 0)
        self.interleave: Optional[Tuple[int, int, int]] = None
        self.n_rows = 0               # rows of this context's band
        self.num_accumulated = 0      # ref: Main.cpp:205
        self._glossy = False          # the device holds a roughness > 0 (cgpt_scene_update_roughness)
        self._rough_glass = False     # the device holds a transmission roughness > 0 (cgpt_scene_update_transmission_roughness)
        self._nee_candidates = 1      # cgpt_set_nee_candidates
        self._top_level = False       # cgpt_set_top_level
        self._smooth = False          # the device holds a smooth-normal flag (cgpt_scene_update_smooth_normals)
        self._transformed = False     # the device holds a transform that is not the identity (cgpt_scene_update_transforms)
        self.instanced = False        # the last upload was cgpt_scene_upload_instanced
        self._skin_joints = {}        # object -> joint count of the skin set_skin installed (joint_matrices)
        self._cost_baseline = {}      # device copy (_copy_of) -> the tree cost rebuild_degraded compares with; dropped by upload()
        self._cost_constants = (1.0, 1.0)   # ... and the (c_inner, c_tri) it was measured under

    def _check(self, rc: int):
        if rc != 0:
            raise DeviceError(rc, self.L.cgpt_last_error(self._ctx).decode())

    def set_stream(self, hip_stream):
        """cgpt_set_stream: the calls that follow run on the caller's stream, behind whatever the caller queued on it, and return
        once their own work is done ("Streams").  hip_stream: a hipStream_t as an int, or an object with a
        cuda_stream attribute (torch.cuda.Stream, torch.cuda.current_stream()); None restores the context's own stream.  A handle
        of 0 is the device's default stream -- torch's current stream on ROCm unless another was made current -- which the library
        cannot run on (include/cpugpupt_abi.h) and which the C ABI would read as "the context's own stream", unordered against the
        caller's work: ValueError, and nothing changed."""
        handle = None
        if hip_stream is not None:
            handle = int(hip_stream.cuda_stream if hasattr(hip_stream, "cuda_stream") else hip_stream)
            if handle == 0:
                raise ValueError("set_stream: handle 0 is the default stream, which this library cannot run on; use a non-default stream "
                                 "(torch.cuda.Stream()), or None for the context's own stream")
        self._check(self.L.cgpt_set_stream(self._ctx, C.c_void_p(handle)))

    def set_nee_candidates(self, m: int):
        """cgpt_set_nee_candidates: the NEE light sample of the renders that follow is the survivor of m candidates (resampled importance
        sampling; 1..32, 1 = the reference's single sample, bit for bit).  State of the renderer, kept across upload(); call
        reset_accumulator() before the next frame."""
        self._check(self.L.cgpt_set_nee_candidates(self._ctx, int(m)))
        self._nee_candidates = int(m)

    @property
    def nee_candidates(self) -> int:
        return self._nee_candidates

    def set_top_level(self, on: bool):
        """cgpt_set_top_level: True walks a tree over the objects' world boxes instead of the object list.  The image,
        the guides and every counter but inner_steps are the list walk's, bit for bit; it pays from some tens of objects on, when
        neighbouring object indices are neighbours in space (Scene.sort_objects_spatially).  State of the renderer, kept across
        upload(); the accumulator may be kept."""
        self._check(self.L.cgpt_set_top_level(self._ctx, 1 if on else 0))
        self._top_level = bool(on)

    @property
    def top_level(self) -> bool:
        return self._top_level

    def upload(self, scene: Scene, instanced: Optional[bool] = None):
        """cgpt_scene_upload, then the scene's roughness (cgpt_scene_update_roughness), transmission roughness
        (cgpt_scene_update_transmission_roughness) and smooth-normal flags (cgpt_scene_update_smooth_normals) when any is nonzero, and
        its transforms (cgpt_scene_update_transforms) when any is not the identity.
        instanced: True uploads with cgpt_scene_upload_instanced -- one device copy for the mesh objects that share a mesh
        (Scene.add_instance), same image bit for bit, and a refit_mesh then moves every sharer -- False with
        cgpt_scene_upload, None (the default) instanced exactly when the scene has an instance."""
        desc = scene.flatten()
        if instanced is None:
            instanced = scene.has_instances(desc)
        self._check((self.L.cgpt_scene_upload_instanced if instanced else self.L.cgpt_scene_upload)(self._ctx, C.byref(desc)))
        self.instanced = bool(instanced)
        self._glossy = self._rough_glass = self._smooth = self._transformed = False   # the upload reset every roughness, flag and transform
        self.scene = scene
        self._cost_baseline = {}
        self._node_counts = [desc.objects[k].node_count for k in range(desc.n_objects)]   # the uploaded trees (export_bvh)
        # the objects that share a device copy (rebuild_mesh): the same four slice words under an instanced upload, else every object alone
        slices = [(o.kind, o.node_offset, o.node_count, o.tri_offset, o.tri_count) for o in (desc.objects[k] for k in range(desc.n_objects))]
        self._copy_of = [slices.index(x) if instanced and x[0] == N.OBJECT_MESH else k for k, x in enumerate(slices)]
        rough = scene.roughness(desc.n_materials)
        if rough.any():
            self.update_roughness(rough)
        rough_t = scene.transmission_roughness(desc.n_materials)
        if rough_t.any():
            self.update_transmission_roughness(rough_t)
        smooth = scene.smooth_normals(desc.n_objects)
        if smooth.any():
            self.update_smooth_normals(smooth)
        transforms = scene.transforms(desc.n_objects)
        if not _all_identity(transforms):
            self.update_transforms(transforms)

    def scene_footprint(self) -> N.SceneFootprint:
        """cgpt_get_scene_footprint: what the uploaded scene occupies on one device -- device_bytes, n_objects, n_mesh_objects,
        n_mesh_copies (the meshes actually laid out), n_leaf_records, n_pair_records, n_orig_triangles."""
        fp = N.SceneFootprint()
        self._check(self.L.cgpt_get_scene_footprint(self._ctx, C.byref(fp)))
        return fp

    def update_materials(self, scene: Scene):
        """cgpt_scene_update_materials, then each of the scene's two roughnesses when it or the device's is nonzero."""
        desc = scene.flatten()
        self._check(self.L.cgpt_scene_update_materials(self._ctx, desc.materials, desc.n_materials))
        rough = scene.roughness(desc.n_materials)
        if rough.any() or self._glossy:
            self.update_roughness(rough)
        rough_t = scene.transmission_roughness(desc.n_materials)
        if rough_t.any() or self._rough_glass:
            self.update_transmission_roughness(rough_t)

    def update_roughness(self, values):
        """cgpt_scene_update_roughness: the specular lobe's roughness of every uploaded material (0: mirror, > 0: GGX with
        alpha = roughness^2).  Only the device copy changes; call reset_accumulator() before the next frame."""
        v = np.ascontiguousarray(values, np.float32).ravel()
        self._check(self.L.cgpt_scene_update_roughness(self._ctx, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
        self._glossy = bool((v > 0.0).any())

    def update_transmission_roughness(self, values):
        """cgpt_scene_update_transmission_roughness: the dielectric lobe's transmission roughness of every uploaded material (0: polished
        glass, > 0: GGX refraction with alpha_t = value^2).  Only the device copy changes; call reset_accumulator() before the next frame."""
        v = np.ascontiguousarray(values, np.float32).ravel()
        self._check(self.L.cgpt_scene_update_transmission_roughness(self._ctx, v.ctypes.data_as(C.POINTER(C.c_float)), v.size))
        self._rough_glass = bool((v > 0.0).any())

    def update_smooth_normals(self, flags):
        """cgpt_scene_update_smooth_normals: one flag per uploaded object (0: the reference's flat v0.normal, 1: interpolated vertex
        normals on a mesh or triangle object).  Only the device copy changes; call reset_accumulator() before the next frame."""
        v = np.ascontiguousarray(flags, np.uint32).ravel()
        self._check(self.L.cgpt_scene_update_smooth_normals(self._ctx, v.ctypes.data_as(C.POINTER(C.c_uint32)), v.size))
        self._smooth = bool(v.any())

    def update_transforms(self, matrices):
        """cgpt_scene_update_transforms: one object-to-world matrix per uploaded object, (n, 3, 4) or (n, 12) float32, the rows of
        [A | b].  Meshes and triangle objects; spheres, planes and lights take the identity only.  Only the device copy
        changes; call reset_accumulator() before the next frame."""
        v = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12)
        self._check(self.L.cgpt_scene_update_transforms(self._ctx, v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0]))
        self._transformed = not _all_identity(v)

    def refit_mesh(self, obj_index: int, triangles) -> float:
        """BVH refit on the device (cgpt_scene_refit_mesh): new triangles for uploaded mesh `obj_index` (or triangle object), in its
        original order, as many as were uploaded (scene.triangles_from_arrays); the tree is kept, its bounds follow.  Returns the new
        total_area.  Only the device copy changes: the host Scene is not touched (Scene.refit_mesh does the same there).  Call
        reset_accumulator() before the next frame, as the reference does after an edit."""
        rows = _triangle_rows(triangles)
        area = C.c_float()
        self._check(self.L.cgpt_scene_refit_mesh(self._ctx, obj_index, _triangle_ptr(rows), rows.shape[0], C.byref(area)))
        return area.value

    def set_skin(self, obj_index: int, bind_triangles, joints, weights, n_joints: int):
        """cgpt_scene_set_skin: keeps a skin for uploaded mesh (or triangle object) `obj_index` on the device -- its bind pose ((n, 18)
        triangles in the object's original order, as refit_mesh takes them), four joint indices and four weights per triangle corner
        ((n, 3, 4) each) -- for skin_mesh to pose from.  The scene does not change until the first skin_mesh.  A second
        call replaces the skin; upload() drops every skin; a light, a sphere or a plane takes none.  n_joints: 1..1024."""
        rows, j, w = _skin_arrays(bind_triangles, joints, weights)
        self._check(self.L.cgpt_scene_set_skin(self._ctx, obj_index, _triangle_ptr(rows), j.ctypes.data_as(C.POINTER(C.c_uint16)),
                                               w.ctypes.data_as(C.POINTER(C.c_float)), rows.shape[0], int(n_joints)))
        self._skin_joints[int(obj_index)] = int(n_joints)

    def skin_mesh(self, obj_index: int, matrices):
        """cgpt_scene_skin_mesh: poses skinned object `obj_index` on the device from its joint matrices, (n_joints, 3, 4) or
        (n_joints, 12) float32, the rows of [A | b] of each joint's object-space skinning matrix (glTF: jointGlobal x inverseBind).
        Always from the bind pose; the tree is kept and its bounds follow, as after refit_mesh(obj_index, scene.skin_triangles(...)),
        except that total_area keeps its uploaded value.  Only the device copy changes: the host Scene is not touched (Scene.skin_mesh
        is the mirror).  Call reset_accumulator() before the next frame."""
        m = _joint_matrices(matrices)
        self._check(self.L.cgpt_scene_skin_mesh(self._ctx, obj_index, m.ctypes.data_as(C.POINTER(C.c_float)), m.shape[0]))

    def clear_skin(self, obj_index: int):
        """cgpt_scene_clear_skin: frees the skin of object `obj_index`; the geometry stays at the last pose.  No skin: nothing happens."""
        self._check(self.L.cgpt_scene_clear_skin(self._ctx, obj_index))

    def set_morph_targets(self, obj_index: int, base_triangles, deltas):
        """cgpt_scene_set_morph_targets: keeps morph targets for uploaded mesh (or triangle object) `obj_index` on the device -- its base
        triangles ((n, 18) in the object's original order, as refit_mesh takes them) and deltas (n_targets, n, 18), displacement records of
        the same layout -- for morph_mesh to pose from.  The scene does not change until the first pose; the weights start
        at zero.  While they are installed the morphed base is also the bind pose of the object's skin (skin_mesh).  A second call replaces
        them; upload() drops them; a light, a sphere or a plane takes none.  n_targets: 1..256."""
        rows, d = _morph_arrays(base_triangles, deltas)
        self._check(self.L.cgpt_scene_set_morph_targets(self._ctx, obj_index, _triangle_ptr(rows), _triangle_ptr(d), rows.shape[0], d.shape[0]))

    def morph_mesh(self, obj_index: int, weights):
        """cgpt_scene_morph_mesh: poses object `obj_index` on the device from one weight per installed target (used as given; a zero of
        either sign skips its target).  Always from the base; the tree is kept and its bounds follow, as after
        refit_mesh(obj_index, morph_triangles(...)) -- or, with a posed skin, refit_mesh(obj_index, skin_triangles(morph_triangles(...), ...))
        -- except that total_area keeps its uploaded value.  Only the device copy changes.  Call reset_accumulator() before the next frame."""
        w = _morph_weights(weights)
        self._check(self.L.cgpt_scene_morph_mesh(self._ctx, obj_index, w.ctypes.data_as(C.POINTER(C.c_float)), w.size))

    def clear_morph_targets(self, obj_index: int):
        """cgpt_scene_clear_morph_targets: frees the targets of object `obj_index`; the geometry stays where it is and a skin goes back to
        its own bind pose at its next skin_mesh.  No targets: nothing happens."""
        self._check(self.L.cgpt_scene_clear_morph_targets(self._ctx, obj_index))

    def pose_objects(self, entries):
        """cgpt_scene_pose_objects: poses many objects in one call.  `entries` is an iterable of (obj_index, matrices or
        None, weights or None) with the array shapes skin_mesh and morph_mesh accept; the device scene afterwards is what
        morph_mesh(obj_index, weights) and then skin_mesh(obj_index, matrices) of every entry in turn would leave, bit for bit, for a
        number of kernel launches that does not grow with the number of entries.  An object (or an instanced mesh group) may be named
        once; a refused batch changes nothing.  Only the device copy changes.  Call reset_accumulator() before the next frame."""
        keep, rows = [], []
        for obj_index, matrices, weights in entries:
            m = _joint_matrices(matrices) if matrices is not None else None
            w = _morph_weights(weights) if weights is not None else None
            keep.append((m, w))
            rows.append(N.Pose(int(obj_index), 0 if m is None else m.shape[0], None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
                               0 if w is None else w.size, None if w is None else w.ctypes.data_as(C.POINTER(C.c_float))))
        poses = (N.Pose * max(1, len(rows)))(*rows)
        self._check(self.L.cgpt_scene_pose_objects(self._ctx, poses, len(rows)))

    def set_skeleton(self, obj_index: int, parents, inverse_bind, rest, root=None):
        """cgpt_scene_set_skeleton: keeps a skeleton for the skin of object `obj_index` on the device -- parents (n_joints int32, -1 a
        root, any order), inverse_bind (n_joints, 12) or (n_joints, 3, 4), rest (n_joints, 10) {T.xyz, R.xyzw, S.xyz} and an optional
        root matrix (12 floats) -- for animate_objects to pose from.  The object needs a skin with the same joint
        count; the skeleton is replaced, cleared and dropped with that skin."""
        desc, keep = _skeleton_desc(parents, inverse_bind, rest, root)
        self._check(self.L.cgpt_scene_set_skeleton(self._ctx, obj_index, C.byref(desc)))

    def create_clip(self, n_joints: int, channels, times, values) -> int:
        """cgpt_clip_create: copies an animation clip to the device(s) and returns its handle.  channels: rows of six words {joint,
        path N.ANIM_PATH_*, interpolation N.ANIM_STEP | N.ANIM_LINEAR, n_keys, first_time, first_value}; key i of a channel is
        times[first_time + i] with 3 (translation, scale) or 4 (rotation xyzw) floats at values[first_value + width * i].  A clip
        belongs to the renderer, is shared by any number of objects and survives upload()."""
        desc, keep = _clip_desc(n_joints, channels, times, values)
        handle = C.c_uint32()
        self._check(self.L.cgpt_clip_create(self._ctx, C.byref(desc), C.byref(handle)))
        return handle.value

    def destroy_clip(self, clip: int):
        """cgpt_clip_destroy: frees a clip."""
        self._check(self.L.cgpt_clip_destroy(self._ctx, int(clip)))

    def animate_objects(self, entries):
        """cgpt_scene_animate_objects: pose_objects with every entry's joint matrices computed on the device.
        `entries` is an iterable of (obj_index, clip, time, weights or None); the device scene afterwards is what
        pose_objects([(obj_index, animate_joints(skeleton, clip, time), weights), ...]) leaves, bit for bit, without the matrices
        being evaluated or uploaded by the host.  A refused call changes nothing.  Call reset_accumulator() before the next frame."""
        keep, rows = [], []
        for obj_index, clip, time, weights in entries:
            w = _morph_weights(weights) if weights is not None else None
            keep.append(w)
            rows.append(N.Animation(int(obj_index), int(clip), float(time), 0 if w is None else w.size,
                                    None if w is None else w.ctypes.data_as(C.POINTER(C.c_float))))
        table = (N.Animation * max(1, len(rows)))(*rows)
        self._check(self.L.cgpt_scene_animate_objects(self._ctx, table, len(rows)))

    def animate_layers(self, entries):
        """cgpt_scene_animate_layers: animate_objects with every entry's joints blended from 1 .. 4 clips.  `entries`
        is an iterable of (obj_index, [(clip, time, weight, wrap), ...], weights or None) with wrap one of N.ANIM_WRAP_CLAMP, _LOOP,
        _PINGPONG; the device scene afterwards is what pose_objects leaves for the matrices of the host's animate_layers, bit for bit.
        A refused call changes nothing.  Call reset_accumulator() before the next frame."""
        table, n, keep = _layer_tables(entries)
        self._check(self.L.cgpt_scene_animate_layers(self._ctx, table, n))

    def clip_range(self, clip: int):
        """cgpt_clip_get_range: (begin, end) of a clip, the smallest first-key and the largest last-key time of its channels."""
        b, e = C.c_float(), C.c_float()
        self._check(self.L.cgpt_clip_get_range(self._ctx, int(clip), C.byref(b), C.byref(e)))
        return np.float32(b.value), np.float32(e.value)

    def joint_matrices(self, obj_index: int, n_joints: Optional[int] = None) -> np.ndarray:
        """cgpt_scene_get_joint_matrices: the (n_joints, 12) float32 matrices of the last pose of object `obj_index`'s skin, however
        given (skin_mesh, pose_objects, animate_objects).  n_joints: the skin's count; None takes what set_skin was given."""
        if n_joints is None:
            n_joints = self._skin_joints.get(int(obj_index), 1)
        out = np.empty((int(n_joints), 12), np.float32)
        self._check(self.L.cgpt_scene_get_joint_matrices(self._ctx, obj_index, out.ctypes.data_as(C.POINTER(C.c_float)), int(n_joints)))
        return out

    def rebuild_mesh(self, obj_index: int, build_option: int = N.BUILD_SAH_BINNED):
        """cgpt_scene_rebuild_mesh: splits the tree of uploaded mesh `obj_index` again, in place on the device, over the triangles its
        copy holds now (after refits, skins, morphs) and from its current leaf order -- what Scene.rebuild_bvh(obj_index, build_option)
        does on the host, without the triangles leaving the device.  Skins, morph targets, transforms, materials and
        total_area are kept.  Returns (n_nodes, max_depth) of the new tree; export_bvh follows.  Only the device copy changes.  Call
        reset_accumulator() before the next frame."""
        n_nodes, depth = C.c_uint32(), C.c_uint32()
        self._check(self.L.cgpt_scene_rebuild_mesh(self._ctx, obj_index, int(build_option), C.byref(n_nodes), C.byref(depth)))
        for k in range(len(self._node_counts)):                          # every placement of the copy shows the new tree
            if self._copy_of[k] == self._copy_of[obj_index]:
                self._node_counts[k] = n_nodes.value
        if self._copy_of[obj_index] in self._cost_baseline:               # rebuild_degraded's baseline follows the new tree
            c_inner, c_tri = self._cost_constants
            self._cost_baseline[self._copy_of[obj_index]] = float(self.tree_costs([obj_index], c_inner, c_tri)["cost"][0])
        return n_nodes.value, depth.value

    def tree_costs(self, objs, c_inner: float = 1.0, c_tri: float = 1.0) -> np.ndarray:
        """cgpt_scene_tree_costs: the surface-area cost of the trees of the uploaded meshes `objs` as they are now on the device, one
        call and one small readback for all of them.  A structured array with the fields cost, root_half_area,
        n_inner, n_leaves, max_leaf_tris per entry -- what Scene.tree_cost / tree_cost(export_bvh(obj)) compute on the host, to
        rounding.  The call only reads: the accumulator, the guides and the temporal history are kept."""
        o = np.ascontiguousarray(objs, np.uint32).ravel()
        out = np.zeros(o.size, TREE_COST_DTYPE)
        self._check(self.L.cgpt_scene_tree_costs(self._ctx, o.ctypes.data_as(C.POINTER(C.c_uint32)), o.size, float(c_inner), float(c_tri),
                                                 out.ctypes.data_as(C.POINTER(N.TreeCost))))
        return out

    def rebuild_degraded(self, objs, ratio: float, build_option: int = N.BUILD_SAH_BINNED, c_inner: float = 1.0, c_tri: float = 1.0) -> np.ndarray:
        """cgpt_scene_rebuild_degraded with the baseline kept here: rebuilds, as rebuild_mesh does, every mesh of `objs` whose tree's
        cost has grown past `ratio` times its baseline (DESIGN.md 5.36 has the table to choose a ratio from; there is no default).  The
        baseline of a device copy is its cost at the first call that names it (so call it once at the bind pose), is replaced by the new
        tree's cost after every rebuild -- this call's or rebuild_mesh's -- and is dropped by upload() and by a change of the
        constants.  Returns a structured array with cost_before, cost_after and rebuilt per entry.  When nothing is rebuilt the scene
        and the temporal history are untouched; otherwise call reset_accumulator() before the next frame."""
        o = np.ascontiguousarray(objs, np.uint32).ravel()
        if self._cost_constants != (float(c_inner), float(c_tri)):
            self._cost_baseline = {}
            self._cost_constants = (float(c_inner), float(c_tri))
        copy_of = lambda k: self._copy_of[k] if k < len(self._copy_of) else ("out of range", k)   # the call refuses it
        fresh = [int(k) for k in o if copy_of(int(k)) not in self._cost_baseline]
        if fresh:
            for k, c in zip(fresh, self.tree_costs(fresh, c_inner, c_tri)["cost"]):
                self._cost_baseline.setdefault(copy_of(k), float(c))
        rows = (N.RebuildCandidate * max(1, o.size))(*[N.RebuildCandidate(int(k), 0, self._cost_baseline[copy_of(int(k))]) for k in o])
        out = np.zeros(o.size, REBUILD_RESULT_DTYPE)
        rc = self.L.cgpt_scene_rebuild_degraded(self._ctx, rows, o.size, float(ratio), int(build_option), float(c_inner), float(c_tri),
                                                out.ctypes.data_as(C.POINTER(N.RebuildResult)))
        if rc != 0:                                                       # a refusal mid-call leaves the meshes rebuilt before it rebuilt:
            message = self.L.cgpt_last_error(self._ctx).decode()          # follow their node counts and measure their baselines afresh next time
            for k in sorted(set(int(k) for k in o if int(k) < len(self._copy_of))):
                self._cost_baseline.pop(self._copy_of[k], None)
                try:
                    self._follow_tree(k, self.tree_costs([k], c_inner, c_tri)[0])
                except DeviceError:
                    pass
            raise DeviceError(rc, message)
        rebuilt = [int(k) for k, r in zip(o, out["rebuilt"]) if r]
        if rebuilt:
            for k, c in zip(rebuilt, self.tree_costs(rebuilt, c_inner, c_tri)):
                self._follow_tree(k, c)
                self._cost_baseline[self._copy_of[k]] = float(c["cost"])
        return out

    def _follow_tree(self, obj_index: int, cost):
        """the node count (export_bvh) of every placement of `obj_index`'s copy, from its tree's cost record"""
        for j in range(len(self._node_counts)):
            if self._copy_of[j] == self._copy_of[obj_index]:
                self._node_counts[j] = int(cost["n_inner"]) + int(cost["n_leaves"])

    def export_bvh(self, obj_index: int) -> np.ndarray:
        """The device's tree of mesh `obj_index` as it is now (after refits): nodes[n,8] uint32 words in the reference's 32-byte layout
        and numbering, as Scene.bvh_export returns them.  Reads the device only; the host Scene is not touched."""
        nodes = np.zeros((self._node_counts[obj_index] if obj_index < len(self._node_counts) else 0, 8), np.uint32)
        self._check(self.L.cgpt_scene_export_bvh(self._ctx, obj_index, nodes.ctypes.data_as(C.POINTER(N.BvhNode)), nodes.shape[0]))
        return nodes

    def update_primitive(self, obj_index: int, mat_index: int, center=None, radius=None, normal=None, point=None):
        """cgpt_scene_update_primitive: a sphere's center and radius, or a plane's normal and point (mat_index: the object's
        uploaded material, which does not change).  Only the device copy changes: the host Scene is not touched."""
        kind = N.OBJECT_SPHERE if center is not None or radius is not None else N.OBJECT_PLANE
        abi = primitive_abi(kind, mat_index, center, radius, normal, point)
        self._check(self.L.cgpt_scene_update_primitive(self._ctx, obj_index, C.byref(abi)))

    def render(self, width: int, height: int, n_samples: int = 1, seed: int = 0x12345678, rows: Optional[Tuple[int, int]] = None,
               kernel: int = N.KERNEL_AUTO, counters: bool = False, settings: Optional[Settings] = None,
               interleave: Optional[Tuple[int, int, int]] = None, camera: Optional[N.Camera] = None):
        """Render() x n_samples (ref: Main.cpp:691-755).  Accumulates; call reset_accumulator() to start over.
        rows = (begin, end): a contiguous band.  interleave = (band_rows, count, index): every count-th band of band_rows
        rows starting at band `index` (load-balanced multi-GPU tiling); the band is stored compactly in that order.
        camera: a cgpt_camera (default: the uploaded scene's)."""
        assert self.scene is not None, "upload a scene first"
        assert rows is None or interleave is None
        r0, r1 = rows if rows is not None else (0, height)
        il = interleave if interleave is not None else (0, 0, 0)
        if (width, height, (r0, r1), interleave) != (self.width, self.height, self.rows, self.interleave):
            self.num_accumulated = 0          # the library re-allocates (zeroed) on a size/band change
        cam = camera if camera is not None else self.scene.camera()
        st = settings.to_abi() if settings is not None else self.scene.settings()
        p = N.RenderParams(width, height, r0, r1, self.num_accumulated, n_samples, seed & 0xFFFFFFFF, kernel,
                           N.RENDER_COUNTERS if counters else 0, il[0], il[1], il[2])
        self._check(self.L.cgpt_render(self._ctx, C.byref(cam), C.byref(st), C.byref(p)))
        self.width, self.height, self.rows, self.interleave = width, height, (r0, r1), interleave
        if interleave is None:
            self.n_rows = r1 - r0
        else:
            from .distributed import interleaved_rows
            self.n_rows = len(interleaved_rows(height, interleave[2], interleave[1], interleave[0]))
        self.num_accumulated += n_samples

    def reset_accumulator(self):
        self._check(self.L.cgpt_reset_accumulator(self._ctx))
        self.num_accumulated = 0

    def accumulator(self) -> np.ndarray:
        """float4 running sums of this context's row band: (rows, width, 4)"""
        out = np.empty((self.n_rows, self.width, 4), np.float32)
        self._check(self.L.cgpt_read_accumulator(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def load_accumulator(self, acc: np.ndarray, num_accumulated: int, width: int, height: int,
                         rows: Optional[Tuple[int, int]] = None, interleave: Optional[Tuple[int, int, int]] = None):
        """Restores a saved accumulator band and its sample count (checkpoint / resume: data.accumulator + data.num_accumulated,
        ref: Main.cpp:204-205); the next render() continues at sample `num_accumulated`, bit-identical to an uninterrupted run."""
        a = np.ascontiguousarray(acc, np.float32)
        r0, r1 = rows if rows is not None else (0, height)
        il = interleave if interleave is not None else (0, 0, 0)
        p = N.RenderParams(width, height, r0, r1, 0, 0, 0, 0, 0, il[0], il[1], il[2])
        self._check(self.L.cgpt_write_accumulator(self._ctx, C.byref(p), a.ctypes.data_as(C.POINTER(C.c_float)), a.size, num_accumulated))
        self.width, self.height, self.rows, self.interleave = width, height, (r0, r1), interleave
        if interleave is None:
            self.n_rows = r1 - r0
        else:
            from .distributed import interleaved_rows
            self.n_rows = len(interleaved_rows(height, interleave[2], interleave[1], interleave[0]))
        self.num_accumulated = num_accumulated

    def set_tuning(self, **knobs: int):
        """cgpt_set_tuning: wavefront knobs for this context (pools=1, batch=16, ...); never changes results."""
        for name, value in knobs.items():
            self._check(self.L.cgpt_set_tuning(self._ctx, name.encode(), int(value)))

    def measure_issue_rate(self, kind: int = 0, waves_per_simd: int = 6, iters: int = 20000) -> Tuple[float, float]:
        """Measured vector-instruction issue rate of the device (wave64 instructions / s over the chip) and the launch's ms."""
        rate = C.c_double(); ms = C.c_double()
        self._check(self.L.cgpt_measure_issue_rate(self._ctx, kind, waves_per_simd, iters, C.byref(rate), C.byref(ms)))
        return rate.value, ms.value

    def pixels(self) -> np.ndarray:
        out = np.empty((self.n_rows, self.width), np.uint32)
        self._check(self.L.cgpt_read_pixels(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def guides(self, camera: Optional[N.Camera] = None) -> np.ndarray:
        """The denoiser's first-hit guides of this context's band (cgpt_read_guides): (rows, width, 12) float32 per pixel
        {x.xyz, t, n.xyz, bits(obj), albedo.xyz, bits(mat_index)}; a miss is zeros, t = 1e34 and obj = mat = 0xFFFFFFFF.
        camera: the one the accumulator was rendered with (default: the uploaded scene's)."""
        cam = camera if camera is not None else self.scene.camera()
        out = np.empty((self.n_rows, self.width, 12), np.float32)
        self._check(self.L.cgpt_read_guides(self._ctx, C.byref(cam), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def denoise(self, iterations: int = 5, sigma_color: float = 4.0, sigma_normal: float = 0.2, sigma_position: float = 0.3,
                demodulate: bool = True, camera: Optional[N.Camera] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The accumulated image through the edge-avoiding a-trous filter (cgpt_denoise): (rows, width, 4) float32 radiance {rgb, 1}
        and (rows, width) uint32 pixels packed as data.pixels is.  The accumulator, pixels and statistics are left as they are."""
        cam = camera if camera is not None else self.scene.camera()
        p = N.DenoiseParams(iterations, N.DENOISE_DEMODULATE_ALBEDO if demodulate else 0, sigma_color, sigma_normal, sigma_position)
        rgba = np.empty((self.n_rows, self.width, 4), np.float32)
        px = np.empty((self.n_rows, self.width), np.uint32)
        self._check(self.L.cgpt_denoise(self._ctx, C.byref(cam), C.byref(p), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                        px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
        return rgba, px

    def denoise_temporal(self, iterations: int = 5, sigma_color: float = 4.0, sigma_normal: float = 0.2, sigma_position: float = 0.3,
                         demodulate: bool = True, max_history: float = 64.0, normal_cos_min: float = 0.9, plane_tolerance: float = 0.01,
                         keep_view_dependent: bool = False, camera: Optional[N.Camera] = None,
                         follow_transforms: bool = False, follow_poses: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """denoise() with the temporal stage in front (cgpt_denoise_temporal): the history of the earlier calls is reprojected onto
        `camera` (the one of this frame's render; default: the uploaded scene's) and merged with the accumulated frame by sample counts
        before the filter runs.  Per frame: reset_accumulator(), render(), denoise_temporal(); each call consumes the accumulated
        samples once.  Every scene edit drops the history; follow_transforms=True (CGPT_TEMPORAL_FOLLOW_TRANSFORMS) keeps it across
        update_transforms() calls and carries the hits on the moved objects back to where they were; follow_poses=True
        (CGPT_TEMPORAL_FOLLOW_POSES) keeps it across skin_mesh() calls and carries the hits on the re-posed objects back to where the
        same surface points were under the history's pose (previous_hits() reads those records).  denoise_temporal_following() also
        follows morph_mesh() calls."""
        return self._denoise_temporal(iterations, sigma_color, sigma_normal, sigma_position, demodulate, max_history, normal_cos_min, plane_tolerance,
                                      keep_view_dependent, camera, (N.TEMPORAL_FOLLOW_TRANSFORMS if follow_transforms else 0) |
                                      (N.TEMPORAL_FOLLOW_POSES if follow_poses else 0))

    def denoise_temporal_following(self, iterations: int = 5, sigma_color: float = 4.0, sigma_normal: float = 0.2, sigma_position: float = 0.3,
                                   demodulate: bool = True, max_history: float = 64.0, normal_cos_min: float = 0.9, plane_tolerance: float = 0.01,
                                   keep_view_dependent: bool = False, camera: Optional[N.Camera] = None,
                                   transforms: bool = False, poses: bool = False, morphs: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """denoise_temporal() with one keyword per kind of edit the history is kept across: transforms (update_transforms();
        CGPT_TEMPORAL_FOLLOW_TRANSFORMS), poses (skin_mesh(); CGPT_TEMPORAL_FOLLOW_POSES) and morphs (morph_mesh();
        CGPT_TEMPORAL_FOLLOW_MORPHS).  Each keeps its own kind only: a character with a skeleton and blend shapes needs
        poses=True and morphs=True.  The hits on an object that was re-posed through its morph targets are carried back to where the same
        surface points were under the history's weights (and joint matrices); previous_hits() reads those records too."""
        return self._denoise_temporal(iterations, sigma_color, sigma_normal, sigma_position, demodulate, max_history, normal_cos_min, plane_tolerance,
                                      keep_view_dependent, camera, (N.TEMPORAL_FOLLOW_TRANSFORMS if transforms else 0) |
                                      (N.TEMPORAL_FOLLOW_POSES if poses else 0) | (N.TEMPORAL_FOLLOW_MORPHS if morphs else 0))

    def _denoise_temporal(self, iterations, sigma_color, sigma_normal, sigma_position, demodulate, max_history, normal_cos_min, plane_tolerance,
                          keep_view_dependent, camera, follow_flags) -> Tuple[np.ndarray, np.ndarray]:
        cam = camera if camera is not None else self.scene.camera()
        p = N.DenoiseParams(iterations, N.DENOISE_DEMODULATE_ALBEDO if demodulate else 0, sigma_color, sigma_normal, sigma_position)
        t = N.TemporalParams(max_history, normal_cos_min, plane_tolerance, (N.TEMPORAL_KEEP_VIEW_DEPENDENT if keep_view_dependent else 0) | follow_flags)
        rgba = np.empty((self.n_rows, self.width, 4), np.float32)
        px = np.empty((self.n_rows, self.width), np.uint32)
        self._check(self.L.cgpt_denoise_temporal(self._ctx, C.byref(cam), C.byref(p), C.byref(t), rgba.ctypes.data_as(C.POINTER(C.c_float)),
                                                 rgba.size, px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
        return rgba, px

    def temporal_reset(self):
        """Drops the temporal history (cgpt_temporal_reset)."""
        self._check(self.L.cgpt_temporal_reset(self._ctx))

    def temporal_history(self) -> np.ndarray:
        """The history the last denoise_temporal() stored (cgpt_read_temporal_history): (rows, width, 4) float32 {merged colour in the
        filter's input domain, history length in samples}."""
        out = np.empty((self.n_rows, self.width, 4), np.float32)
        self._check(self.L.cgpt_read_temporal_history(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def previous_hits(self) -> np.ndarray:
        """The carry-back records of the last denoise_temporal(follow_poses=True) or denoise_temporal_following(poses / morphs=True) in
        which an object was re-posed (cgpt_read_previous_hits): (rows, width, 8) float32 {x_p.xyz, bits(state), n_p.xyz, 0} -- where each pixel's first hit was under
        the history's pose; state 0 (not re-posed: the pixel's own x, n), 1 (re-posed) or 2 (no history)."""
        out = np.empty((self.n_rows, self.width, 8), np.float32)
        self._check(self.L.cgpt_read_previous_hits(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def denoise_variance_guided(self, iterations: int = 5, sigma_luminance: float = 4.0, sigma_normal: float = 0.2, sigma_position: float = 0.3,
                                demodulate: bool = True, temporal: bool = False, min_history_frames: int = 4, camera: Optional[N.Camera] = None,
                                max_history: float = 64.0, normal_cos_min: float = 0.9, plane_tolerance: float = 0.01,
                                keep_view_dependent: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """denoise() with the colour edge-stop in standard deviations of each pixel's luminance (cgpt_denoise_variance_guided): the
        variance is estimated over a 7x7 window, or -- temporal=True: denoise_temporal()'s stage runs in front, with its keywords, and
        luminance moments are kept with its history -- over time once a pixel has min_history_frames frames' worth of samples.
        Returns what denoise() returns; variance() reads the map the first pass used."""
        cam = camera if camera is not None else self.scene.camera()
        p = N.DenoiseParams(iterations, N.DENOISE_DEMODULATE_ALBEDO if demodulate else 0, 4.0, sigma_normal, sigma_position)
        t = N.TemporalParams(max_history, normal_cos_min, plane_tolerance, N.TEMPORAL_KEEP_VIEW_DEPENDENT if keep_view_dependent else 0)
        v = N.VarianceParams(sigma_luminance, min_history_frames, N.VARIANCE_TEMPORAL if temporal else 0)
        rgba = np.empty((self.n_rows, self.width, 4), np.float32)
        px = np.empty((self.n_rows, self.width), np.uint32)
        self._check(self.L.cgpt_denoise_variance_guided(self._ctx, C.byref(cam), C.byref(p), C.byref(t), C.byref(v),
                                                        rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                                        px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
        return rgba, px

    def variance(self) -> np.ndarray:
        """The per-pixel luminance variance the first pass of the last denoise_variance_guided() read (cgpt_read_variance):
        (rows, width) float32."""
        out = np.empty((self.n_rows, self.width), np.float32)
        self._check(self.L.cgpt_read_variance(self._ctx, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def tonemap(self, source="accumulator", curve="aces", transfer="srgb", auto: bool = True, image: Optional[np.ndarray] = None,
                **params) -> Tuple[np.ndarray, np.ndarray]:
        """cgpt_tonemap, the display stage: linear radiance through an exposure, a tone curve ("clamp", "reinhard",
        "aces", "hable") and a transfer function ("linear", "srgb") on the device.  source: "accumulator" (the rendered band, divided
        as pixels() divides it), "denoised" (the result of the last denoise*() call, still on the device) or "host" with
        image = (rows, width, 4) float32.  auto=True meters the frame's luminance histogram and moves the renderer's adapted exposure
        towards it by alpha (adaptation_alpha(dt, speed); exposure() reads the result, exposure_reset() forgets the adaptation);
        auto=False applies exposure_scale 2^ev_bias.  params: exposure_scale, ev_bias, white, key, low_fraction, high_fraction, alpha
        (tonemap.tonemap_params).  Returns (rows, width, 4) float32 {r, g, b, 1} and (rows, width) uint32 pixels packed as pixels()
        packs them.  The accumulator, pixels(), the denoiser's state and the statistics are left as they are."""
        from .tonemap import tonemap_params
        p, keep = tonemap_params(source=source, curve=curve, transfer=transfer, auto=auto, image=image, **params)
        rows, width = (keep.shape[0], keep.shape[1]) if keep is not None and p.source == N.TONEMAP_HOST else (self.n_rows, self.width)
        rgba = np.empty((rows, width, 4), np.float32)
        px = np.empty((rows, width), np.uint32)
        self._check(self.L.cgpt_tonemap(self._ctx, C.byref(p), rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                                        px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
        return rgba, px

    def exposure(self) -> N.ExposureInfo:
        """cgpt_read_exposure: the reading of the last successful tonemap(auto=True) -- .mean_index and .adapted_index (histogram
        indices: eighths of an octave above 2^-16), .exposure, .valid (N.EXPOSURE_ADAPTED | N.EXPOSURE_METERED), .n_counted,
        .n_ignored, .histogram[256]."""
        info = N.ExposureInfo()
        self._check(self.L.cgpt_read_exposure(self._ctx, C.byref(info)))
        return info

    def exposure_reset(self):
        """cgpt_exposure_reset: the next auto-exposure call sets the adapted exposure instead of approaching it."""
        self._check(self.L.cgpt_exposure_reset(self._ctx))

    def accumulator_device_ptr(self) -> Tuple[int, int]:
        ptr = C.c_void_p(); nbytes = C.c_size_t()
        self._check(self.L.cgpt_accumulator_device_ptr(self._ctx, C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def pixels_device_ptr(self) -> Tuple[int, int]:
        """cgpt_pixels_device_ptr: the packed uint32 pixels of this context's band on the device, (pointer, bytes = rows * width * 4);
        on a multi-device context the gathered frame on the first device, as accumulator_device_ptr()."""
        ptr = C.c_void_p(); nbytes = C.c_size_t()
        self._check(self.L.cgpt_pixels_device_ptr(self._ctx, C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def stats(self) -> N.Stats:
        s = N.Stats()
        self._check(self.L.cgpt_get_stats(self._ctx, C.byref(s)))
        unwalked = C.c_uint64()                                      # cgpt_stats keeps its size: this counter has an accessor of its own
        self._check(self.L.cgpt_get_retrace_unwalked(self._ctx, C.byref(unwalked)))
        s.retrace_unwalked = unwalked.value
        return s

    def reset_stats(self):
        self._check(self.L.cgpt_reset_stats(self._ctx))

    def intersect_rays(self, origins, dirs, tmax=None):
        """IntersectScene on a ray batch (ref: Main.cpp:299-316): returns t, obj_idx, tri_idx, bvh_depth"""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = o.shape[0]
        tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32)
        t = np.empty(n, np.float32); obj = np.empty(n, np.uint32); tri = np.empty(n, np.uint32); dep = np.empty(n, np.uint32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(self.L.cgpt_intersect_rays(self._ctx, o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                               tm.ctypes.data_as(fp) if tm is not None else None, n, t.ctypes.data_as(fp),
                                               obj.ctypes.data_as(up), tri.ctypes.data_as(up), dep.ctypes.data_as(up)))
        return t, obj, tri, dep

    def shade_samples(self, samples, settings: Optional[Settings] = None) -> np.ndarray:
        """cgpt_shade_samples: one bounce of TracePathAdvanced on each record of `samples` (SHADE_SAMPLE: a traced ray with its hit
        record, obj 0xFFFFFFFF for a miss, and the path state before the bounce), in the instantiation a render of this context runs.
        Returns SHADE_RESULT records.  settings: default the uploaded scene's.  Nothing is traced; the accumulator and stats stay."""
        a = np.ascontiguousarray(samples, SHADE_SAMPLE).ravel()
        out = np.zeros(a.size, SHADE_RESULT)
        st = settings.to_abi() if settings is not None else self.scene.settings()
        self._check(self.L.cgpt_shade_samples(self._ctx, C.byref(st), a.ctypes.data_as(C.POINTER(N.ShadeSample)), a.size,
                                              out.ctypes.data_as(C.POINTER(N.ShadeResult))))
        return out

    def trace_rays(self, origins=None, dirs=None, tmax=None, shadow_origins=None, shadow_dirs=None, shadow_tmax=None,
                   counters: bool = False, reverse: bool = False):
        """cgpt_trace_rays: the wavefront pipeline's later-round trace launch on host rays, extend rays (closest hit) and shadow rays
        (occlusion) in one launch, in the instantiation and with the knobs a render of this context runs.  Returns t, obj_idx, tri_idx,
        bvh_depth per extend ray (a miss's bvh_depth is 0 while the retire_misses knob is 1) and one uint8 per shadow ray, 1 = occluded.
        counters: the counting instantiation; reverse: slots and lists laid out back to front (CGPT_TRACE_REVERSED; same results)."""
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

        def rays(o, d, tm):
            if o is None:
                return None, None, None, 0
            o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
            d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
            assert o.shape == d.shape
            tm = None if tm is None else np.ascontiguousarray(tm, np.float32).reshape(o.shape[0])
            return o, d, tm, o.shape[0]

        def ptr(a):
            return a.ctypes.data_as(fp) if a is not None and a.size else None
        eo, ed, et, n = rays(origins, dirs, tmax)
        so, sd, st, m = rays(shadow_origins, shadow_dirs, shadow_tmax)
        t = np.empty(n, np.float32); obj = np.empty(n, np.uint32); tri = np.empty(n, np.uint32); dep = np.empty(n, np.uint32)
        occ = np.empty(m, np.uint8)
        flags = (N.TRACE_COUNTERS if counters else 0) | (N.TRACE_REVERSED if reverse else 0)
        self._check(self.L.cgpt_trace_rays(self._ctx, ptr(eo), ptr(ed), ptr(et), n, ptr(so), ptr(sd), ptr(st), m, flags,
                                           t.ctypes.data_as(fp), obj.ctypes.data_as(up), tri.ctypes.data_as(up), dep.ctypes.data_as(up),
                                           occ.ctypes.data_as(C.POINTER(C.c_uint8))))
        return t, obj, tri, dep, occ

    def trace_first_hits(self, width: int, height: int, rows: Optional[Tuple[int, int]] = None, camera: Optional[N.Camera] = None,
                         counters: bool = False):
        """cgpt_trace_first_hits: the wavefront pipeline's round-0 trace launch on the primary rays of a band: obj_idx, tri_idx, bvh_depth
        and t, each (rows, width).  camera: default the uploaded scene's."""
        r0, r1 = rows if rows is not None else (0, height)
        cam = camera if camera is not None else self.scene.camera()
        shape = (max(r1 - r0, 0), width)
        obj = np.empty(shape, np.uint32); tri = np.empty(shape, np.uint32); dep = np.empty(shape, np.uint32); t = np.empty(shape, np.float32)
        up = C.POINTER(C.c_uint32)
        self._check(self.L.cgpt_trace_first_hits(self._ctx, C.byref(cam), width, height, r0, r1, N.TRACE_COUNTERS if counters else 0,
                                                 obj.ctypes.data_as(up), tri.ctypes.data_as(up), dep.ctypes.data_as(up),
                                                 t.ctypes.data_as(C.POINTER(C.c_float))))
        return obj, tri, dep, t

    def build_bvh(self, triangles, n_tris: int, build_option: int = N.BUILD_SAH_INTERVALS, initial_tri_indices=None):
        """BVH::Build (or, with initial_tri_indices = the current m_tri_indices, BVH::Rebuild) on the GPU for any BuildOption
        (ref: Source/BVH.cpp:11-59,204-297) and for BUILD_SAH_BINNED (not in the reference: DESIGN.md 5.10; finite positions of magnitude
        <= 1e30 only): returns (nodes[n,8] uint32 words in the reference's 32-byte layout, tri_indices[n_tris],
        max_depth, total_area).  triangles: ctypes pointer to n_tris cgpt_triangle (e.g. SceneDesc.triangles + tri_offset)."""
        nodes = np.zeros((max(2 * n_tris - 1, 1), 8), np.uint32)
        tri = np.zeros(n_tris, np.uint32)
        n_nodes = C.c_uint32(); depth = C.c_uint32(); area = C.c_float()
        init = None
        if initial_tri_indices is not None:
            init_arr = np.ascontiguousarray(initial_tri_indices, np.uint32)
            assert init_arr.shape == (n_tris,)
            init = init_arr.ctypes.data_as(C.POINTER(C.c_uint32))
        self._check(self.L.cgpt_bvh_build_ex(self._ctx, triangles, n_tris, build_option, init, nodes.ctypes.data_as(C.POINTER(N.BvhNode)), C.byref(n_nodes),
                                             tri.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(depth), C.byref(area)))
        return nodes[:n_nodes.value].copy(), tri, depth.value, area.value

    def synchronize(self):
        self._check(self.L.cgpt_synchronize(self._ctx))

    def close(self):
        if self._ctx:
            self.L.cgpt_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
