"""A host-side model of the state that in-place scene edits leave behind, and a seeded generator of edit sequences.

An operation is a tuple (name, arguments...) of plain data.  apply_to_model interprets it on a Model -- a host P.Scene edited through the
host mirrors (P.skin_triangles, P.morph_triangles, P.animate_joints, Scene.refit_mesh, Scene.rebuild_bvh, ...) plus what the device keeps
besides the scene: skins with their last matrices, skeletons, morph targets with their last weights, clips, the top-level switch and the
tuning knobs.  apply_to_device issues the same operation as a Renderer call.  The rules are the documents' (DESIGN.md 5.16, 5.24, 5.26,
5.28, 5.30, 5.32, 5.33 and the docstrings of renderer.py), stated once, here.  Nothing in this file touches a GPU; the device library
is only called by apply_to_device, which the GPU tests use."""
import ctypes as C
import dataclasses
import zlib

import numpy as np

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import anim_cases
import morph_cases
import skin_cases
from test_gpu_refit import BIG, GROUND, LAMP, SUN, WALL, octahedron
from test_gpu_skinning import OCTA, STRIP255, STRIP256, STRIP257, TRI, build_scene
from test_pose_batch_plan import crowd_scene

SCENE_KINDS = ("plain", "instanced", "crowd")
CROWD = 24                                                                     # two dozen characters: half of them can be reached in 16 steps
OPTIONS = (P.BUILD_NAIVE, P.BUILD_SAH_INTERVALS, P.BUILD_SAH_BINNED)           # BUILD_SAH_PRIMITIVES never splits: refused by the device
TUNING_DEFAULTS = {"skin_joints_lds": 1, "morph_leaf_order": 1, "morph_max_blocks": 1024}
IDENTITY = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
LAMP_MESH = ((2.0, 1.0, -1.0), 0.7)                                            # build_scene's mesh light

OP_KINDS = ("set_top_level", "set_tuning", "upload", "update_materials", "update_roughness", "update_transmission_roughness",
            "update_smooth_normals", "update_transforms", "update_primitive", "refit_mesh", "set_skin", "skin_mesh", "clear_skin",
            "set_morph_targets", "morph_mesh", "clear_morph_targets", "pose_objects", "set_skeleton", "create_clip", "destroy_clip",
            "animate_objects", "rebuild_mesh")
REFUSAL_KINDS = ("out_of_range", "no_skin_or_targets", "matrix_count", "weight_count", "not_finite", "skin_on_primitive",
                 "refit_count", "rebuild_without_tree", "named_twice", "destroyed_clip", "clip_joint_count", "skeleton_without_skin")
MUTANTS = ("pose_from_current", "set_skin_keeps_matrices", "set_morph_keeps_weights", "clear_morph_keeps_base", "refit_drops_skin",
           "rebuild_from_identity", "one_placement_only", "refused_batch_applies_prefix", "entry_without_weights_resets")
SKIN_JOINTS = {"rigid": 3, "bend": 2, "four": 6, "half": 2, "one_joint": 1, "wide": 1024}
MORPH_NAMES = ("one", "mix", "zeros_among", "flatten", "limit")


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def _shift(x, y, z):
    return np.float32([[1, 0, 0, x], [0, 1, 0, y], [0, 0, 1, z]])


def make_scene(kind, shared=True):
    """(scene, binds, materials, instanced): binds maps every object with triangles to its uploaded (n, 18) array.  shared=False gives
    the instanced scene's placements meshes of their own (the mutant whose poses move one placement only)."""
    if kind == "crowd":
        s = crowd_scene(CROWD)
        s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
        s.set_settings(P.Settings())
        binds = {k: P.triangles_from_arrays(*octahedron((0.5 * (k % 20) - 5.0, 0.5 * (k // 20) - 3.0, 0.0), 0.2)) for k in range(CROWD)}
        return s, binds, list(P.REFERENCE_MATERIALS), False
    s, binds = build_scene()
    binds[LAMP] = P.triangles_from_arrays(*octahedron(*LAMP_MESH))
    materials = list(P.REFERENCE_MATERIALS) + [P.Material(emissive=(1.0, 0.6, 0.3), intensity=6.0, is_light=True)]
    if kind == "instanced":
        places = ((OCTA, 1, _shift(1.5, 2.0, 0.5)), (OCTA, 0, _shift(-1.0, 2.5, -0.5)), (STRIP256, 0, _shift(0.5, 3.0, 1.0)), (STRIP256, 1, _shift(1.0, -1.5, 2.0)))
        for src, mat, xf in places:
            if shared:
                k = s.add_instance(src, mat, transform=xf)
            else:
                k = s.add_mesh(P.Mesh.from_arrays(binds[src].reshape(-1, 6), np.arange(3 * len(binds[src]), dtype=np.uint32)), mat, transform=xf)
            binds[k] = binds[src]
    elif kind != "plain":
        raise ValueError(kind)
    return s, binds, materials, kind == "instanced"


def scene_words(scene):
    """((head, geometry) bytes per object, bytes of the tables): what an upload of the scene reads, total_area and slice offsets left out
    -- poses keep the uploaded area by design and an offset is only a name.  geometry: nodes, triangles, leaf order."""
    d = scene.flatten()
    tris = np.ctypeslib.as_array(C.cast(d.triangles, C.POINTER(C.c_float)), shape=(max(d.n_triangles, 1), 18)) if d.n_triangles else np.zeros((0, 18), np.float32)
    nodes = np.ctypeslib.as_array(C.cast(d.nodes, C.POINTER(C.c_uint32)), shape=(max(d.n_nodes, 1), 8)) if d.n_nodes else np.zeros((0, 8), np.uint32)
    order = np.ctypeslib.as_array(d.tri_indices, shape=(max(d.n_triangles, 1),)) if d.n_triangles else np.zeros(0, np.uint32)
    per_object = []
    for k in range(d.n_objects):
        o = d.objects[k]
        head = np.float32([o.kind, o.mat_index, o.node_count, o.tri_count, *o.sphere_center, o.sphere_radius, *o.plane_normal, *o.plane_point]).tobytes()
        per_object.append((head, nodes[o.node_offset:o.node_offset + o.node_count].tobytes() + tris[o.tri_offset:o.tri_offset + o.tri_count].tobytes()
                           + order[o.tri_offset:o.tri_offset + o.tri_count].tobytes()))
    tables = (bytes(C.string_at(d.materials, C.sizeof(N.Material) * d.n_materials)) + scene.roughness(d.n_materials).tobytes()
              + scene.transmission_roughness(d.n_materials).tobytes() + scene.smooth_normals(d.n_objects).tobytes() + scene.transforms(d.n_objects).tobytes())
    return per_object, tables


def _blob(v):
    if isinstance(v, np.ndarray):
        return np.ascontiguousarray(v).tobytes()
    if isinstance(v, tuple):
        return b",".join(_blob(x) for x in v)
    return repr(v).encode()


# ---- the model ------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, kind, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.kind, self.mutant = kind, mutant
        self.scene, self.binds, self.materials, self.instanced = make_scene(kind, shared=mutant != "one_placement_only")
        d = self.scene.flatten()
        self.n_objects = d.n_objects
        self.kinds = [d.objects[k].kind for k in range(d.n_objects)]
        self.mat_index = [d.objects[k].mat_index for k in range(d.n_objects)]
        self.lights = {d.light_indices[k] for k in range(d.n_lights)}
        self.n_tris = [len(self.binds[k]) if k in self.binds else 0 for k in range(d.n_objects)]
        # the objects that share one device copy after an instanced upload: object -> the group's first member
        first = {}
        self.group = [first.setdefault(id(self.binds[k]), k) if (self.instanced and k in self.binds and self.kinds[k] == N.OBJECT_MESH) else k for k in range(d.n_objects)]
        self.tris = {k: self.binds[k].copy() for k in self.binds}              # current triangles, original order, per object
        self.skins, self.morphs, self.clips = {}, {}, {}
        self.top_level = False
        self.tuning = dict(TUNING_DEFAULTS)
        self.last_refusal = None                                               # the REFUSAL_KINDS name of the last refused operation
        self.last_area = None                                                  # Scene.bvh_info(obj).total_area after the last accepted refit of a mesh
        self._shadow = {}                                                      # mutant rebuild_from_identity: group -> (scene, tree built afresh)
        self.uploaded = scene_words(self.scene)[0]

    def close(self):
        for s, _ in self._shadow.values():
            s.close()
        self.scene.close()

    # -- what the tests read -------------------------------------------------------------------------------------------------------
    def mesh_objects(self):
        return [k for k in range(self.n_objects) if self.kinds[k] == N.OBJECT_MESH]

    def members(self, obj):
        return [k for k in range(self.n_objects) if self.group[k] == self.group[obj]]

    def scene_bytes(self):
        per_object, tables = scene_words(self.scene)
        for g, (shadow, _) in self._shadow.items():
            for k in self.members(g):
                per_object[k] = (per_object[k][0], scene_words(shadow)[0][0][1])   # the tree built afresh stands in for the scene's
        return b"".join(h + g for h, g in per_object) + tables

    def state_bytes(self):
        """the scene and everything kept besides it: equal before and after a step that changed nothing"""
        h = [self.scene_bytes(), repr((self.top_level, sorted(self.tuning.items()), sorted((k, v is not None) for k, v in self.clips.items()))).encode()]
        for name, table in (("skin", self.skins), ("morph", self.morphs)):
            for obj in sorted(table):
                h.append(f"{name}{obj}".encode())
                h += [_blob(table[obj][key]) for key in sorted(table[obj])]
        return b"|".join(h)

    def differing_meshes(self):
        now = scene_words(self.scene)[0]
        return [k for k in self.mesh_objects() if now[k][1] != self.uploaded[k][1]]

    def posed_skins(self):
        return {obj: sk["M"] for obj, sk in self.skins.items() if sk["M"] is not None}

    # -- geometry ------------------------------------------------------------------------------------------------------------------
    def _refit(self, obj, t):
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 18)
        self.scene.refit_mesh(obj, t)                                          # an instance shares its MeshBVH: every placement follows
        targets = self.members(obj) if self.mutant != "one_placement_only" else [obj]
        for k in targets:
            self.tris[k] = t.copy()
        g = self.group[obj]
        if g in self._shadow:
            self._shadow[g][0].refit_mesh(0, t)

    def _pose(self, obj):
        """DESIGN.md 5.28, "Fusion with the skin": always from the base or the bind pose, never from the current triangles"""
        sk, mo = self.skins.get(obj), self.morphs.get(obj)
        from_current = self.mutant == "pose_from_current"
        if mo is not None:
            b = P.morph_triangles(self.tris[obj] if from_current else mo["base"], mo["deltas"], mo["w"])
        else:
            b = self.tris[obj] if from_current else sk["bind"]
        if sk is not None and sk["M"] is not None:
            b = P.skin_triangles(b, sk["joints"], sk["weights"], sk["M"])
        self._refit(obj, b)

    # -- checks shared by the single calls and the batches ----------------------------------------------------------------------------
    def _in_range(self, obj):
        return 0 <= int(obj) < self.n_objects

    def _check_skin_pose(self, obj, m):
        if not self._in_range(obj):
            return "out_of_range"
        if obj not in self.skins:
            return "no_skin_or_targets"
        m = np.asarray(m, np.float32).reshape(-1, 12)
        if m.shape[0] != self.skins[obj]["n_joints"]:
            return "matrix_count"
        return None if np.isfinite(m).all() else "not_finite"

    def _check_morph_pose(self, obj, w):
        if not self._in_range(obj):
            return "out_of_range"
        if obj not in self.morphs:
            return "no_skin_or_targets"
        w = np.asarray(w, np.float32).ravel()
        if w.size != len(self.morphs[obj]["deltas"]):
            return "weight_count"
        return None if np.isfinite(w).all() else "not_finite"

    def _takes_skin(self, obj, n):
        if not self._in_range(obj):
            return "out_of_range"
        if self.kinds[obj] in (N.OBJECT_SPHERE, N.OBJECT_PLANE) or obj in self.lights:
            return "skin_on_primitive"
        return None if n == self.n_tris[obj] else "refit_count"

    def _check_batch(self, entries):
        """entries: (obj, matrices or None, weights or None); every refusal comes before the first write"""
        seen = {}
        for obj, m, w in entries:
            if not self._in_range(obj):
                return "out_of_range"
            if m is None and w is None:
                return "no_skin_or_targets"
            for bad in (self._check_skin_pose(obj, m) if m is not None else None, self._check_morph_pose(obj, w) if w is not None else None):
                if bad:
                    return bad
            if self.group[obj] in seen:
                return "named_twice"
            seen[self.group[obj]] = obj
        return None

    def _apply_batch(self, entries):
        for obj, m, w in entries:                                             # morph_mesh, then skin_mesh, of every entry in turn
            if w is not None:
                self.morphs[obj]["w"] = np.asarray(w, np.float32).ravel().copy()
            elif self.mutant == "entry_without_weights_resets" and obj in self.morphs:
                self.morphs[obj]["w"] = np.zeros_like(self.morphs[obj]["w"])
            if m is not None:
                self.skins[obj]["M"] = np.asarray(m, np.float32).reshape(-1, 12).copy()
            self._pose(obj)

    def _batch(self, entries):
        bad = self._check_batch(entries)
        if bad and self.mutant == "refused_batch_applies_prefix":
            good = []
            for e in entries:
                if self._check_batch(good + [e]):
                    break
                good.append(e)
            self._apply_batch(good)
        if bad:
            return bad
        self._apply_batch(entries)
        return None

    # -- one method an operation: returns None (accepted) or the refusal's kind ----------------------------------------------------------
    def op_set_top_level(self, on):
        self.top_level = bool(on)

    def op_set_tuning(self, name, value):
        self.tuning[name] = int(value)

    def op_upload(self):
        """drops skins, targets and skeletons; keeps clips, the top-level switch and tuning; transforms, smooth flags and both roughnesses
        are reset and Renderer.upload re-applies the Scene's, which are the model's"""
        self.skins.clear(); self.morphs.clear()

    def op_update_materials(self, materials):
        for k, m in enumerate(materials):
            self.scene.set_material(k, m)
        self.materials = list(materials)

    def op_update_roughness(self, values):
        for k, v in enumerate(np.asarray(values, np.float32)):
            self.scene.set_roughness(k, float(v))
            self.materials[k] = dataclasses.replace(self.materials[k], roughness=float(v))

    def op_update_transmission_roughness(self, values):
        for k, v in enumerate(np.asarray(values, np.float32)):
            self.scene.set_transmission_roughness(k, float(v))
            self.materials[k] = dataclasses.replace(self.materials[k], transmission_roughness=float(v))

    def op_update_smooth_normals(self, flags):
        for k, f in enumerate(np.asarray(flags, np.uint32)):
            self.scene.set_smooth_normals(k, bool(f))

    def op_update_transforms(self, matrices):
        for k, m in enumerate(np.asarray(matrices, np.float32).reshape(-1, 12)):
            self.scene.set_transform(k, m)

    def op_update_primitive(self, obj, mat_index, kw):
        self.scene.update_primitive(obj, **kw)

    def op_refit_mesh(self, obj, t):
        if not self._in_range(obj):
            return "out_of_range"
        if self.kinds[obj] in (N.OBJECT_SPHERE, N.OBJECT_PLANE):
            return "skin_on_primitive"
        if len(t) != self.n_tris[obj]:
            return "refit_count"
        self._refit(obj, t)                                                    # skin and targets are kept: the next pose starts from bind or base again
        self.last_area = self.scene.bvh_info(obj).total_area if self.kinds[obj] == N.OBJECT_MESH else None
        if self.mutant == "refit_drops_skin":
            self.skins.pop(obj, None)

    def op_set_skin(self, obj, bind, joints, weights, n_joints):
        bad = self._takes_skin(obj, len(bind))
        if bad:
            return bad
        old = self.skins.get(obj)
        keep = old["M"] if (self.mutant == "set_skin_keeps_matrices" and old is not None and old["n_joints"] == n_joints) else None
        self.skins[obj] = dict(bind=bind, joints=joints, weights=weights, n_joints=int(n_joints), M=keep, skeleton=None)   # forgets the pose, drops the skeleton

    def op_skin_mesh(self, obj, m):
        bad = self._check_skin_pose(obj, m)
        if bad:
            return bad
        self.skins[obj]["M"] = np.asarray(m, np.float32).reshape(-1, 12).copy()
        self._pose(obj)

    def op_clear_skin(self, obj):
        self.skins.pop(obj, None)                                              # the geometry stays where it is

    def op_set_morph_targets(self, obj, base, deltas):
        bad = self._takes_skin(obj, len(base))
        if bad:
            return bad
        old = self.morphs.get(obj)
        w = np.zeros(len(deltas), np.float32)
        if self.mutant == "set_morph_keeps_weights" and old is not None and len(old["w"]) == len(w):
            w = old["w"]
        self.morphs[obj] = dict(base=base, deltas=deltas, w=w)

    def op_morph_mesh(self, obj, w):
        bad = self._check_morph_pose(obj, w)
        if bad:
            return bad
        self.morphs[obj]["w"] = np.asarray(w, np.float32).ravel().copy()
        self._pose(obj)

    def op_clear_morph_targets(self, obj):
        mo = self.morphs.pop(obj, None)                                        # the geometry stays; a skin goes back to its own bind pose at its next skin_mesh
        if mo is not None and self.mutant == "clear_morph_keeps_base" and obj in self.skins:
            self.skins[obj]["bind"] = P.morph_triangles(mo["base"], mo["deltas"], mo["w"])

    def op_pose_objects(self, entries):
        return self._batch(entries)

    def op_set_skeleton(self, obj, parents, inverse_bind, rest, root):
        if not self._in_range(obj):
            return "out_of_range"
        if obj not in self.skins:
            return "skeleton_without_skin"
        if len(parents) != self.skins[obj]["n_joints"]:
            return "matrix_count"
        self.skins[obj]["skeleton"] = (parents, inverse_bind, rest, root)

    def op_create_clip(self, slot, n_joints, channels, times, values):
        self.clips[slot] = (n_joints, channels, times, values)

    def op_destroy_clip(self, slot):
        if self.clips.get(slot) is None:
            return "destroyed_clip"
        self.clips[slot] = None

    def op_animate_objects(self, entries):
        """pose_objects with P.animate_joints(skeleton, clip, t)"""
        posed = []
        for obj, slot, t, w in entries:
            if not self._in_range(obj):
                return "out_of_range"
            if obj not in self.skins or self.skins[obj]["skeleton"] is None:
                return "no_skin_or_targets"
            clip = self.clips.get(slot)
            if clip is None:
                return "destroyed_clip"
            if clip[0] != self.skins[obj]["n_joints"]:
                return "clip_joint_count"
            if not np.isfinite(np.float32(t)):
                return "not_finite"
            posed.append((obj, P.animate_joints(self.skins[obj]["skeleton"], clip, t), w))
        return self._batch(posed)

    def op_rebuild_mesh(self, obj, option):
        if not self._in_range(obj):
            return "out_of_range"
        if self.kinds[obj] != N.OBJECT_MESH:
            return "rebuild_without_tree"
        self.scene.rebuild_bvh(obj, option)                                    # over the current triangles and leaf order; everything else is kept
        if self.mutant == "rebuild_from_identity":
            g = self.group[obj]
            if g in self._shadow:
                self._shadow.pop(g)[0].close()
            shadow = P.Scene()
            shadow.add_material(P.Material())
            t = self.tris[obj]
            shadow.add_mesh(P.Mesh.from_arrays(t.reshape(-1, 6), np.arange(3 * len(t), dtype=np.uint32)), 0, option)
            self._shadow[g] = (shadow, option)


def apply_to_model(model, op):
    """"accepted" or "refused"; a refused operation changes nothing and leaves its kind in model.last_refusal"""
    bad = getattr(model, "op_" + op[0])(*op[1:])
    model.last_refusal = bad
    return "refused" if bad else "accepted"


def apply_to_device(renderer, op, status, model=None):
    """The Renderer call of `op`.  status: what apply_to_model said -- "refused" expects P.DeviceError, "accepted" expects success.
    Returns what the call returned.  model: the one an `upload` takes its scene from.  Clip handles are kept on the renderer by slot."""
    handles = renderer.__dict__.setdefault("_edit_model_clips", {})
    name, args = op[0], op[1:]

    def call():
        if name == "upload":
            return renderer.upload(model.scene, instanced=model.instanced)
        if name == "set_tuning":
            return renderer.set_tuning(**{args[0]: args[1]})
        if name == "update_materials":
            s = P.Scene()
            for m in args[0]:
                s.add_material(m)
            try:
                return renderer.update_materials(s)
            finally:
                s.close()
        if name == "update_primitive":
            return renderer.update_primitive(args[0], args[1], **args[2])
        if name == "set_skeleton":
            return renderer.set_skeleton(args[0], args[1], args[2], args[3], args[4])
        if name == "create_clip":
            handles[args[0]] = renderer.create_clip(*args[1:])
            return handles[args[0]]
        if name == "destroy_clip":
            return renderer.destroy_clip(handles[args[0]])
        if name == "animate_objects":
            return renderer.animate_objects([(obj, handles[slot], t, w) for obj, slot, t, w in args[0]])
        return getattr(renderer, name)(*args)

    if status == "refused":
        try:
            call()
        except P.DeviceError as e:
            return e
        raise AssertionError(f"the device accepted what the model refuses: {describe(op)}")
    try:
        return call()
    except P.DeviceError as e:
        raise AssertionError(f"the device refused what the model accepts: {describe(op)}: {e}") from e


def describe(op):
    """one line: the call's name, its scalars, and shape and checksum of every array"""
    def show(v):
        if isinstance(v, np.ndarray):
            return f"<{v.dtype}{list(v.shape)} crc {zlib.crc32(np.ascontiguousarray(v).tobytes()):08x}>" if v.size > 4 else repr(v.tolist())
        if isinstance(v, (list, tuple)):
            return "[" + ", ".join(show(x) for x in v) + "]"
        if isinstance(v, dict):
            return "{" + ", ".join(f"{k}: {show(x)}" for k, x in v.items()) + "}"
        return repr(v)
    return f"{op[0]}({', '.join(show(a) for a in op[1:])})"


def same_operation(a, b):
    def eq(x, y):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            return isinstance(x, np.ndarray) and isinstance(y, np.ndarray) and x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        if isinstance(x, (list, tuple)):
            return isinstance(y, (list, tuple)) and len(x) == len(y) and all(eq(p, q) for p, q in zip(x, y))
        if isinstance(x, dict):
            return isinstance(y, dict) and x.keys() == y.keys() and all(eq(x[k], y[k]) for k in x)
        return type(x) is type(y) and x == y
    return eq(a, b)


# ---- the generator ---------------------------------------------------------------------------------------------------------------
class _Done(Exception):
    pass


def eased_matrices(m, a):
    """test_gpu_pose_batch.eased: the matrices a of the way to the identity"""
    return (np.float32(1 - a) * m + np.float32(a) * IDENTITY).astype(np.float32)


class _Generator:
    def __init__(self, seed, n_steps, kind, knobs=None):
        self.rng = np.random.default_rng([int(seed), SCENE_KINDS.index(kind)])
        self.seed, self.n_steps, self.kind = int(seed), n_steps, kind
        self.model = Model(kind)
        self.model.tuning.update(knobs or {})
        self.ops, self.statuses = [], []
        self.budget = max(n_steps // 4 - 1, 0)                                 # refused on purpose; one step of room for a step without effect
        self.weak = 0                                                          # steps refused or without effect so far
        self.refusals = 0
        self.next_slot = 0
        self.decks = {}
        self.case = {}                                                         # obj -> name of its skin's pose in skin_cases; ("morph", obj) -> (name, seed)
        self.touched = set()                                                   # groups whose geometry an accepted step of this sequence edited
        m = self.model
        self.posable = [k for k in range(m.n_objects) if m.n_tris[k] and k not in m.lights]
        self.rebuildable = [k for k in self.posable if m.kinds[k] == N.OBJECT_MESH]

    # -- plumbing ------------------------------------------------------------------------------------------------------------------
    def emit(self, op, edits=()):
        if len(self.ops) >= self.n_steps:
            raise _Done
        if self.ops and same_operation(op, self.ops[-1]):                      # never a pure repeat of the previous operation
            return None
        before = self.model.state_bytes()
        status = apply_to_model(self.model, op)
        if status == "refused" or self.model.state_bytes() == before:
            self.weak += 1
        elif edits:
            self.touched.update(self.model.group[o] for o in edits)
        self.ops.append(op); self.statuses.append(status)
        if len(self.ops) >= self.n_steps:
            raise _Done
        return status

    def has(self, o, want):
        sk, mo = self.model.skins.get(o), self.model.morphs.get(o)
        return {"skin": sk is not None, "morph": mo is not None, "both": sk is not None and mo is not None,
                "posed": sk is not None and sk["M"] is not None, "rigged": sk is not None and sk["skeleton"] is not None,
                "both_posed": sk is not None and mo is not None and sk["M"] is not None,
                "moved": sk is not None and mo is not None and bool(mo["w"].any())}[want]

    def pick(self, cands, want=None):
        """one of cands; mostly one that already has the state the motif needs, so that its steps go to edits and not to installing"""
        cands = list(cands)
        ready = [o for o in cands if want and self.has(o, want)]
        if ready and self.rng.random() < 0.85:
            cands = ready
        return int(cands[self.rng.integers(len(cands))])

    def draw(self, deck, items, start):
        """the next of `items` in their cyclic order, the first one `start`: a sequence goes through them all before it repeats one, and
        sequences of different seeds start at different ones, so that a handful of sequences reaches every item"""
        k = self.decks.get(deck, start % len(items))
        self.decks[deck] = (k + 1) % len(items)
        return items[k]

    def ease(self):
        return float(self.rng.choice([0.0, 0.2, 0.35, 0.5, 0.65, 0.8]))

    # -- draws -----------------------------------------------------------------------------------------------------------------------
    def skin_op(self, obj, name=None, other_than=None, same_as=None):
        names = [n for n in skin_cases.POSES if (other_than is None or SKIN_JOINTS[n] != other_than) and (same_as is None or SKIN_JOINTS[n] == same_as)]
        name = name or str(self.rng.choice(names))
        seed = int(self.rng.integers(1000))
        j, w, n_joints, _ = skin_cases.make_case(name, self.model.binds[obj], seed=seed)
        self.case[obj] = (name, seed)
        return ("set_skin", obj, self.model.binds[obj], j, w, n_joints)

    def matrices(self, obj):
        name, seed = self.case[obj]
        return eased_matrices(skin_cases.make_case(name, self.model.binds[obj], seed=seed)[3], self.ease())

    def morph_op(self, obj, name=None):
        names = [n for n in MORPH_NAMES if n != "limit" or self.model.n_tris[obj] <= 257]
        name = name or str(self.rng.choice(names, p=[(0.4 if n == "limit" else 1.0) / (len(names) - 0.6 * ("limit" in names)) for n in names]))
        seed = int(self.rng.integers(1000))
        base, deltas, _ = morph_cases.make_case(name, self.model.binds[obj], seed=seed)
        self.case["morph", obj] = (name, seed)
        return ("set_morph_targets", obj, base, deltas)

    def weights(self, obj):
        name, seed = self.case["morph", obj]
        w = morph_cases.make_case(name, self.model.binds[obj][:1], seed=seed)[2]   # the weights do not depend on the mesh
        return (np.float32(1 - 0.9 * self.ease()) * w).astype(np.float32)

    def deformed(self, obj):
        t = self.model.binds[obj].copy().reshape(-1, 3, 6)
        t[..., :3] = t[..., :3] * self.rng.uniform(0.9, 1.15, 3).astype(np.float32) + self.rng.uniform(-0.3, 0.3, 3).astype(np.float32)
        return t.reshape(-1, 18)

    def rig(self, obj):
        n = self.model.skins[obj]["n_joints"]
        shape = str(self.rng.choice(["tree", "chain", "reversed", "two_roots"])) if n <= 6 else "tree"
        return anim_cases.rig(n, int(self.rng.integers(100)), shape, bool(self.rng.integers(2)))

    def clip_for(self, n_joints, alive=True):
        for slot, c in self.model.clips.items():
            if c is not None and c[0] == n_joints:
                return slot
        return None

    # -- state the motifs need -----------------------------------------------------------------------------------------------------------
    def ensure_skin(self, obj):
        if obj not in self.model.skins:
            self.emit(self.skin_op(obj))

    def ensure_morph(self, obj, moved=False):
        if obj not in self.model.morphs:
            self.emit(self.morph_op(obj))
        if moved and not self.model.morphs[obj]["w"].any():
            self.emit(("morph_mesh", obj, self.weights(obj)), edits=(obj,))

    def ensure_posed(self, obj):
        self.ensure_skin(obj)
        if self.model.skins[obj]["M"] is None:
            self.emit(("skin_mesh", obj, self.matrices(obj)), edits=(obj,))

    def ensure_rigged(self, obj):
        """a skin, a skeleton and a clip of its joint count: the clip's slot"""
        self.ensure_skin(obj)
        n = self.model.skins[obj]["n_joints"]
        slot = self.clip_for(n)
        if self.model.skins[obj]["skeleton"] is None or slot is None:
            skeleton, clip, _ = self.rig(obj)
            if slot is None:
                slot = self.next_slot
                self.next_slot += 1
                self.emit(("create_clip", slot) + tuple(clip))
            self.emit(("set_skeleton", obj) + tuple(skeleton))
        return slot

    def with_state(self, both=False):
        m = self.model
        if both:
            return [o for o in self.posable if o in m.skins and o in m.morphs]
        return [o for o in self.posable if o in m.skins or o in m.morphs]

    def entry(self, obj, partial=False):
        """a pose_objects entry for an object with state; partial: one of the two arrays left out where it has both"""
        m = self.model
        mat = self.matrices(obj) if obj in m.skins else None
        w = self.weights(obj) if obj in m.morphs else None
        if partial and mat is not None and w is not None:
            if self.rng.integers(2):
                mat = None
            else:
                w = None
        return (obj, mat, w)

    def one_per_group(self, objs):
        seen, out = set(), []
        for o in objs:
            if self.model.group[o] not in seen:
                seen.add(self.model.group[o])
                out.append(o)
        return out

    # -- motifs: the ordered pairs the CPU test asks for (tests/test_edit_model.py) ----------------------------------------------------
    def m_rebuild_morph(self):
        o = self.pick(self.rebuildable, "morph")
        if o not in self.model.morphs:
            want = int(self.rng.integers(2))
            if self.model.tuning["morph_leaf_order"] != want:
                self.emit(("set_tuning", "morph_leaf_order", want))
            self.emit(self.morph_op(o))                                        # installed in the old leaf order: the rebuild permutes the planes
        self.emit(("rebuild_mesh", o, int(self.rng.choice(OPTIONS))), edits=(o,))
        self.emit(("morph_mesh", o, self.weights(o)), edits=(o,))

    def m_rebuild_skin(self):
        o = self.pick(self.rebuildable, "skin")
        self.ensure_skin(o)
        self.emit(("rebuild_mesh", o, int(self.rng.choice(OPTIONS))), edits=(o,))
        self.emit(("skin_mesh", o, self.matrices(o)), edits=(o,))

    def m_rebuild_refit_rebuild(self):
        o = self.pick(self.rebuildable)
        first, second = (int(x) for x in self.rng.choice(OPTIONS, 2, replace=False))
        self.emit(("rebuild_mesh", o, first), edits=(o,))
        self.emit(("refit_mesh", o, self.deformed(o)), edits=(o,))
        self.emit(("rebuild_mesh", o, second), edits=(o,))

    def m_set_morph_skin(self):
        o = self.pick(self.posable, "moved")
        self.ensure_posed(o)
        self.ensure_morph(o, moved=True)                                       # targets with weights to forget
        old = self.case.get(("morph", o))
        self.emit(self.morph_op(o, name=old[0] if old and o in self.model.morphs else None))   # as many targets as before: the weights must still restart at zero
        self.emit(("skin_mesh", o, self.matrices(o)), edits=(o,))

    def m_clear_morph_skin(self):
        o = self.pick(self.posable, "moved")
        self.ensure_skin(o)
        self.ensure_morph(o, moved=True)
        self.emit(("clear_morph_targets", o))
        self.emit(("skin_mesh", o, self.matrices(o)), edits=(o,))

    def m_refit_skin(self):
        o = self.pick(self.posable, "skin")
        self.ensure_skin(o)
        self.emit(("refit_mesh", o, self.deformed(o)), edits=(o,))
        self.emit(("skin_mesh", o, self.matrices(o)), edits=(o,))

    def m_replace_skin_morph(self):
        o = self.pick(self.posable, "both_posed")
        self.ensure_posed(o)
        self.ensure_morph(o)
        n = self.model.skins[o]["n_joints"]
        self.emit(self.skin_op(o, other_than=n) if self.rng.random() < 0.5 else self.skin_op(o, same_as=n))
        self.emit(("morph_mesh", o, self.weights(o)), edits=(o,))

    def m_clear_skin_morph(self):
        o = self.pick(self.posable, "both")
        self.ensure_skin(o)
        self.ensure_morph(o)
        self.emit(("clear_skin", o))
        self.emit(("morph_mesh", o, self.weights(o)), edits=(o,))

    def m_animate_then_weights(self):
        o = self.pick(self.posable, "rigged")
        slot = self.ensure_rigged(o)
        self.ensure_morph(o)
        self.emit(("animate_objects", [(o, slot, float(self.rng.uniform(-0.2, 1.2)), self.weights(o) if self.rng.integers(2) else None)]), edits=(o,))
        others = [p for p in self.one_per_group(self.with_state()) if self.model.group[p] != self.model.group[o]][:3]
        self.emit(("pose_objects", [(o, None, self.weights(o))] + [self.entry(p, partial=True) for p in others]), edits=[o] + others)

    def m_animate_skin(self):
        o = self.pick(self.posable, "rigged")
        slot = self.ensure_rigged(o)
        self.emit(("animate_objects", [(o, slot, float(self.rng.uniform(-0.2, 1.2)), None)]), edits=(o,))
        self.emit(("skin_mesh", o, self.matrices(o)), edits=(o,))
        if self.refusals < self.budget:
            self.refused(kind="clip_joint_count" if self.seed % 2 else "destroyed_clip")

    def m_upload_animate(self):
        o = self.pick(self.posable)
        name = str(self.rng.choice(["bend", "half", "rigid", "four", "one_joint"]))
        n = SKIN_JOINTS[name]
        slot = self.clip_for(n)
        skeleton, clip, _ = anim_cases.rig(n, int(self.rng.integers(100)), "tree", bool(self.rng.integers(2)))
        if slot is None:
            slot = self.next_slot
            self.next_slot += 1
            self.emit(("create_clip", slot) + tuple(clip))                     # before the upload: a clip survives it, a skin does not
        self.emit(("upload",))
        self.emit(self.skin_op(o, name=name))
        self.emit(("set_skeleton", o) + tuple(skeleton))
        self.emit(("animate_objects", [(o, slot, float(self.rng.uniform(0.0, 1.0)), None)]), edits=(o,))

    def m_transforms_pose(self):
        m = self.model
        if not m.top_level:
            self.emit(("set_top_level", True))
        xf = np.tile(IDENTITY, (m.n_objects, 1))
        movable = [k for k in self.posable]
        for k in self.rng.choice(movable, min(3, len(movable)), replace=False):
            a = np.eye(3) + self.rng.uniform(-0.15, 0.15, (3, 3))
            xf[k] = np.concatenate([a, self.rng.uniform(-0.4, 0.4, (3, 1))], axis=1).astype(np.float32).reshape(12)
        have = self.with_state()
        o = self.pick(have) if have else self.pick(self.posable)
        if not have:
            self.ensure_skin(o)
        self.emit(("update_transforms", xf))
        e = self.entry(o)
        kind = int(self.rng.integers(3))
        if kind == 0 or (e[1] is not None and e[2] is not None):
            self.emit(("pose_objects", [e]), edits=(o,))
        elif e[1] is not None:
            self.emit(("skin_mesh", o, e[1]), edits=(o,))
        else:
            self.emit(("morph_mesh", o, e[2]), edits=(o,))

    def m_refused_then_accepted_batch(self):
        first = self.pick(self.posable, "both")
        self.ensure_skin(first)
        self.ensure_morph(first)
        rest = [o for o in self.one_per_group(self.with_state()) if self.model.group[o] != self.model.group[first]]
        if not rest:
            o = self.pick([p for p in self.posable if self.model.group[p] != self.model.group[first]])
            self.ensure_skin(o)
            rest = [o]
        rest = rest[:4]
        last = rest[-1]
        good = [(first, self.matrices(first), None)] + [self.entry(o) for o in rest[:-1]]
        self.refused(("batch", last, good))
        accepted = [(first, None, self.weights(first))] + [self.entry(o) for o in rest]   # over the same objects; `first` by its weights alone
        self.emit(("pose_objects", accepted), edits=[first] + rest)

    def m_batch(self):
        have = self.one_per_group(self.rng.permutation(self.with_state()).tolist())
        if len(have) < 2:
            for _ in range(2):
                o = self.pick([p for p in self.posable if p not in self.model.skins and p not in self.model.morphs] or self.posable)
                self.emit(self.skin_op(o) if self.rng.random() < 0.6 else self.morph_op(o))
            have = self.one_per_group(self.with_state())
        self.emit(("pose_objects", [self.entry(o, partial=bool(self.rng.integers(2))) for o in have]), edits=have)

    # -- the rest of the calls, one step each ----------------------------------------------------------------------------------------------
    def m_single(self):
        m, rng = self.model, self.rng
        kind = self.draw("singles", ["materials", "roughness", "transmission", "smooth", "primitive", "top", "tuning", "destroy", "upload", "clear"], self.seed)
        if kind == "materials":
            k = int(rng.integers(2))
            mats = list(m.materials)
            mats[k] = dataclasses.replace(mats[k], albedo=tuple(float(x) for x in rng.uniform(0.2, 0.9, 3).round(3)), specular=float(rng.choice([0.0, 0.2, 0.5])),
                                          roughness=float(rng.choice([0.0, 0.3])))
            self.emit(("update_materials", mats))
        elif kind == "roughness":
            v = np.array([x.roughness for x in m.materials], np.float32)
            v[int(rng.integers(2))] = np.float32(rng.choice([0.15, 0.4, 0.6]))
            self.emit(("update_roughness", v))
        elif kind == "transmission":
            v = np.array([x.transmission_roughness for x in m.materials], np.float32)
            v[3] = np.float32(rng.choice([0.1, 0.25, 0.5]))
            self.emit(("update_transmission_roughness", v))
        elif kind == "smooth":
            f = m.scene.smooth_normals(m.n_objects)
            for k in rng.choice(self.posable, min(2, len(self.posable)), replace=False):
                f[k] ^= 1
            self.emit(("update_smooth_normals", f))
        elif kind == "primitive":
            spheres = [k for k in range(m.n_objects) if m.kinds[k] == N.OBJECT_SPHERE]
            planes = [k for k in range(m.n_objects) if m.kinds[k] == N.OBJECT_PLANE]
            if planes and rng.integers(2):
                k = planes[0]
                self.emit(("update_primitive", k, m.mat_index[k], dict(normal=(0.0, float(rng.choice([0.0, 0.6])), float(rng.choice([1.0, 0.8]))), point=(0.0, 0.0, round(float(rng.uniform(-30, -12)), 1)))))
            else:
                k = spheres[0]
                self.emit(("update_primitive", k, m.mat_index[k], dict(center=tuple(float(x) for x in rng.uniform(6.0, 11.0, 3).round(2)), radius=round(float(rng.uniform(3.0, 5.5)), 2))))
        elif kind == "top":
            self.emit(("set_top_level", not m.top_level))
        elif kind == "tuning":
            name = str(rng.choice(list(TUNING_DEFAULTS)))
            value = {"skin_joints_lds": 1 - m.tuning["skin_joints_lds"], "morph_leaf_order": 1 - m.tuning["morph_leaf_order"],
                     "morph_max_blocks": int(rng.choice([v for v in (1, 2, 3, 1024) if v != m.tuning["morph_max_blocks"]]))}[name]
            self.emit(("set_tuning", name, value))
        elif kind == "destroy":
            alive = [s for s, c in m.clips.items() if c is not None]
            if not alive:
                alive = [self.next_slot]
                self.next_slot += 1
                self.emit(("create_clip", alive[0]) + tuple(anim_cases.rig(int(rng.choice([1, 2, 3, 6])), int(rng.integers(100)))[1]))
            self.emit(("destroy_clip", int(rng.choice(alive))))
        elif kind == "clear":
            have = self.with_state()
            if have:
                o = int(rng.choice(have))
                self.emit(("clear_skin", o) if o in m.skins and (o not in m.morphs or rng.integers(2)) else ("clear_morph_targets", o))
        elif kind == "upload":
            self.emit(("upload",))

    # -- refused calls: only the kinds the per-feature tests exercise one at a time -------------------------------------------------------
    def refused(self, what=None, kind=None):
        m, rng = self.model, self.rng
        batch = what
        self.refusals += 1
        if batch is not None:                                                  # a batch whose last entry is bad, accepted entries in front
            _, last, good = batch
            bad_kinds = ["named_twice", "out_of_range"]
            if last in m.skins:
                bad_kinds += ["matrix_count", "not_finite"]
            if last in m.morphs:
                bad_kinds += ["weight_count"]
            kind = bad_kinds[(self.seed + self.refusals) % len(bad_kinds)]
            e = self.entry(last)
            if kind == "named_twice":
                twin = [k for k in m.members(good[0][0]) if k != good[0][0]]
                return self.emit(("pose_objects", good + [e, (twin[0] if twin and twin[0] in m.skins else good[0][0], good[0][1], None)]))
            if kind == "out_of_range":
                return self.emit(("pose_objects", good + [e, (m.n_objects + 3, e[1], e[2])]))
            if kind == "matrix_count":
                bad = (last, np.concatenate([e[1], e[1][:1]]), e[2])
            elif kind == "not_finite":
                nan = e[1].copy(); nan[-1, 5] = np.nan
                bad = (last, nan, e[2])
            else:
                bad = (last, e[1], np.concatenate([e[2], np.float32([0.5])]))
            return self.emit(("pose_objects", good + [bad]))
        skinned = [o for o in self.posable if o in m.skins]
        morphed = [o for o in self.posable if o in m.morphs]
        plain = [o for o in self.posable if o not in m.skins and o not in m.morphs]
        rigged = [p for p in skinned if m.skins[p]["skeleton"] is not None]
        possible = {"no_skin_or_targets": plain, "matrix_count": skinned, "weight_count": morphed, "not_finite": skinned or morphed, "named_twice": skinned or morphed,
                    "destroyed_clip": rigged, "clip_joint_count": rigged, "skeleton_without_skin": [q for q in self.posable if q not in m.skins]}
        first = 5 * self.seed + 7 * SCENE_KINDS.index(self.kind) + self.refusals       # the kinds in turn, the first one the state allows
        kind = kind or next(k for k in (REFUSAL_KINDS[(first + t) % len(REFUSAL_KINDS)] for t in range(len(REFUSAL_KINDS))) if possible.get(k, True))
        o = int(rng.choice(self.posable))
        if kind == "out_of_range":
            bad = m.n_objects + int(rng.integers(0, 4))
            j, w, n_joints, _ = skin_cases.make_case("bend", m.binds[o], seed=2)
            op = [("refit_mesh", bad, m.binds[o]), ("rebuild_mesh", bad, P.BUILD_SAH_BINNED), ("set_skin", bad, m.binds[o], j, w, n_joints),
                  ("skin_mesh", bad, np.tile(IDENTITY, (2, 1)))][int(rng.integers(4))]
        elif kind == "no_skin_or_targets" and plain:
            p = int(rng.choice(plain))
            op = ("skin_mesh", p, np.tile(IDENTITY, (2, 1))) if rng.integers(2) else ("morph_mesh", p, np.float32([0.5]))
        elif kind == "matrix_count" and skinned:
            p = int(rng.choice(skinned))
            mat = self.matrices(p)
            op = ("skin_mesh", p, np.concatenate([mat, mat[:1]]) if rng.integers(2) or len(mat) == 1 else mat[:-1])
        elif kind == "weight_count" and morphed:
            p = int(rng.choice(morphed))
            op = ("morph_mesh", p, np.concatenate([self.weights(p), np.float32([0.25])]))
        elif kind == "not_finite" and (skinned or morphed):
            if skinned and (not morphed or rng.integers(2)):
                p = int(rng.choice(skinned))
                mat = self.matrices(p); mat[0, 3] = np.inf
                op = ("skin_mesh", p, mat)
            else:
                p = int(rng.choice(morphed))
                w = self.weights(p); w[-1] = np.nan
                op = ("morph_mesh", p, w)
        elif kind == "skin_on_primitive":
            prims = [k for k in range(m.n_objects) if m.kinds[k] in (N.OBJECT_SPHERE, N.OBJECT_PLANE)] + [k for k in m.lights if m.kinds[k] == N.OBJECT_MESH]
            p = int(rng.choice(prims))
            src = LAMP if (p in m.binds) else o
            j, w, n_joints, _ = skin_cases.make_case("bend", m.binds[src], seed=1)
            op = ("set_skin", p, m.binds[src], j, w, n_joints)
        elif kind == "refit_count":
            op = ("refit_mesh", o, self.deformed(o)[:-1] if m.n_tris[o] > 1 else np.concatenate([m.binds[o], m.binds[o]]))
        elif kind == "rebuild_without_tree":
            cands = [k for k in range(m.n_objects) if m.kinds[k] != N.OBJECT_MESH]
            op = ("rebuild_mesh", int(rng.choice(cands)), int(rng.choice(OPTIONS)))
        elif kind == "named_twice" and (skinned or morphed):
            p = int(rng.choice(skinned or morphed))
            op = ("pose_objects", [self.entry(p), self.entry(p)])
        elif kind in ("destroyed_clip", "clip_joint_count"):
            if not rigged:
                return self.emit(("refit_mesh", o, np.concatenate([m.binds[o], m.binds[o][:1]])))
            p = int(rng.choice(rigged))
            n = m.skins[p]["n_joints"]
            if kind == "destroyed_clip":
                slot = self.clip_for(n)
                if slot is not None:
                    self.emit(("destroy_clip", slot))
                else:                                                          # its clip is gone already: any destroyed clip will do
                    slot = next(k for k, c in m.clips.items() if c is None)
            else:
                slot = next((s for s, c in m.clips.items() if c is not None and c[0] != n), None)
                if slot is None:
                    slot = self.next_slot
                    self.next_slot += 1
                    self.emit(("create_clip", slot) + tuple(anim_cases.rig(n + 1, 3, "chain")[1]))
            op = ("animate_objects", [(p, slot, 0.3, None)])
        elif kind == "skeleton_without_skin" and (plain or morphed):
            p = int(rng.choice([q for q in self.posable if q not in m.skins]))
            op = ("set_skeleton", p) + tuple(anim_cases.rig(2, 1, "chain")[0])
        else:                                                                  # the state for that kind is not there yet: the refit is always possible
            op = ("refit_mesh", o, np.concatenate([m.binds[o], m.binds[o][:1]]))
        return self.emit(op)

    # -- the crowd: batches of many entries ------------------------------------------------------------------------------------------------
    def crowd_step(self):
        m, rng = self.model, self.rng
        half = (len(m.mesh_objects()) + 1) // 2
        reach = self.touched | {m.group[o] for o in self.with_state()}
        left = self.n_steps - len(self.ops)
        fresh = [o for o in self.posable if m.group[o] not in reach]
        need = half - len(reach)
        if left <= 1 or (need <= 0 and left <= 2 and any(m.group[o] not in self.touched for o in self.with_state())):
            have = self.with_state()
            return self.emit(("pose_objects", [self.entry(o) for o in have]), edits=have)
        if fresh and need > 0 and (need >= left - 2 or rng.random() < 0.7):
            o = int(rng.choice(fresh))
            r = rng.random()
            if r < 0.55:
                return self.emit(self.skin_op(o, name=str(rng.choice(["bend", "half", "rigid", "four"]))))
            if r < 0.8:
                return self.emit(self.morph_op(o))
            return self.emit(("refit_mesh", o, self.deformed(o)), edits=(o,))
        r = rng.random()
        have = self.with_state()
        if r < 0.35 and len(have) >= 2:
            some = [o for o in have if rng.random() < 0.8] or have
            return self.emit(("pose_objects", [self.entry(o, partial=True) for o in some]), edits=some)
        if r < 0.5 and len(have) >= 3 and self.refusals < self.n_steps // 4 - 1:
            return self.m_refused_then_accepted_batch()
        if r < 0.65 and have:
            skinned = [o for o in have if o in m.skins and m.skins[o]["n_joints"] == 2]
            if len(skinned) >= 2:
                slot = None
                for o in skinned[:3]:
                    slot = self.ensure_rigged(o)
                t0 = float(rng.uniform(0.0, 0.5))
                rigged = [o for o in skinned if m.skins[o]["skeleton"] is not None]
                return self.emit(("animate_objects", [(o, slot, t0 + 0.1 * k, None) for k, o in enumerate(rigged)]), edits=rigged)
        if r < 0.8:
            o = self.pick(self.rebuildable)
            return self.emit(("rebuild_mesh", o, int(rng.choice([P.BUILD_NAIVE, P.BUILD_SAH_BINNED]))), edits=(o,))
        if r < 0.88:
            return self.m_transforms_pose() if have else None
        return self.m_single()

    def reach_half(self):
        """towards the end, one-step edits of meshes no step has edited yet, so that half of the meshes differ from the upload"""
        m = self.model
        meshes = m.mesh_objects()
        need = (len(meshes) + 1) // 2 - sum(1 for k in meshes if m.group[k] in self.touched)
        fresh = [k for k in self.rebuildable + [k for k in m.lights if m.kinds[k] == N.OBJECT_MESH] if m.group[k] not in self.touched]
        if need <= 0 or not fresh or self.n_steps - len(self.ops) > need + 1:
            return False
        o = self.pick(fresh)
        if m.n_tris[o] >= 255 and o not in m.lights and self.rng.integers(2):
            self.emit(("rebuild_mesh", o, P.BUILD_NAIVE), edits=(o,))          # the uploaded trees are SAH trees
        else:
            self.emit(("refit_mesh", o, self.deformed(o)), edits=(o,))
        return True

    def run(self):
        motifs = [self.m_rebuild_morph, self.m_rebuild_skin, self.m_rebuild_refit_rebuild, self.m_set_morph_skin, self.m_clear_morph_skin, self.m_refit_skin,
                  self.m_replace_skin_morph, self.m_clear_skin_morph, self.m_animate_then_weights, self.m_animate_skin, self.m_upload_animate,
                  self.m_transforms_pose, self.m_refused_then_accepted_batch, self.m_batch]
        budget = self.budget
        try:
            guard = 0
            while guard < 50 * self.n_steps:
                guard += 1
                if self.kind == "crowd":
                    self.crowd_step()
                elif not self.reach_half():
                    m = self.draw("motifs", motifs, self.seed // 10)
                    if m == self.m_refused_then_accepted_batch and self.refusals >= budget:
                        continue
                    m()
                    if not self.reach_half():
                        self.m_single()
                if self.refusals < budget and self.rng.random() < 0.3:
                    self.refused()
        except _Done:
            pass
        assert len(self.ops) == self.n_steps, (len(self.ops), self.n_steps)
        self.model.close()
        return self.ops


def random_sequence(seed, n_steps, scene_kind, knobs=None):
    """n_steps operations, the same for the same arguments.  knobs: tuning the context has from the start (the generator only needs it to
    know which value a set_tuning would change)."""
    return _Generator(seed, n_steps, scene_kind, knobs).run()


# ---- the default set: what tests/test_gpu_edit_sequences.py runs and tests/test_edit_model.py checks ------------------------------------
STEPS = 16
SLOW_KNOBS = {"skin_joints_lds": 0, "morph_max_blocks": 1}
# chosen so that the conditions of tests/test_edit_model.py hold over the set (seeds 0 .. 279 of every row were searched)
DEFAULT_SEEDS = {("plain", "default"): (50, 83, 130, 269), ("plain", "knobs"): (112, 258), ("instanced", "default"): (182, 236), ("crowd", "default"): (110,),
                 ("plain", "group"): (178,)}


def default_set(extra_seeds=0, steps=STEPS):
    """[(scene kind, context, seed, steps)]: context is "default", "knobs" (SLOW_KNOBS from the start) or "group" (a two-member context).
    extra_seeds: that many more seeds per row, counted on from 1000."""
    out = []
    for (kind, context), seeds in DEFAULT_SEEDS.items():
        for seed in tuple(seeds) + tuple(range(1000, 1000 + extra_seeds)):
            out.append((kind, context, seed, steps))
    return out


def sequence_of(kind, context, seed, steps):
    return random_sequence(seed, steps, kind, knobs=SLOW_KNOBS if context == "knobs" else None)
