"""Following morph-target poses in the temporal stage (CGPT_TEMPORAL_FOLLOW_MORPHS; csrc/device/denoise.hip: PreparePoses,
morph_carry_back) stated in numpy, on top of pose_motion_ref.py, morph_ref.py and skin_ref.py.

A pose is always computed from the base, so where a surface point was under an earlier pose is a function of that pose's weights (and,
for an object that also has a skin, joint matrices) alone.  pose_motion_ref's six steps carry a first hit back unchanged; only step 3,
the history pose's corners, differs: skin_ref.skin_f32(morph_ref.morph_f32(base, deltas, w_prev), joints, skin weights, M_prev), or the
morph alone -- float32 line for line, the bits cgpt_scene_morph_mesh / cgpt_scene_skin_mesh wrote then.  carry_hits, carry_back and
reproject are pose_motion_ref's own functions: a Morphed object answers their triangles(prev) call.

The edits since the history fall into four classes -- transforms, skin poses, morphs, everything else -- and each flag keeps its own
class only (history_kept).  An object's state comes from its pose keys (pose_motion_ref.pose_state: equal 0, same installations and
counts 1, anything else 2) and from the call's flags (object_state)."""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import morph_ref as MR
import motion_ref as M
import pose_motion_ref as PM
import skin_ref as SK
import temporal_ref as T

UNPOSED, REPOSED, DROP = PM.UNPOSED, PM.REPOSED, PM.DROP


class Morphed(PM.Posed):
    """One object with morph targets as a frame sees it: the base (n, 18), the deltas (K, n, 18), the weights of its last pose (K,)
    float32 or None ("no pose known"), the number of the installation (cgpt_scene_set_morph_targets), and -- if a skin took part in
    that pose -- skin = (joints, skin weights, joint matrices, the skin's installation); the smooth flag and the object-to-world matrix
    as pose_motion_ref.Posed has them."""

    def __init__(self, base, deltas, weights, serial=1, smooth=False, xform=None, skin=None):
        base = np.ascontiguousarray(base, np.float32).reshape(-1, 18)
        n = base.shape[0]
        joints, skin_weights, matrices, self.skin_serial = skin if skin is not None else (np.zeros((n, 3, 4), np.uint16), np.zeros((n, 3, 4), np.float32), None, 0)
        super().__init__(base, joints, skin_weights, matrices, serial, smooth, xform)
        self.deltas = np.ascontiguousarray(deltas, np.float32).reshape(-1, n, 18)
        self.morph_weights = None if weights is None else np.ascontiguousarray(weights, np.float32).ravel().copy()
        assert self.morph_weights is None or self.morph_weights.size == self.deltas.shape[0]

    def key(self):
        """what the history remembers of the pose: None, or (installations, counts, weights, matrices) -- pose_motion_ref.pose_state
        compares the first two entries for state 2 and the whole for state 0"""
        if self.morph_weights is None:
            return None
        m = self.matrices
        return ((self.serial, self.skin_serial), (self.morph_weights.size, 0 if m is None else m.shape[0]), self.morph_weights.tobytes(),
                b"" if m is None else m.tobytes())

    def triangles(self, prev=None) -> np.ndarray:
        """(n, 18) float32: the triangles the device writes under prev = (weights, matrices or None) (default: the current pose)"""
        w, m = (self.morph_weights, self.matrices) if prev is None else prev
        rows = MR.morph_f32(self.bind, self.deltas, w)
        return rows if m is None else SK.skin_f32(rows, self.joints, self.weights, m)


def history_pose(key):
    """the `prev` of Morphed.triangles from a history key"""
    w = np.frombuffer(key[2], np.float32)
    return w, (np.frombuffer(key[3], np.float32).reshape(-1, 12) if key[3] else None)


def history_kept(transforms, poses, morphs, others, follow=False, follow_poses=False, follow_morphs=False) -> bool:
    """The four-class rule: the counts of cgpt_scene_update_transforms, cgpt_scene_skin_mesh, accepted cgpt_scene_morph_mesh and all
    other edits since the history was stored.  Each flag keeps its own class only; any other edit drops the history."""
    return others == 0 and (transforms == 0 or follow) and (poses == 0 or follow_poses) and (morphs == 0 or follow_morphs)


def object_state(prev_key, cur_key, posed_since=True, has_targets=True, follow_morphs=True) -> int:
    """An object's state at a call that kept its history.  Not posed since the history: 0 whatever the keys.  An object with targets
    reaches states 0 (equal keys) and 1 only with CGPT_TEMPORAL_FOLLOW_MORPHS in the call; one without targets keeps 5.27's rules."""
    if not posed_since:
        return UNPOSED
    if has_targets and not follow_morphs:
        return DROP
    return PM.pose_state(prev_key, cur_key)


def edit_classes(prev_key, cur_key):
    """(a skin pose happened, a morph happened) for one object, as the statement knows them: by the keys (it covers the cases in
    which every change of a key comes with the call that makes it)"""
    if prev_key == cur_key or prev_key is None or cur_key is None:
        return False, False
    if len(cur_key) == 3:                                                      # pose_motion_ref.Posed: (installation, joints, matrices)
        return True, False
    return prev_key[3] != cur_key[3], prev_key[2] != cur_key[2]


class Temporal(PM.Temporal):
    """pose_motion_ref.Temporal whose frame() takes follow_morphs and Morphed objects among `posed`.  A changed weight without
    follow_morphs, or changed matrices without follow_poses, drops the history; with the flags the re-posed objects' hits are carried
    back.  When no key changed the frame is motion_ref.Temporal's."""

    def frame(self, acc, num_accumulated, guides, camera, tri=None, posed=None, xform=None, follow=False, follow_poses=False, follow_morphs=False, **kw):
        g = np.asarray(guides, np.float32)
        posed = posed or {}
        keys, states = self.states(posed)
        for o, s in list(states.items()):
            if isinstance(posed[o], Morphed):
                states[o] = object_state(self.poses.get(o), keys[o], s != UNPOSED, True, follow_morphs)
        changed = any(s != UNPOSED for s in states.values())
        edits = [edit_classes(self.poses.get(o), k) for o, k in keys.items()] if self.poses is not None and self.history is not None else []
        n_obj = 0 if xform is None else len(np.asarray(xform).reshape(-1, 12))
        cur = np.zeros((0, 12), np.float32) if xform is None else np.ascontiguousarray(xform, np.float32).reshape(n_obj, 12).copy()
        moved = self.history is not None and self.xform is not None and self.xform.tobytes() != cur.tobytes()
        if not history_kept(int(moved), sum(e[0] for e in edits), sum(e[1] for e in edits), 0, follow, follow_poses, follow_morphs):
            self.history = None
        self.records = None
        if self.history is None or not changed:
            out = M.Temporal.frame(self, acc, num_accumulated, g, camera, xform=xform, follow=follow, **kw)
            self.poses = keys
            return out
        rows, width = g.shape[:2]
        height = kw.get("height") or rows
        first_row = kw.get("first_row", 0)
        demodulate = kw.get("demodulate", True)
        key = (width, height, first_row, rows, kw.get("generation", 0), bool(demodulate))
        m = D.demodulation(g, kw.get("light_materials", ())) if demodulate else np.ones((rows, width, 3))
        c0 = D.radiance(acc, num_accumulated).astype(np.float64) / m
        c_h, H = np.zeros((rows, width, 3)), np.zeros((rows, width))
        if self.key == key:
            objects = {}
            for o, s in states.items():
                prev = None
                if s == REPOSED:
                    prev = history_pose(self.poses[o]) if isinstance(posed[o], Morphed) else PM.matrices_of(self.poses[o])
                objects[o] = (s, posed[o], prev)
            self.records = PM.carry_back(g, tri, objects)
            c_h, H, _ = PM.reproject(g, self.records, self.history, self.guides, self.camera, height, first_row, kw.get("normal_cos_min", 0.9),
                                     kw.get("plane_tolerance", 0.01), motion_records=M.motion_records(self.xform, cur) if moved else None)
            if not kw.get("keep_view_dependent", False):
                hit = D.hit_mask(g)
                mat = np.ascontiguousarray(g[..., 11]).view(np.uint32)
                vd = np.zeros((rows, width), bool)
                vd[hit] = np.asarray(kw.get("view_dependent_materials", ()), bool)[mat[hit]]
                H = np.where(vd, 0.0, H)
        c, Hn = T.merge(c0, num_accumulated, c_h, H, kw.get("max_history", 64.0))
        self.history = np.concatenate([c, Hn[..., None]], -1)
        self.guides, self.camera, self.key, self.xform, self.poses = g.copy(), T.camera_array(camera), key, cur, keys
        it = kw.get("iterations", 5)
        r = c * m if it == 0 else D.atrous(c, g, it, kw.get("sigma_color", 4.0), kw.get("sigma_normal", 0.2), kw.get("sigma_position", 0.3)) * m
        rgba = np.concatenate([r, np.ones((rows, width, 1))], -1)
        return rgba, D.pack_pixels(r)
