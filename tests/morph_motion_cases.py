"""The scene, the morph targets and the pose changes shared by the morph-following tests (test_morph_motion_reference.py on the CPU,
test_gpu_morph_motion.py on the device): pose_motion_cases.py's ten-object scene at its 97x61 and its cameras, with the mover under the
identity so that one morphed mesh has no transform.

  MOVER   the faceted level-2 icosphere (320 triangles): targets alone, no transform;
  SMOOTH  the smooth-flagged icosphere: targets alone, under its transform;
  INST_A  the instanced icosphere (80 triangles): targets and the skin "bend", fused; a pose moves INST_B, the second placement, too;
  TRI     the one-triangle object: targets alone;
  STATIC  the transformed box: the skin "bend" and no targets -- it follows 5.27's rules in the same pass.
A target displaces every corner by a smooth function of its base position (a sine along a direction of its own, position and normal
deltas alike), so corners that share a position move together and the surface stays connected.  A case names the weights and joint
matrices the history is stored under and those of the frame after it; a case without a camera move gets motion_cases.JITTER."""
from __future__ import annotations

import numpy as np

import morph_motion_ref as MM
import motion_cases as MC
import pose_motion_cases as PC
import pose_motion_ref as PM

W, H, FOV, BASE, CAP = PC.W, PC.H, PC.FOV, PC.BASE, PC.CAP
WALL, LAMP, BALL, STATIC, MOVER, INST_A, INST_B, GLASS, SMOOTH, TRI = range(10)
N_OBJECTS = PC.N_OBJECTS
MORPHED = (MOVER, INST_A, SMOOTH, TRI)                                         # the objects that own targets
SKINNED = (STATIC, INST_A)                                                     # ... a skin
OWNER = {STATIC: STATIC, MOVER: MOVER, INST_A: INST_A, INST_B: INST_A, SMOOTH: SMOOTH, TRI: TRI}
FOLLOWED = tuple(OWNER)                                                        # the objects a pose can move
SMALL = (INST_A, TRI)                                                          # `limit` puts its 256 targets on these


def base_matrices():
    m = PC.base_matrices()
    m[MOVER] = np.eye(3, 4, dtype=np.float32)
    return m


def product_scene(mats=None, instances=True):
    return PC.product_scene(base_matrices() if mats is None else mats, instances)


def base_triangles():
    """object index -> (n, 18) float32 base (and bind) triangles of every object that owns targets or a skin"""
    return PC.bind_triangles()


def smooth_deltas(base, n_targets, seed, pos=0.15, nrm=0.1):
    """(n_targets, n, 18) float32: target k moves a corner at p by pos sin(f_k . p + phase_k) u_k and its normal by nrm cos(..) v_k"""
    rng = np.random.default_rng(1000 + seed)
    p = base.reshape(-1, 3, 6)[..., :3].astype(np.float64)
    size = float(np.max(np.abs(p))) or 1.0
    d = np.zeros((n_targets,) + p.shape[:2] + (6,))
    for k in range(n_targets):
        u, v, f = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
        arg = p @ (f / np.linalg.norm(f) * 2.0 / size) + rng.uniform(0, 2 * np.pi)
        d[k, ..., :3] = pos * np.sin(arg)[..., None] * (u / np.linalg.norm(u))
        d[k, ..., 3:] = nrm * np.cos(arg)[..., None] * (v / np.linalg.norm(v))
    return d.reshape(n_targets, -1, 18).astype(np.float32)


def _w(k, pairs):
    w = np.zeros(k, np.float32)
    for i, v in pairs:
        w[i] = v
    return w


def _limit(sign):
    rng = np.random.default_rng(77)
    w = rng.uniform(0.005, 0.03, 256) * np.where(rng.random(256) < 0.5, -1.0, 1.0)
    return (w * (1.0 if sign > 0 else -0.6)).astype(np.float32)


# name -> (targets per object, history weights, current weights, (degrees, shift) the skins' matrices change by or None, the view after)
CASES = {
    "nudge": (1, lambda k: _w(k, [(0, 0.3)]), lambda k: _w(k, [(0, 0.5)]), None, MC.JITTER),                      # 0.03 world units: an eighth of a pixel
    "mix": (8, lambda k: _w(k, [(0, 0.4), (3, -0.3), (5, 0.6)]), lambda k: _w(k, [(0, 0.5), (2, 0.25), (3, -0.45), (7, 0.35)]), None, MC.CAMERA_MOVE),
    "fused": (3, lambda k: _w(k, [(0, 0.4), (2, -0.2)]), lambda k: _w(k, [(0, 0.6), (1, 0.3)]), (1.5, (0.05, 0.03, 0.0)), MC.JITTER),
    "skin_only_on_morphed": (3, lambda k: _w(k, [(0, 0.4), (2, -0.2)]), lambda k: _w(k, [(0, 0.4), (2, -0.2)]), (2.0, (0.1, -0.05, 0.04)), MC.JITTER),
    "limit": (1, lambda k: _limit(1) if k == 256 else _w(k, [(0, 0.3)]), lambda k: _limit(-1) if k == 256 else _w(k, [(0, 0.45)]), None, MC.JITTER),
    "from_base": (2, lambda k: _w(k, []), lambda k: _w(k, [(0, 0.3), (1, -0.2)]), None, MC.JITTER),                 # the history's corners are the base
    "a_b_a": (1, lambda k: _w(k, [(0, 0.3)]), lambda k: _w(k, [(0, 0.3)]), None, MC.JITTER),                      # B = nudge's weights, in between
}


class Case:
    """the targets, skins and the two poses of one of CASES"""

    def __init__(self, name):
        k_all, w_hist, w_cur, skin_change, self.view = CASES[name]
        self.name = name
        self.base = base_triangles()
        self.n_targets = {o: (256 if name == "limit" and o in SMALL else k_all) for o in MORPHED}
        self.deltas = {o: smooth_deltas(self.base[o], self.n_targets[o], o) for o in MORPHED}
        self.w_hist = {o: w_hist(self.n_targets[o]) for o in MORPHED}
        self.w_cur = {o: w_cur(self.n_targets[o]) for o in MORPHED}
        self.w_between = {o: _w(self.n_targets[o], [(0, 0.5)]) for o in MORPHED}   # a_b_a's B
        sk = PC.skins()
        self.skins = {o: sk[o] for o in SKINNED}                               # (bind, joints, weights, n_joints, base matrices)
        self.m_hist = {o: self.skins[o][4] for o in SKINNED}
        self.m_cur = dict(self.m_hist)
        if skin_change is not None:
            deg, shift = skin_change
            self.m_cur = {o: PC.varied(self.skins[o][4], self.skins[o][0], deg, shift, 1.0 if k % 2 == 0 else -1.0) for k, o in enumerate(SKINNED)}
        weights_change = any(self.w_hist[o].tobytes() != self.w_cur[o].tobytes() for o in MORPHED)
        # the objects in state 1 after the change: the fused pair follows either edit, a morph-only object the weights, the skin-only box the matrices
        self.reposed = tuple(o for o in FOLLOWED if (weights_change and OWNER[o] in MORPHED) or (skin_change is not None and OWNER[o] in SKINNED))

    def poses(self, which):
        return (self.w_hist, self.m_hist) if which == "hist" else (self.w_between, self.m_hist) if which == "between" else (self.w_cur, self.m_cur)

    def triangles(self, o, which):
        """(n, 18) float32: what the device writes for owner o under the pose `which` ("hist", "between" or "cur")"""
        return self.objects(which)[o].triangles()

    def objects(self, which, mats=None, serial=1):
        """object index -> morph_motion_ref.Morphed (or pose_motion_ref.Posed for the skin-only box) under the pose `which`"""
        mats = base_matrices() if mats is None else mats
        w, m = self.poses(which)
        out = {}
        for o in FOLLOWED:
            k = OWNER[o]
            if k in MORPHED:
                skin = (self.skins[k][1], self.skins[k][2], m[k], 1) if k in SKINNED else None
                out[o] = MM.Morphed(self.base[k], self.deltas[k], w[k], serial, o == SMOOTH, mats[o], skin)
            else:
                out[o] = PM.Posed(self.skins[k][0], self.skins[k][1], self.skins[k][2], m[k], serial, False, mats[o])
        return out

    def history_of(self, o):
        """the `prev` pose_motion_ref.carry_back takes for object o: the history's (weights, matrices), or its matrices alone"""
        k = OWNER[o]
        return (self.w_hist[k], self.m_hist[k] if k in SKINNED else None) if k in MORPHED else self.m_hist[k]

    def extent(self, o, mats=None):
        """the largest world coordinate of object o's corners under the history's pose, for the tolerance on x_p"""
        mats = base_matrices() if mats is None else mats
        p = self.triangles(o, "hist").reshape(-1, 6)[:, :3].astype(np.float64)
        return float(np.max(np.abs(p @ mats[o][:, :3].astype(np.float64).T + mats[o][:, 3].astype(np.float64))))


def camera(s, view):
    return PC.camera(s, view)


def host_guides(cam, case, which, mats=None):
    """pose_motion_cases.host_guides of the scene with every followed object at the pose `which`.  That function poses its objects by
    skin_f32; it is given the posed triangles as the bind pose of a one-joint identity skin, which returns the positions unchanged
    (the normals within a rounding: these guides are the CPU tests' scene, not a yardstick)."""
    mats = base_matrices() if mats is None else mats
    one = np.eye(3, 4, dtype=np.float32).reshape(1, 12)
    sk, matrices = {}, {}
    for o in PC.SKINNED:                                                       # the owners pose_motion_cases knows: the same five
        rows = case.triangles(o, which)
        j, w = np.zeros((len(rows), 3, 4), np.uint16), np.zeros((len(rows), 3, 4), np.float32)
        w[..., 0] = 1.0
        sk[o], matrices[o] = (rows, j, w, 1, one), one
    return PC.host_guides(cam, sk, matrices, mats)
