"""Following skinned poses in the temporal stage (CGPT_TEMPORAL_FOLLOW_POSES; csrc/device/denoise.hip: PreparePoses, pose_carry_back,
temporal_merge<.., POSE>) stated in numpy, on top of motion_ref.py and skin_ref.py.

A pose is always computed from the bind pose, so where a surface point was under an earlier pose is a function of that pose's joint
matrices alone.  A first hit on triangle tri of a re-posed object is carried back in six steps:
  1. P, the hit in object space: x, or Ainv x + binv with the float32 inverse the scene holds (transform_ref.invert);
  2. its coordinates on the current pose's triangle (p0, p1, p2): e1 = p1 - p0, e2 = p2 - p0, w = P - p0, g = e1 x e2,
     u = ((w x e2) . g) / (g . g), v = ((e1 x w) . g) / (g . g) -- smooth_ref.smooth_normal's steps 2-3, not clamped;
  3. the history pose's corners q_c and normals m_c: skin_ref.skin_f32, float32 line for line, under the history's matrices;
  4. x' = (q0 + u (q1 - q0)) + v (q2 - q0);
  5. n' = m0, or with the smooth flag ((1 - u - v) m0 + u m1) + v m2 over its length (m0 where the squared length is not > 1e-12);
  6. x_p = A x' + b, n_p = normalize(Ainv^T n') through the object's current transform; x', n' themselves without one.
Steps 1, 2, 4, 5 and 6 are float64 on the float32 inputs, every product ((a0 b0 + a1 b1) + a2 b2), and x_p, n_p are rounded to float32
once.  g . g zero or not finite, or a result that is not finite: the pixel takes no history (state 2).  motion_ref.carry_back (moved
objects) and temporal_ref.reproject then run on the carried-back guides; `dtype` runs that reprojection in another precision, as
motion_ref.reproject does (the tests ask how many pixels a float32 run decides differently).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import motion_ref as M
import skin_ref as SK
import temporal_ref as T
import transform_ref as TR

UNPOSED, REPOSED, DROP = 0, 1, 2


class Posed:
    """One skinned object as a frame sees it: the skin (bind (n, 18), joints and weights (n, 3, 4)), the joint matrices of its last pose
    (n_joints, 12) float32 or None ("no pose known"), the number of the installation (cgpt_scene_set_skin), the smooth flag and the
    object's current object-to-world matrix (None or the identity: no transform)."""

    def __init__(self, bind, joints, weights, matrices, serial=1, smooth=False, xform=None):
        self.bind = np.ascontiguousarray(bind, np.float32).reshape(-1, 18)
        self.joints, self.weights = np.asarray(joints), np.ascontiguousarray(weights, np.float32)
        self.matrices = None if matrices is None else np.ascontiguousarray(matrices, np.float32).reshape(-1, 12).copy()
        self.serial, self.smooth = serial, bool(smooth)
        self.xform = None if xform is None or TR.is_identity(xform) else np.ascontiguousarray(xform, np.float32).reshape(3, 4).copy()

    def key(self):
        """what the history remembers of the pose: None, or (installation, matrices)"""
        return None if self.matrices is None else (self.serial, self.matrices.shape[0], self.matrices.tobytes())

    def triangles(self, matrices=None) -> np.ndarray:
        """(n, 18) float32: the triangles cgpt_scene_skin_mesh writes under `matrices` (default: the current pose), bit for bit"""
        return SK.skin_f32(self.bind, self.joints, self.weights, self.matrices if matrices is None else matrices)


def pose_state(prev_key, cur_key) -> int:
    """An object's state from the history's key and the current one.  Equal keys (the same pose of the same skin, A -> B -> A, or no
    pose on either side): unposed.  Matrices that differ under one installation and joint count: re-posed.  Everything else -- no pose
    known on one side, another installation, another joint count -- drops."""
    if prev_key == cur_key:
        return UNPOSED
    if prev_key is None or cur_key is None or prev_key[:2] != cur_key[:2]:
        return DROP
    return REPOSED


def matrices_of(key) -> np.ndarray:
    return np.frombuffer(key[2], np.float32).reshape(-1, 12)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _affine(rows, x):
    """((r0 x + r1 y) + r2 z) + r3 per row of the (3, 4) float64 `rows`"""
    return np.stack([((rows[r, 0] * x[..., 0] + rows[r, 1] * x[..., 1]) + rows[r, 2] * x[..., 2]) + rows[r, 3] for r in range(3)], -1)


def barycentric(x, current, xform=None):
    """steps 1-2: (u, v, g . g) in float64 of the hits x (k, 3) float32 on the current triangles `current` (k, 18) float32"""
    P = x.astype(np.float64)
    if xform is not None:
        P = _affine(TR.invert(xform).astype(np.float64), P)
    c = current.astype(np.float64)
    p0, p1, p2 = c[:, 0:3], c[:, 6:9], c[:, 12:15]
    e1, e2, w = p1 - p0, p2 - p0, P - p0
    g = _cross(e1, e2)
    gg = _dot(g, g)
    with np.errstate(all="ignore"):
        return _dot(_cross(w, e2), g) / gg, _dot(_cross(e1, w), g) / gg, gg


def carry_hits(x, tau, posed: Posed, prev_matrices):
    """steps 1-6 for the hits x (k, 3) float32 on triangles tau (k,) of one re-posed object: (x_p (k, 3) float32, n_p (k, 3) float32,
    ok (k,) bool)"""
    tau = np.asarray(tau, np.int64)
    u, v, gg = barycentric(x, posed.triangles()[tau], posed.xform)
    h = posed.triangles(prev_matrices)[tau].astype(np.float64)                  # step 3, float32 bits widened
    q0, q1, q2, m0, m1, m2 = h[:, 0:3], h[:, 6:9], h[:, 12:15], h[:, 3:6], h[:, 9:12], h[:, 15:18]
    with np.errstate(all="ignore"):
        xp = (q0 + u[:, None] * (q1 - q0)) + v[:, None] * (q2 - q0)
        n = m0
        if posed.smooth:
            w0 = 1.0 - u - v
            s = (w0[:, None] * m0 + u[:, None] * m1) + v[:, None] * m2
            l2 = _dot(s, s)
            n = np.where((l2 > 1e-12)[:, None], s / np.sqrt(l2)[:, None], m0)
        if posed.xform is not None:
            inv = TR.invert(posed.xform).astype(np.float64)
            xp = _affine(posed.xform.astype(np.float64), xp)
            t = np.stack([(inv[0, j] * n[:, 0] + inv[1, j] * n[:, 1]) + inv[2, j] * n[:, 2] for j in range(3)], -1)
            n = t / np.sqrt(_dot(t, t))[:, None]
        x32, n32 = xp.astype(np.float32), n.astype(np.float32)
    ok = (gg != 0.0) & np.isfinite(gg) & np.all(np.isfinite(x32), -1) & np.all(np.isfinite(n32), -1)
    return x32, n32, ok


def carry_back(guides, tri, objects) -> np.ndarray:
    """The records of cgpt_read_previous_hits, (rows, width, 8) float32 {x_p.xyz, bits(state), n_p.xyz, 0}.  objects: object index ->
    (state, Posed, the history's matrices or None).  A miss, an object that is not named or unposed and a dropped pixel keep their own
    x and n."""
    g = np.asarray(guides, np.float32)
    out = np.zeros(g.shape[:2] + (8,), np.float32)
    out[..., 0:3], out[..., 4:7] = g[..., 0:3], g[..., 4:7]
    state = np.zeros(g.shape[:2], np.uint32)
    obj = np.ascontiguousarray(g[..., 7]).view(np.uint32)
    hit = D.hit_mask(g)
    for o, (st, posed, prev) in objects.items():
        on = hit & (obj == o)
        if st == DROP:
            state[on] = DROP
        elif st == REPOSED and on.any():
            x, n, ok = carry_hits(g[on][:, 0:3], np.asarray(tri)[on], posed, prev)
            rec = out[on]
            rec[ok, 0:3], rec[ok, 4:7] = x[ok], n[ok]
            out[on] = rec
            state[on] = np.where(ok, REPOSED, DROP)
    out.view(np.uint32)[..., 3] = state
    return out


def record_states(records):
    return np.ascontiguousarray(np.asarray(records, np.float32)[..., 3]).view(np.uint32)


def carried_guides(guides, records):
    """(the guides with x and n of the state-1 pixels replaced by their records, dropped (rows, width) bool)"""
    g = np.array(guides, np.float32)
    st = record_states(records)
    on = st == REPOSED
    g[on, 0:3], g[on, 4:7] = records[on, 0:3], records[on, 4:7]
    return g, st == DROP


def reproject(guides, records, hist, hist_guides, hist_camera, height, first_row, normal_cos_min=0.9, plane_tolerance=0.01, dtype=np.float64,
              motion_records=None):
    """temporal_ref.reproject on the guides carried back through their pose records and then, with motion_records, through
    motion_ref.carry_back (two roundings to float32); a dropped pixel has no history"""
    gc, dropped = carried_guides(guides, records)
    if motion_records is not None:
        gc, moved_drop = M.carry_back(gc, motion_records)
        dropped = dropped | moved_drop
    c_h, H, taps = T.reproject(gc, hist, hist_guides, hist_camera, height, first_row, normal_cos_min, plane_tolerance, dtype)
    return np.where(dropped[..., None], 0.0, c_h), np.where(dropped, 0.0, H), np.where(dropped, -1, taps)


class Temporal(M.Temporal):
    """M.Temporal whose frame() also takes the frame's triangle indices and skinned objects (object index -> Posed).  Without
    follow_poses any change of a pose key drops the history; with it the history is kept and the re-posed objects' hits are carried
    back, under equal camera bytes too.  When no key changed the frame is M.Temporal's.  (The statement knows a pose by its key: it
    covers the cases in which every change of a key comes with a cgpt_scene_skin_mesh call.)"""

    def reset(self):
        super().reset()
        self.poses = None
        self.records = None           # the last frame's carry-back records, or None when it had none

    def states(self, posed):
        keys = {o: p.key() for o, p in posed.items()}
        if self.history is None or self.poses is None:
            return keys, {}
        return keys, {o: pose_state(self.poses.get(o), k) for o, k in keys.items()}

    def frame(self, acc, num_accumulated, guides, camera, tri=None, posed=None, xform=None, follow=False, follow_poses=False, **kw):
        g = np.asarray(guides, np.float32)
        posed = posed or {}
        keys, states = self.states(posed)
        changed = any(s != UNPOSED for s in states.values())
        n_obj = 0 if xform is None else len(np.asarray(xform).reshape(-1, 12))
        cur = np.zeros((0, 12), np.float32) if xform is None else np.ascontiguousarray(xform, np.float32).reshape(n_obj, 12).copy()
        moved = self.history is not None and self.xform is not None and self.xform.tobytes() != cur.tobytes()
        if (changed and not follow_poses) or (moved and not follow):
            self.history = None
        self.records = None
        if self.history is None or not changed:
            out = super().frame(acc, num_accumulated, g, camera, xform=xform, follow=follow, **kw)
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
            objects = {o: (s, posed[o], matrices_of(self.poses[o]) if s == REPOSED else None) for o, s in states.items()}
            self.records = carry_back(g, tri, objects)
            c_h, H, _ = reproject(g, self.records, self.history, self.guides, self.camera, height, first_row, kw.get("normal_cos_min", 0.9),
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
