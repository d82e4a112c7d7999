"""Following object transforms in the temporal stage (CGPT_TEMPORAL_FOLLOW_TRANSFORMS; csrc/device/transform_math.h: MakeMotionRecord,
csrc/device/denoise.hip: temporal_merge<.., MOTION>) stated in numpy, on top of temporal_ref.py.

An object whose 12 matrix floats differ bytewise from those in force when the history was stored is moved: its first hits are carried
back, x' = D x with D = M_prev M_cur^-1 and n' = normalize(N n) with N = A_prev^-T A_cur^T, and temporal_ref.reproject runs on the
carried-back guides.  D and N are formed in double from the float entries (the adjugate / determinant inverses of InvertTransform, every
product ((p0 q0 + p1 q1) + p2 q2)) and each entry is rounded to float32 once; x' and n' are evaluated in double and rounded once.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import temporal_ref as T

UNMOVED, MOVED, DROP = 0, 1, 2


def _inverse(m):
    """the double inverse of the linear part of a (3, 4) float32 matrix (InvertTransform's cofactors, not rounded); None: singular"""
    a = m.astype(np.float64)
    c00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
    c01 = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
    c02 = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
    with np.errstate(all="ignore"):
        det = (a[0, 0] * c00 + a[0, 1] * c01) + a[0, 2] * c02
        if det == 0.0 or not np.isfinite(det):
            return None
        return np.array([
            [c00 / det, (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) / det, (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) / det],
            [c01 / det, (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) / det, (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) / det],
            [c02 / det, (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) / det, (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) / det]])


def motion_record(prev12, cur12) -> np.ndarray:
    """The 24 words (uint32 view of 6 float4) of one object's record: rows 0..2 {D row, translation}, rows 3..5 {N row, 0}, the state
    word in place of row 3's last float.  Unmoved and drop records have zero rows."""
    prev = np.ascontiguousarray(prev12, np.float32).reshape(3, 4)
    cur = np.ascontiguousarray(cur12, np.float32).reshape(3, 4)
    rec = np.zeros((6, 4), np.float32)
    words = rec.view(np.uint32)

    def with_state(state):
        words[3, 3] = state
        return words.reshape(24).copy()

    if prev.tobytes() == cur.tobytes():
        return with_state(UNMOVED)
    with np.errstate(all="ignore"):
        ic, ip = _inverse(cur), _inverse(prev)
        if ic is None or ip is None:
            return with_state(DROP)
        p, c = prev.astype(np.float64), cur.astype(np.float64)
        binv = [-((ic[i, 0] * c[0, 3] + ic[i, 1] * c[1, 3]) + ic[i, 2] * c[2, 3]) for i in range(3)]
        out = np.zeros((6, 4), np.float64)
        for r in range(3):
            for k in range(3):
                out[r, k] = (p[r, 0] * ic[0, k] + p[r, 1] * ic[1, k]) + p[r, 2] * ic[2, k]
                out[3 + r, k] = (ip[0, r] * c[k, 0] + ip[1, r] * c[k, 1]) + ip[2, r] * c[k, 2]
            out[r, 3] = ((p[r, 0] * binv[0] + p[r, 1] * binv[1]) + p[r, 2] * binv[2]) + p[r, 3]
        out32 = out.astype(np.float32)
    if not np.all(np.isfinite(out32)):
        return with_state(DROP)
    rec[:] = out32
    return with_state(MOVED)


def motion_records(prev, cur) -> np.ndarray:
    """(n, 24) uint32: the record of every object; matrices (n, 3, 4) or (n, 12) float32"""
    prev = np.ascontiguousarray(prev, np.float32).reshape(-1, 12)
    cur = np.ascontiguousarray(cur, np.float32).reshape(-1, 12)
    assert prev.shape == cur.shape
    return np.stack([motion_record(p, c) for p, c in zip(prev, cur)]) if len(cur) else np.zeros((0, 24), np.uint32)


def record_states(records):
    return np.asarray(records, np.uint32).reshape(-1, 24)[:, 15]


def carry_back(guides, records, normals=True):
    """(float32 guides with x and n of the pixels on moved objects carried back, dropped (rows, width) bool: a hit on a drop object).
    Pixels on unmoved objects and misses keep their bits.  normals=False leaves n alone (what an implementation without N would do)."""
    g = np.array(guides, np.float32)
    rec = np.asarray(records, np.uint32).reshape(-1, 24)
    rows = rec.view(np.float32).reshape(-1, 6, 4).astype(np.float64)
    state = rec[:, 15]
    obj = np.ascontiguousarray(g[..., 7]).view(np.uint32)
    hit = D.hit_mask(g)
    o = np.where(hit, obj, 0).astype(np.int64)
    st = np.where(hit, state[o], UNMOVED) if len(state) else np.zeros(obj.shape, np.uint32)
    moved = st == MOVED
    if moved.any():
        R = rows[o[moved]]
        x, n = g[moved][:, 0:3].astype(np.float64), g[moved][:, 4:7].astype(np.float64)
        xc = np.stack([((R[:, r, 0] * x[:, 0] + R[:, r, 1] * x[:, 1]) + R[:, r, 2] * x[:, 2]) + R[:, r, 3] for r in range(3)], -1)
        v = np.stack([(R[:, 3 + r, 0] * n[:, 0] + R[:, 3 + r, 1] * n[:, 1]) + R[:, 3 + r, 2] * n[:, 2] for r in range(3)], -1)
        with np.errstate(all="ignore"):
            length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            nc = v / length[:, None]
        new = g[moved]
        new[:, 0:3] = xc.astype(np.float32)
        if normals:
            new[:, 4:7] = nc.astype(np.float32)
        g[moved] = new
    return g, st == DROP


def reproject(guides, records, hist, hist_guides, hist_camera, height, first_row, normal_cos_min=0.9, plane_tolerance=0.01, dtype=np.float64):
    """temporal_ref.reproject on the carried-back guides; a pixel on a drop object has no history"""
    gc, dropped = carry_back(guides, records)
    c_h, H, taps = T.reproject(gc, hist, hist_guides, hist_camera, height, first_row, normal_cos_min, plane_tolerance, dtype)
    return np.where(dropped[..., None], 0.0, c_h), np.where(dropped, 0.0, H), np.where(dropped, -1, taps)


class Temporal(T.Temporal):
    """T.Temporal whose frame() takes the current matrices.  follow=False is cgpt_denoise_temporal without the flag: any change of
    the matrices drops the history.  follow=True keeps it and reprojects the carried-back guides, under equal camera bytes too when
    an object moved; when none moved the frame is T.Temporal's."""

    def reset(self):
        super().reset()
        self.xform = None

    def frame(self, acc, num_accumulated, guides, camera, xform=None, follow=False, **kw):
        g = np.asarray(guides, np.float32)
        n_obj = 0 if xform is None else len(np.asarray(xform).reshape(-1, 12))
        cur = np.zeros((0, 12), np.float32) if xform is None else np.ascontiguousarray(xform, np.float32).reshape(n_obj, 12).copy()
        changed = self.history is not None and self.xform is not None and self.xform.tobytes() != cur.tobytes()
        if changed and not follow:
            self.history = None
        moved = changed and follow
        if not moved:
            out = super().frame(acc, num_accumulated, g, camera, **kw)
            self.xform = cur
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
            records = motion_records(self.xform, cur)
            c_h, H, _ = reproject(g, records, self.history, self.guides, self.camera, height, first_row, kw.get("normal_cos_min", 0.9),
                                  kw.get("plane_tolerance", 0.01))
            if not kw.get("keep_view_dependent", False):
                hit = D.hit_mask(g)
                mat = np.ascontiguousarray(g[..., 11]).view(np.uint32)
                vd = np.zeros((rows, width), bool)
                vd[hit] = np.asarray(kw.get("view_dependent_materials", ()), bool)[mat[hit]]
                H = np.where(vd, 0.0, H)
        c, Hn = T.merge(c0, num_accumulated, c_h, H, kw.get("max_history", 64.0))
        self.history = np.concatenate([c, Hn[..., None]], -1)
        self.guides, self.camera, self.key, self.xform = g.copy(), T.camera_array(camera), key, cur
        it = kw.get("iterations", 5)
        r = c * m if it == 0 else D.atrous(c, g, it, kw.get("sigma_color", 4.0), kw.get("sigma_normal", 0.2), kw.get("sigma_position", 0.3)) * m
        rgba = np.concatenate([r, np.ones((rows, width, 1))], -1)
        return rgba, D.pack_pixels(r)
