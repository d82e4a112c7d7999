"""The temporal stage of cgpt_denoise_temporal (csrc/device/denoise.hip) stated in numpy float64, for the tests.

The history is a merged colour c and a history length H (in samples) per pixel, with the guides, the camera, the frame key, the scene
generation and the demodulate bit of the frame it was stored for.  A call resolves c_0 = acc / N / m as cgpt_denoise does, finds each
pixel's history (c_h, H) -- none, the pixel's own (same camera bytes), or four validated bilinear taps around its reprojection onto the
history's camera -- and merges c = (He c_h + N c_0) / (He + N), He = min(H, max_history), H' = min(He + N, max_history); a pixel without
history keeps c = c_0 bit for bit.  The a-trous passes of denoise_ref then run on c.

`dtype` runs the geometry of the reprojection in another precision (the tests ask how many pixels a float32 run decides differently).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D

W_MIN = 0.01                      # valid bilinear weights summing to this or less: no history


def camera_array(cam) -> np.ndarray:
    """the 12 floats {pos, top_left, top_right, bottom_left} of a cgpt_camera (a ctypes struct or anything array-like)"""
    if hasattr(cam, "pos"):
        return np.float32(list(cam.pos) + list(cam.top_left) + list(cam.top_right) + list(cam.bottom_left))
    return np.asarray(cam, np.float32).reshape(12)


def camera_minv(cam):
    """Minv of a camera: the inverse (adjugate / determinant, in double from the float entries) of the matrix with the columns
    top_left - pos, top_right - top_left, bottom_left - top_left, each entry rounded to float32 once; None for a singular camera"""
    c = camera_array(cam).astype(np.float64)
    pos, tl, tr, bl = c[0:3], c[3:6], c[6:9], c[9:12]
    m = np.stack([tl - pos, tr - tl, bl - tl], axis=1)
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = (m[0, 0] * c00 + m[0, 1] * c01) + m[0, 2] * c02
    if det == 0.0 or not np.isfinite(det):
        return None
    inv = np.array([
        [c00, m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
        [c01, m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
        [c02, m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]]) / det
    with np.errstate(over="ignore"):
        out = inv.astype(np.float32)
    return out if np.all(np.isfinite(out)) else None


def previous_position(guides, hist_camera, height, first_row, dtype=np.float64):
    """(fx, fy, front) of every pixel of the band: where its first hit lies in the history's band (in pixels; the integer coordinates are
    that frame's sample points), and whether it is a hit in front of the history's camera.  None for a singular camera."""
    T = dtype
    g = np.asarray(guides, np.float32)
    rows, width = g.shape[:2]
    minv = camera_minv(hist_camera)
    if minv is None:
        return None
    M = minv.astype(T)
    pos_prev = camera_array(hist_camera)[0:3].astype(T)
    d = g[..., 0:3].astype(T) - pos_prev
    a, b, c = ((M[r, 0] * d[..., 0] + M[r, 1] * d[..., 1]) + M[r, 2] * d[..., 2] for r in range(3))
    front = D.hit_mask(g) & (a > 0)                                           # a <= 0: behind the history's camera
    a_s = np.where(front, a, T(1))
    fx = np.where(front, (b / a_s) * T(width), T(0))
    fy = np.where(front, (c / a_s) * T(height) - T(first_row), T(0))
    fx = np.clip(fx, T(-2), T(width + 1))                                     # two pixels outside the band every tap is outside it
    fy = np.clip(fy, T(-2), T(rows + 1))
    return fx, fy, front


def reproject(guides, hist, hist_guides, hist_camera, height, first_row, normal_cos_min=0.9, plane_tolerance=0.01, dtype=np.float64):
    """The history of every pixel of the band `guides` (rows, width, 12) under a changed camera: (c_h (rows, width, 3), H (rows, width),
    taps (rows, width) int64).  H = 0: no history.  taps names the accepted tap set -- the top-left tap's position and the four
    validity bits -- and is -1 without history.  hist (rows, width, 4) = {c, H} and hist_guides (rows, width, 12) are the history's."""
    T = dtype
    g = np.asarray(guides, np.float32)
    gp = np.asarray(hist_guides, np.float32)
    rows, width = g.shape[:2]
    where = previous_position(g, hist_camera, height, first_row, T)
    if where is None:
        return np.zeros((rows, width, 3)), np.zeros((rows, width)), np.full((rows, width), -1, np.int64)
    fx, fy, front = where
    x, t, n = g[..., 0:3].astype(T), g[..., 3].astype(T), g[..., 4:7].astype(T)
    obj = np.ascontiguousarray(g[..., 7]).view(np.uint32)
    obj_prev = np.ascontiguousarray(gp[..., 7]).view(np.uint32)
    x_prev, n_prev = gp[..., 0:3].astype(T), gp[..., 4:7].astype(T)
    h = np.asarray(hist, np.float64)
    flx, fly = np.floor(fx), np.floor(fy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    wx, wy = fx - flx, fy - fly
    tol = T(np.float32(plane_tolerance)) * t
    cos_min = T(np.float32(normal_cos_min))
    wsum = np.zeros((rows, width), T)
    sc = np.zeros((rows, width, 3))
    sh = np.zeros((rows, width))
    bits = np.zeros((rows, width), np.int64)
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        inb = (qx >= 0) & (qx < width) & (qy >= 0) & (qy < rows)
        qxc, qyc = np.clip(qx, 0, width - 1), np.clip(qy, 0, rows - 1)
        np_k, xp_k = n_prev[qyc, qxc], x_prev[qyc, qxc]
        ndot = (np_k[..., 0] * n[..., 0] + np_k[..., 1] * n[..., 1]) + np_k[..., 2] * n[..., 2]
        dp = xp_k - x
        dplane = (n[..., 0] * dp[..., 0] + n[..., 1] * dp[..., 1]) + n[..., 2] * dp[..., 2]
        valid = inb & (obj_prev[qyc, qxc] == obj) & (ndot >= cos_min) & (np.abs(dplane) <= tol)
        w = np.where(valid, (wx if k & 1 else T(1) - wx) * (wy if k >> 1 else T(1) - wy), T(0))
        wsum = wsum + w
        sc += w[..., None].astype(np.float64) * h[qyc, qxc, :3]
        sh += w.astype(np.float64) * h[qyc, qxc, 3]
        bits |= valid.astype(np.int64) << k
    use = front & (wsum > T(W_MIN))
    den = np.where(use, wsum, 1).astype(np.float64)
    c_h = np.where(use[..., None], sc / den[..., None], 0.0)
    H = np.where(use, sh / den, 0.0)
    taps = np.where(use, ((y0 + 2) * (width + 4) + (x0 + 2)) * 16 + bits, -1)
    return c_h, H, taps


def merge(c0, n_samples, c_h, H, max_history=64.0):
    """(c, H') of the merge; H = 0 is no history: c = c_0 itself"""
    mh = float(np.float32(max_history))
    c0 = np.asarray(c0, np.float64)
    He = np.minimum(np.asarray(H, np.float64), mh)
    N = float(n_samples)
    c = np.where((He > 0)[..., None], (He[..., None] * c_h + N * c0) / (He + N)[..., None], c0)
    return c, np.minimum(He + N, mh)


class Temporal:
    """The state of a context: the history and what it was stored for.  frame() is one cgpt_denoise_temporal call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.history = None           # (rows, width, 4) float64 {c, H}

    def frame(self, acc, num_accumulated, guides, camera, height=None, first_row=0, generation=0, iterations=5, sigma_color=4.0,
              sigma_normal=0.2, sigma_position=0.3, demodulate=True, light_materials=(), view_dependent_materials=(), max_history=64.0,
              normal_cos_min=0.9, plane_tolerance=0.01, keep_view_dependent=False):
        """(rgba float64 (rows, width, 4), pixels uint32 (rows, width)); view_dependent_materials: specular > 0 or refractivity > 0 of
        every material index; generation: anything that changes with every scene edit"""
        g = np.asarray(guides, np.float32)
        rows, width = g.shape[:2]
        height = rows if height is None else height
        cam = camera_array(camera)
        key = (width, height, first_row, rows, generation, bool(demodulate))
        m = D.demodulation(g, light_materials) if demodulate else np.ones((rows, width, 3))
        c0 = D.radiance(acc, num_accumulated).astype(np.float64) / m
        c_h, H = np.zeros((rows, width, 3)), np.zeros((rows, width))
        if self.history is not None and self.key == key:
            if self.camera.tobytes() == cam.tobytes():                         # the same scene and camera: the same hit
                c_h, H = self.history[..., :3], self.history[..., 3]
            else:
                c_h, H, _ = reproject(g, self.history, self.guides, self.camera, height, first_row, normal_cos_min, plane_tolerance)
                if not keep_view_dependent:                                     # a reflection or refraction does not move with the surface
                    hit = D.hit_mask(g)
                    mat = np.ascontiguousarray(g[..., 11]).view(np.uint32)
                    vd = np.zeros((rows, width), bool)
                    vd[hit] = np.asarray(view_dependent_materials, bool)[mat[hit]]
                    H = np.where(vd, 0.0, H)
        c, Hn = merge(c0, num_accumulated, c_h, H, max_history)
        self.history = np.concatenate([c, Hn[..., None]], -1)
        self.guides, self.camera, self.key = g.copy(), cam, key
        if iterations == 0:
            r = c * m
        else:
            r = D.atrous(c, g, iterations, sigma_color, sigma_normal, sigma_position) * m
        rgba = np.concatenate([r, np.ones((rows, width, 1))], -1)
        return rgba, D.pack_pixels(r)
