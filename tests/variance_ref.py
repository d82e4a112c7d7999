"""The variance-guided filter of cgpt_denoise_variance_guided (csrc/device/denoise.hip) stated in numpy float64, for the
tests: the third part of SVGF (Schied et al. 2017) behind the a-trous filter (denoise_ref.py) and the temporal stage (temporal_ref.py).

Luminance l(c) = 0.2126 r + 0.7152 g + 0.0722 b in the filter's input domain (c_0 of denoise_ref: acc / N, over the albedo with
demodulation).  A call
  1. (temporal flag) merges the colour exactly as temporal_ref does and keeps luminance moments {mu, v, K} -- mean, population variance,
     samples covered -- beside the colour history, reprojected with the colour's taps and weights and merged by the pooled-variance
     update; var_t = v' N / (Ke + N) estimates the variance of the merged colour;
  2. estimates var_s, the weighted variance of the luminance over a 7x7 window of the image the passes will read;
  3. takes var = var_t where Ke + N >= min_history_frames N, else var_s;
  4. runs the passes: the 5x5 B3 taps of denoise_ref with the colour edge-stop replaced by exp(-|l_q - l_p| / (sigma_l sqrt(gbar) + 1e-6)),
     gbar the 3x3 Gaussian of the variance, and the variance carried along as sum w^2 var_q / (sum w)^2.

`dtype` runs the arithmetic in another precision (the tests measure how far a float32 run is from this one: the device's tolerance).
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import temporal_ref as T

LUMA = (0.2126, 0.7152, 0.0722)
EPS = 1e-6                        # added to sigma_l sqrt(gbar): a zero variance stops at any difference without a division by zero
G3 = (1.0, 2.0, 1.0)              # the 3x3 Gaussian (1 2 1; 2 4 2; 1 2 1) / 16


def luminance(c, dtype=np.float64):
    T_ = dtype
    c = np.asarray(c, T_)
    return (T_(LUMA[0]) * c[..., 0] + T_(LUMA[1]) * c[..., 1]) + T_(LUMA[2]) * c[..., 2]


def _geometry(guides, dtype):
    g = np.asarray(guides, np.float32)
    return g[..., 0:3].astype(dtype), g[..., 4:7].astype(dtype), D.hit_mask(g)


def _inv_sq(sigma, dtype):
    """1 / sigma^2 of a float32 parameter, in double and rounded once (the device's host side does the same)"""
    s = float(np.float32(sigma))
    return dtype(np.float32(1.0 / (s * s))) if dtype is np.float32 else 1.0 / (s * s)


def _geo_exponent(x, n, hit, dy, dx, inv_n, inv_x):
    """(e_geo, both hit, the tap counts) of the tap p + (dx, dy): |n_q - n_p|^2 / sigma_n^2 + (n_p . (x_q - x_p))^2 / sigma_x^2"""
    xq, ok = D._tap(x, dy, dx)
    nq, _ = D._tap(n, dy, dx)
    hq, _ = D._tap(hit, dy, dx)
    dn = nq - n
    d = xq - x
    dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
    dp = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
    return dn2 * inv_n + dp * dp * inv_x, hit & hq, ok & (hit == hq)


def spatial_variance(c, guides, sigma_normal=0.2, sigma_position=0.3, dtype=np.float64):
    """var_s (rows, width): over the 7x7 window, taps in the band with hit(q) == hit(p), weight exp(-e_geo) for two hits and 1 for two
    misses, d_q = l(c_q) - l(c_p): max(0, sum w d^2 / sum w - (sum w d / sum w)^2)"""
    T_ = dtype
    x, n, hit = _geometry(guides, T_)
    inv_n, inv_x = _inv_sq(sigma_normal, T_), _inv_sq(sigma_position, T_)
    l = luminance(c, T_)
    sw, swd, swd2 = (np.zeros(l.shape, T_) for _ in range(3))
    with np.errstate(under="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                e, both, use = _geo_exponent(x, n, hit, dy, dx, inv_n, inv_x)
                lq, _ = D._tap(l, dy, dx)
                w = np.where(use, np.where(both, np.exp(-e), T_(1)), T_(0)).astype(T_)
                d = lq - l
                sw = sw + w
                swd = swd + w * d
                swd2 = swd2 + (w * d) * d
        m1 = swd / sw
        return np.maximum(T_(0), swd2 / sw - m1 * m1)


def gauss3(var, hit, dtype=np.float64):
    """gbar: the 3x3 Gaussian of var over the immediate neighbours in the band with hit == hit(p), renormalised over them"""
    T_ = dtype
    var = np.asarray(var, T_)
    num, den = np.zeros(var.shape, T_), np.zeros(var.shape, T_)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = T_(G3[dy + 1] * G3[dx + 1] / 16.0)
            vq, ok = D._tap(var, dy, dx)
            hq, _ = D._tap(hit, dy, dx)
            use = ok & (hq == hit)
            num = num + np.where(use, k * vq, T_(0))
            den = den + np.where(use, k, T_(0))
    return num / den


def passes(c, var, guides, iterations, sigma_luminance=4.0, sigma_normal=0.2, sigma_position=0.3, dtype=np.float64):
    """(c_I, var_I) from c (rows, width, 3) and var (rows, width)"""
    T_ = dtype
    x, n, hit = _geometry(guides, T_)
    inv_n, inv_x = _inv_sq(sigma_normal, T_), _inv_sq(sigma_position, T_)
    sl = T_(np.float32(sigma_luminance))
    c = np.asarray(c, T_)
    var = np.asarray(var, T_)
    with np.errstate(under="ignore", over="ignore"):
        for i in range(iterations):
            s = 1 << i
            inv_l = T_(1) / (sl * np.sqrt(gauss3(var, hit, T_)) + T_(EPS))    # once per pixel
            l = luminance(c, T_)
            num, den, numv = np.zeros(c.shape, T_), np.zeros(l.shape, T_), np.zeros(l.shape, T_)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    e_geo, both, use = _geo_exponent(x, n, hit, dy * s, dx * s, inv_n, inv_x)
                    cq, _ = D._tap(c, dy * s, dx * s)
                    lq, _ = D._tap(l, dy * s, dx * s)
                    vq, _ = D._tap(var, dy * s, dx * s)
                    e = np.abs(lq - l) * inv_l + np.where(both, e_geo, T_(0))
                    w = np.where(use, T_(D.K[abs(dx)] * D.K[abs(dy)]) * np.exp(-e), T_(0)).astype(T_)
                    num = num + w[..., None] * cq
                    den = den + w
                    numv = numv + (w * w) * vq
            c = num / den[..., None]
            var = numv / (den * den)
    return c, var


def merge_moments(l0, n_samples, mu_h, v_h, K_h, max_history=64.0, dtype=np.float64):
    """(mu', v', K', var_t, Ke): the pooled-variance update of the moments {mu_h, v_h, K_h} with N samples of luminance l0; K_h = 0 is no
    moments: mu' = l0, v' = 0, K' = N"""
    T_ = dtype
    mh, N = T_(np.float32(max_history)), T_(n_samples)
    l0, mu_h, v_h = np.asarray(l0, T_), np.asarray(mu_h, T_), np.asarray(v_h, T_)
    Ke = np.minimum(np.asarray(K_h, T_), mh)
    has = Ke > 0
    tot = Ke + N
    mu = np.where(has, (Ke * mu_h + N * l0) / tot, l0)
    dm, dl = mu_h - mu, l0 - mu
    v = np.where(has, (Ke * (v_h + dm * dm) + N * (dl * dl)) / tot, T_(0))
    K = np.where(has, np.minimum(tot, mh), N)
    return mu, v, K, v * N / tot, Ke


def pack(r):
    r = np.asarray(r, np.float64)
    return np.concatenate([r, np.ones(r.shape[:2] + (1,))], -1), D.pack_pixels(r)


class VarianceGuided:
    """The state of a context -- the colour history of temporal_ref.Temporal and the moments beside it -- and frame(), one
    cgpt_denoise_variance_guided call.  After a frame: var (what cgpt_read_variance returns), used_temporal (the choice), taps (the
    accepted tap sets of the reprojection, -1 without history), c (the image the passes read)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.history = None           # (rows, width, 4) {c, H}
        self.moments = None           # (rows, width, 3) {mu, v, K}; None: absent for the whole frame

    def denoise_temporal_called(self, history):
        """a cgpt_denoise_temporal call in between: it updates the colour history (to `history`, as read back) without the moments"""
        self.history = np.asarray(history, np.float64)
        self.moments = None

    def frame(self, acc, num_accumulated, guides, camera, height=None, first_row=0, generation=0, iterations=5, sigma_luminance=4.0,
              sigma_normal=0.2, sigma_position=0.3, demodulate=True, light_materials=(), temporal=False, min_history_frames=4,
              view_dependent_materials=(), max_history=64.0, normal_cos_min=0.9, plane_tolerance=0.01, keep_view_dependent=False,
              dtype=np.float64):
        """(rgba (rows, width, 4), pixels uint32 (rows, width))"""
        T_ = dtype
        g = np.asarray(guides, np.float32)
        rows, width = g.shape[:2]
        height = rows if height is None else height
        N = int(num_accumulated)
        m = D.demodulation(g, light_materials) if demodulate else np.ones((rows, width, 3))
        m = m.astype(T_)
        c0 = D.radiance(acc, N).astype(T_) / m
        c = c0
        var_t = None
        self.taps = np.full((rows, width), -1, np.int64)
        if temporal:
            cam = T.camera_array(camera)
            key = (width, height, first_row, rows, generation, bool(demodulate))
            c_h, H = np.zeros((rows, width, 3)), np.zeros((rows, width))
            mom_h = np.zeros((rows, width, 3))
            if self.history is not None and self.key == key:
                mom = self.moments if self.moments is not None else np.zeros((rows, width, 3))
                if self.camera.tobytes() == cam.tobytes():                     # the identity
                    c_h, H, mom_h = self.history[..., :3], self.history[..., 3], mom
                else:
                    c_h, H, self.taps = T.reproject(g, self.history, self.guides, self.camera, height, first_row, normal_cos_min, plane_tolerance, T_)
                    # the moments through the same taps, validity tests and weights
                    mom_h = T.reproject(g, np.concatenate([mom, self.history[..., 3:]], -1), self.guides, self.camera, height, first_row,
                                        normal_cos_min, plane_tolerance, T_)[0]
                    if not keep_view_dependent:
                        hit = D.hit_mask(g)
                        mat = np.ascontiguousarray(g[..., 11]).view(np.uint32)
                        vd = np.zeros((rows, width), bool)
                        vd[hit] = np.asarray(view_dependent_materials, bool)[mat[hit]]
                        H = np.where(vd, 0.0, H)
                        self.taps = np.where(vd, -1, self.taps)
            mhT, NT = T_(np.float32(max_history)), T_(N)
            He = np.minimum(np.asarray(H, T_), mhT)
            c = np.where((He > 0)[..., None], (He[..., None] * np.asarray(c_h, T_) + NT * c0) / (He + NT)[..., None], c0)
            K_h = np.where(H > 0, mom_h[..., 2], 0.0)                          # no colour history: no moments
            mu, v, K, var_t, Ke = merge_moments(luminance(c0, T_), N, mom_h[..., 0], mom_h[..., 1], K_h, max_history, T_)
            self.history = np.concatenate([c, np.minimum(He + NT, mhT)[..., None]], -1).astype(np.float64)
            self.moments = np.stack([mu, v, K], -1).astype(np.float64)
            self.guides, self.camera, self.key = g.copy(), cam, key
            self.used_temporal = (Ke + NT) >= T_(min_history_frames) * NT
        else:
            self.used_temporal = np.zeros((rows, width), bool)
        var_s = spatial_variance(c, g, sigma_normal, sigma_position, T_)
        self.var_s = var_s
        self.var = np.where(self.used_temporal, var_t, var_s) if temporal else var_s
        self.c = c
        return self.finish(c, self.var, g, m, iterations, sigma_luminance, sigma_normal, sigma_position, temporal, acc, N, T_)

    @staticmethod
    def finish(c, var, g, m, iterations, sigma_luminance, sigma_normal, sigma_position, temporal, acc, N, dtype=np.float64):
        """the passes on (c, var) and the packing; iterations = 0 without the temporal stage is cgpt_denoise's identity"""
        if iterations == 0:
            return pack(np.asarray(c, np.float64) * m if temporal else D.radiance(acc, N))
        r, _ = passes(c, var, g, iterations, sigma_luminance, sigma_normal, sigma_position, dtype)
        return pack(r.astype(np.float64) * m)


def variance_guided(acc, num_accumulated, guides, **kw):
    """one call without the temporal stage: (rgba, pixels, var)"""
    model = VarianceGuided()
    rgba, px = model.frame(acc, num_accumulated, guides, None, **kw)
    return rgba, px, model.var
