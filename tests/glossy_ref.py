"""The rough specular lobe of the render kernels (csrc/device/shade_device.hpp: ggx_sample) stated in numpy float64, for the
tests.

Isotropic GGX with alpha = roughness^2, Fresnel = the constant albedo:
    D(h) = alpha^2 / (pi ((n.h)^2 (alpha^2 - 1) + 1)^2),  L(w) = (-1 + sqrt(1 + alpha^2 tan^2 theta_w)) / 2,  G2 = 1 / (1 + L(wo) + L(wi)).
A pixel whose primary ray meets a rough floor of albedo a under a uniform unit-radiance sky (no other geometry) converges to a * R with
the directional albedo
    R(cos theta_o, alpha) = (1 / cos theta_o) * integral of D(h) G2(wo, wi(h)) (wo.h) [wo.h > 0, wi.n > 0] over the hemisphere of h,
wi(h) = reflect(-wo, h).

Horizon rule (shade_device.hpp: ggx_visible_normal; tests/shade_ref.py states it per sample): a direction wo whose cosine to n is not > 0,
or whose squared cosine is below the smallest normal float32 (HORIZON_COS_SQ; cos < 1.09e-19), is at the horizon -- tan^2 of its angle is
not a float32 and L(wo) would be inf.  The lobe has no energy there: its limit is a weight of 1 on a direction below the horizon.

Quadrature: with x = tan(theta_h) / alpha and s = 1 / (1 + x^2), D(h) cos(theta_h) dw_h = ds dphi / (2 pi) exactly, so the peak of D at
small alpha costs nothing: the integrand left in (s, phi) is G2 (wo.h) / cos(theta_h), smooth up to the two indicator edges.
"""
from __future__ import annotations

import numpy as np


HORIZON_COS_SQ = float(np.float32(1.17549435e-38))


def above_horizon(cos_o) -> bool:
    """The horizon rule of the module docstring."""
    return bool(cos_o > 0.0 and cos_o * cos_o >= HORIZON_COS_SQ)


def alpha_of(roughness: float) -> float:
    return float(roughness) * float(roughness)


def smith_lambda(cos_theta, alpha):
    c2 = np.clip(np.asarray(cos_theta, np.float64) ** 2, 1e-300, 1.0)
    return 0.5 * (-1.0 + np.sqrt(1.0 + alpha * alpha * (1.0 - c2) / c2))


def ggx_d(cos_h, alpha):
    c2 = np.asarray(cos_h, np.float64) ** 2
    return alpha * alpha / (np.pi * (c2 * (alpha * alpha - 1.0) + 1.0) ** 2)


def directional_albedo(cos_o: float, alpha: float, n_s: int = 8192, n_phi: int = 768) -> float:
    """R(cos theta_o, alpha): the lobe's reflected share of a unit sky for light leaving towards wo (midpoint rule in (s, phi))."""
    cos_o = float(cos_o)
    if alpha <= 0.0:
        return 1.0                                                   # the mirror
    sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
    wo = np.array([sin_o, 0.0, cos_o])
    lam_o = smith_lambda(cos_o, alpha)
    s = (np.arange(n_s) + 0.5) / n_s
    phi = (np.arange(n_phi) + 0.5) / n_phi * 2.0 * np.pi
    x = np.sqrt(1.0 / s - 1.0)
    tan_h = alpha * x
    cos_h = 1.0 / np.sqrt(1.0 + tan_h * tan_h)
    sin_h = tan_h * cos_h
    total = 0.0
    for k0 in range(0, n_phi, 256):                                 # in slices: n_s x 256 points at a time
        p = phi[k0:k0 + 256]
        hx = sin_h[:, None] * np.cos(p)[None, :]
        hy = sin_h[:, None] * np.sin(p)[None, :]
        hz = np.broadcast_to(cos_h[:, None], hx.shape)
        oh = wo[0] * hx + wo[2] * hz
        wiz = 2.0 * oh * hz - wo[2]
        ok = (oh > 0.0) & (wiz > 0.0)
        lam_i = smith_lambda(np.where(ok, wiz, 1.0), alpha)
        g2 = 1.0 / (1.0 + lam_o + lam_i)
        total += float(np.sum(np.where(ok, g2 * oh / hz, 0.0)))
    return total / (n_s * n_phi) / cos_o


def directional_albedo_table(cos_o, alpha) -> np.ndarray:
    return np.array([directional_albedo(c, alpha) for c in np.atleast_1d(cos_o)])


def sample_vndf(wo, alpha, u1, u2):
    """Heitz 2018 visible-normal sampling in the local frame (n = +z), float64: the microfacet normals for the draws u1, u2."""
    wo = np.asarray(wo, np.float64)
    vh = np.array([alpha * wo[0], alpha * wo[1], wo[2]])
    vh /= np.linalg.norm(vh)
    lensq = vh[0] ** 2 + vh[1] ** 2
    t1 = np.array([-vh[1], vh[0], 0.0]) / np.sqrt(lensq) if lensq > 0 else np.array([1.0, 0.0, 0.0])
    t2 = np.cross(vh, t1)
    r = np.sqrt(u1)
    ph = 2.0 * np.pi * u2
    p1 = r * np.cos(ph)
    sv = 0.5 * (1.0 + vh[2])
    p2 = (1.0 - sv) * np.sqrt(np.maximum(0.0, 1.0 - p1 * p1)) + sv * r * np.sin(ph)
    p3 = np.sqrt(np.maximum(0.0, 1.0 - p1 * p1 - p2 * p2))
    nh = p1[:, None] * t1 + p2[:, None] * t2 + p3[:, None] * vh
    h = np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0.0, nh[:, 2])], axis=1)
    return h / np.linalg.norm(h, axis=1, keepdims=True)


def vndf_estimate(cos_o: float, alpha: float, n: int, seed: int = 1):
    """Monte Carlo of R with the kernels' estimator: G2/G1 per VNDF sample, 0 below the horizon.  Returns (mean, standard error)."""
    if not above_horizon(cos_o):
        return 0.0, 0.0                                              # the horizon rule: no energy
    rng = np.random.default_rng(seed)
    sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
    wo = np.array([sin_o, 0.0, cos_o])
    h = sample_vndf(wo, alpha, rng.random(n), rng.random(n))
    oh = h @ wo
    wi = 2.0 * oh[:, None] * h - wo
    ok = wi[:, 2] > 0.0
    lam_o = smith_lambda(cos_o, alpha)
    lam_i = smith_lambda(np.where(ok, wi[:, 2], 1.0), alpha)
    w = np.where(ok, (1.0 + lam_o) / (1.0 + lam_o + lam_i), 0.0)
    return float(w.mean()), float(w.std() / np.sqrt(n))
