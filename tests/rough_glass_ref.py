"""The rough dielectric lobe of the render kernels (csrc/device/shade_device.hpp: rough_glass_sample) stated in numpy
float64, for the tests.  It shares no code with the kernels; smith_lambda and sample_vndf are glossy_ref's.

One interface between the indices etai (the side of wo) and etat, isotropic GGX with alpha = transmission_roughness^2, wo = (sin, 0, cos)
around n = +z, c = wo.h, eta = etai / etat, k = 1 - eta^2 (1 - c^2), F = the reference's fresnel() at the facet (1 where k < 0):

(a) directional reflectance and transmittance, the shares of a unit sky above / below that leave towards wo:
        R = (1 / cos_o) * integral of D G2(wo, wi) (wo.h) F       [wo.h > 0] [wi.n > 0]           over the hemisphere of h
        T = (1 / cos_o) * integral of D G2(wo, wt) (wo.h) (1 - F) [wo.h > 0] [k >= 0] [wt.n < 0]  over the hemisphere of h
    G2 = 1 / (1 + L(wo) + L(|w.n|)).  No eta^2 radiance scaling and no multiple scattering: R + T < 1 at high roughness, as in the kernels.
    Quadrature: glossy_ref's s = 1 / (1 + tan^2(theta_h) / alpha^2) makes D cos(theta_h) dw_h = ds dphi / (2 pi); what is left,
    G2 (wo.h) F / cos(theta_h), has a 1 / sqrt(s) end at the horizon of h that the refracted lobe reaches (the reflected one's horizon test
    cuts it off), so s = v^2 and the midpoint rule runs in (v, phi): the factor 2 v removes it.

(b) slab(): a vectorised Monte Carlo of two parallel rough interfaces a thickness apart between a uniform emitter above and one below,
    following the kernels' steps literally -- draws r-less (refractivity 1), u1, u2, the Fresnel float only when k >= 0, physical TIR at
    the facet, albedo * G2 / G1 per interaction, Beer with the LAST inside segment's length on a refraction out (SURVEY A-4), the wrong
    side ends the path, and the depth cut-off `depth > max_ray_depth`.
"""
from __future__ import annotations

import numpy as np

import glossy_ref as G


def alpha_of(transmission_roughness: float) -> float:
    return float(transmission_roughness) * float(transmission_roughness)


def facet_fresnel(c, k, etai, etat):
    """The reference's fresnel(in, out, etai, etat) at a facet with cos_i = c > 0 and cos_t = sqrt(k); 1 where k < 0."""
    ct = np.sqrt(np.maximum(k, 0.0))
    s_pol = (etai * c - etat * ct) / (etai * c + etat * ct)
    p_pol = (etai * ct - etat * c) / (etai * ct + etat * c)
    return np.where(k < 0.0, 1.0, 0.5 * (s_pol * s_pol + p_pol * p_pol))


# ---- (a) one interface ------------------------------------------------------------------------------------------------------------------
def interface_rt(cos_o: float, alpha: float, etai: float, etat: float, n_v: int = 2048, n_phi: int = 256):
    """(R, T) of the docstring by the midpoint rule in (v, phi), s = v^2; phi over half the circle (the integrand is even in sin phi)."""
    cos_o = float(cos_o)
    sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
    eta = etai / etat
    lam_o = G.smith_lambda(cos_o, alpha)
    v = (np.arange(n_v) + 0.5) / n_v
    s = v * v
    tan_h = alpha * np.sqrt(1.0 / s - 1.0)
    cos_h = 1.0 / np.sqrt(1.0 + tan_h * tan_h)
    sin_h = tan_h * cos_h
    phi = (np.arange(n_phi) + 0.5) / n_phi * np.pi
    sum_r = sum_t = 0.0
    for k0 in range(0, n_phi, 128):
        p = phi[k0:k0 + 128]
        hx = sin_h[:, None] * np.cos(p)[None, :]
        hz = np.broadcast_to(cos_h[:, None], hx.shape)
        c = sin_o * hx + cos_o * hz
        front = c > 0.0
        cc = np.where(front, c, 1.0)
        k = 1.0 - eta * eta * (1.0 - cc * cc)
        F = facet_fresnel(cc, k, etai, etat)
        wiz = 2.0 * cc * hz - cos_o
        wtz = -eta * cos_o + (eta * cc - np.sqrt(np.maximum(k, 0.0))) * hz
        ok_r = front & (wiz > 0.0)
        ok_t = front & (k >= 0.0) & (wtz < 0.0)
        g2_r = 1.0 / (1.0 + lam_o + G.smith_lambda(np.where(ok_r, wiz, 1.0), alpha))
        g2_t = 1.0 / (1.0 + lam_o + G.smith_lambda(np.where(ok_t, -wtz, 1.0), alpha))
        jac = (2.0 * v)[:, None] * cc / hz
        sum_r += float(np.sum(np.where(ok_r, jac * g2_r * F, 0.0)))
        sum_t += float(np.sum(np.where(ok_t, jac * g2_t * (1.0 - F), 0.0)))
    return sum_r / (n_v * n_phi) / cos_o, sum_t / (n_v * n_phi) / cos_o


def interface_rt_table(cos_o, alpha, etai, etat, **kw) -> np.ndarray:
    """(n, 2): R and T at every cos_o."""
    return np.array([interface_rt(c, alpha, etai, etat, **kw) for c in np.atleast_1d(cos_o)])


def interface_estimate(cos_o: float, alpha: float, etai: float, etat: float, n: int, seed: int = 1):
    """Monte Carlo of R and T with the kernels' estimator (G2 / G1 per visible normal, one Fresnel draw where k >= 0, 0 on the wrong side).
    Returns (R mean, R standard error, T mean, T standard error, share of samples with k < 0)."""
    rng = np.random.default_rng(seed)
    sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
    wo = np.array([sin_o, 0.0, cos_o])
    h = G.sample_vndf(wo, alpha, rng.random(n), rng.random(n))
    c = h @ wo
    eta = etai / etat
    k = 1.0 - eta * eta * (1.0 - c * c)
    F = facet_fresnel(c, k, etai, etat)
    refracts = (k >= 0.0) & (rng.random(n) > F)
    wiz = 2.0 * c * h[:, 2] - cos_o
    wtz = -eta * cos_o + (eta * c - np.sqrt(np.maximum(k, 0.0))) * h[:, 2]
    ok_r = ~refracts & (wiz > 0.0)
    ok_t = refracts & (wtz < 0.0)
    lam_o = G.smith_lambda(cos_o, alpha)
    wz = np.where(ok_r, wiz, np.where(ok_t, -wtz, 1.0))
    w = (1.0 + lam_o) / (1.0 + lam_o + G.smith_lambda(wz, alpha))
    r, t = np.where(ok_r, w, 0.0), np.where(ok_t, w, 0.0)
    return float(r.mean()), float(r.std() / np.sqrt(n)), float(t.mean()), float(t.std() / np.sqrt(n)), float(np.mean(k < 0.0))


# ---- (b) the layered slab ---------------------------------------------------------------------------------------------------------------
def _visible_normals(wo, alpha, u1, u2, lengths=False):
    """Heitz 2018 visible-normal sampling for one wo per row, local frame n = +z (glossy_ref.sample_vndf takes a single wo).  Every
    operation in wo's float type (tests/shade_ref.py evaluates it in float32 too); alpha a number or one per row.  lengths: also return
    the length of the unstretched vector before it is normalised (how well conditioned h is: nh is a unit vector with float errors)."""
    vh = np.stack([alpha * wo[:, 0], alpha * wo[:, 1], wo[:, 2]], axis=1)
    vh /= np.linalg.norm(vh, axis=1, keepdims=True)
    lensq = vh[:, 0] ** 2 + vh[:, 1] ** 2
    inv = 1.0 / np.sqrt(np.where(lensq > 0.0, lensq, 1.0))
    t1 = np.where((lensq > 0.0)[:, None], np.stack([-vh[:, 1] * inv, vh[:, 0] * inv, np.zeros_like(inv)], axis=1), np.array([1.0, 0.0, 0.0], vh.dtype))
    t2 = np.cross(vh, t1)
    r, ph = np.sqrt(u1), 2.0 * np.pi * u2
    p1 = r * np.cos(ph)
    sv = 0.5 * (1.0 + vh[:, 2])
    p2 = (1.0 - sv) * np.sqrt(np.maximum(0.0, 1.0 - p1 * p1)) + sv * r * np.sin(ph)
    p3 = np.sqrt(np.maximum(0.0, 1.0 - p1 * p1 - p2 * p2))
    nh = p1[:, None] * t1 + p2[:, None] * t2 + p3[:, None] * vh
    h = np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0.0, nh[:, 2])], axis=1)
    length = np.linalg.norm(h, axis=1, keepdims=True)
    return (h / length, length[:, 0]) if lengths else h / length


def slab(cos_o: float, alpha: float, ior: float, albedo, sigma, thickness: float, l_up, l_down, max_ray_depth: int, n: int,
         face_half: float = np.inf, seed: int = 1):
    """Radiance towards a camera above the slab whose primary ray meets the upper face at cos_o.  The upper face's normal is +y, the
    lower face's -y (both outward); the emitters fill the planes above and below.  Returns (mean (3,), standard error (3,), share of the
    paths that travelled further than face_half sideways from where they entered)."""
    rng = np.random.default_rng(seed)
    albedo, sigma, l_up, l_down = (np.asarray(x, np.float64) for x in (albedo, sigma, l_up, l_down))
    sin_o = np.sqrt(max(0.0, 1.0 - cos_o * cos_o))
    out = np.zeros((n, 3))
    escaped = np.zeros(n, bool)
    idx = np.arange(n)                                               # the paths still alive
    d = np.tile(np.array([sin_o, -cos_o, 0.0]), (n, 1))
    upper = np.ones(n, bool)                                         # which face the ray has hit
    seg = np.zeros(n)                                                # ray.t of the ray that hit it (used when it came from inside)
    side = np.zeros((n, 2))                                          # sideways travel (x, z)
    tp = np.ones((n, 3))
    depth = 0
    while idx.size:
        m = idx.size
        ny = np.where(upper, 1.0, -1.0)                              # the face's outward normal (0, ny, 0)
        inside = ny * d[:, 1] >= 0.0
        etai = np.where(inside, ior, 1.0)
        etat = np.where(inside, 1.0, ior)
        eta = etai / etat
        fy = np.where(inside, -ny, ny)                               # n, the normal turned to face the ray: (0, fy, 0)
        # local frame (x, z, fy * y): a reflection of the frame leaves the isotropic lobe as it is
        wo = np.stack([-d[:, 0], -d[:, 2], -d[:, 1] * fy], axis=1)
        u1, u2, u3 = rng.random(m), rng.random(m), rng.random(m)
        live = wo[:, 2] > 0.0
        h = _visible_normals(np.where(live[:, None], wo, np.array([0.0, 0.0, 1.0])), alpha, u1, u2)
        c = np.sum(wo * h, axis=1)
        k = 1.0 - eta * eta * (1.0 - c * c)
        F = facet_fresnel(c, k, etai, etat)
        refracts = (k >= 0.0) & (u3 > F)
        wr = 2.0 * c[:, None] * h - wo
        wt = -eta[:, None] * wo + (eta * c - np.sqrt(np.maximum(k, 0.0)))[:, None] * h
        wt /= np.linalg.norm(wt, axis=1, keepdims=True)
        w = np.where(refracts[:, None], wt, wr)
        live &= np.where(refracts, w[:, 2] < 0.0, w[:, 2] > 0.0)
        lam_o = G.smith_lambda(np.where(live, wo[:, 2], 1.0), alpha)
        lam_w = G.smith_lambda(np.where(live, np.abs(w[:, 2]), 1.0), alpha)
        tp = tp * (albedo[None, :] * ((1.0 + lam_o) / (1.0 + lam_o + lam_w))[:, None])
        beer = refracts & inside
        tp = np.where(beer[:, None], tp * np.exp(-sigma[None, :] * seg[:, None]), tp)
        depth += 1
        if depth > max_ray_depth:
            live[:] = False                                          # the loop condition: the next ray is never traced
        d = np.stack([w[:, 0], w[:, 2] * fy, w[:, 1]], axis=1)       # back to the world
        # where the next ray goes: out to an emitter, or across the slab to the other face
        going_up = d[:, 1] > 0.0
        leaves = np.where(upper, going_up, ~going_up)
        done = live & leaves
        out[idx[done]] = tp[done] * np.where(going_up[done, None], l_up[None, :], l_down[None, :])
        go = live & ~leaves
        t = thickness / np.maximum(np.abs(d[:, 1]), 1e-300)
        side = side + d[:, [0, 2]] * t[:, None]
        escaped[idx[go & (np.max(np.abs(side), axis=1) > face_half)]] = True
        idx, d, upper, seg, side, tp = idx[go], d[go], ~upper[go], t[go], side[go], tp[go]
    return out.mean(axis=0), out.std(axis=0) / np.sqrt(n), float(escaped.mean())
