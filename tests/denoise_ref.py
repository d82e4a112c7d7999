"""The denoiser of cgpt_denoise (csrc/device/denoise.hip) stated in numpy float64, for the tests.

Guides: 12 floats per pixel {x.xyz, t, n.xyz, bits(obj), albedo.xyz, bits(mat_index)}; a miss has obj = 0xFFFFFFFF.  Pass i of an
edge-avoiding a-trous filter has step 2^i and 5x5 taps, skipped outside the band; weights h(dx) h(dy) w_c w_n w_x; a hit and a miss never
mix.  Pass 0 divides the accumulator by num_accumulated in float32 (data.pixels' division) and demodulates; the last pass remodulates.
"""
from __future__ import annotations

import numpy as np

NO_HIT = 0xFFFFFFFF
K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def pack_pixels(rgb) -> np.ndarray:
    """Vec4ToUint (ref: MathLib.h:144-152) in float32: 255 * min(1, v), negatives to 0, truncated; alpha 255"""
    v = np.asarray(rgb, np.float32)
    f = np.float32(255.0) * np.minimum(np.float32(1.0), v)
    f = np.where(f < 0, np.float32(0.0), f)
    c = f.astype(np.int32).astype(np.uint32) & 0xFF
    return (np.uint32(255) << 24) + (c[..., 2] << 16) + (c[..., 1] << 8) + c[..., 0]


def radiance(acc, num_accumulated) -> np.ndarray:
    """c = acc.xyz / N, the float32 division of data.pixels"""
    return np.asarray(acc, np.float32)[..., :3] / np.float32(num_accumulated)


def hit_mask(guides) -> np.ndarray:
    return np.ascontiguousarray(guides[..., 7]).view(np.uint32) != NO_HIT


def demodulation(guides, light_materials) -> np.ndarray:
    """m(p): the albedo per channel where it is >= 1e-3 on a hit whose material is not a light, else 1.  light_materials: is_light of
    every material index"""
    g = np.asarray(guides, np.float32)
    hit = hit_mask(g)
    mat = np.ascontiguousarray(g[..., 11]).view(np.uint32)
    lights = np.asarray(light_materials, bool)
    is_light = np.zeros(hit.shape, bool)
    is_light[hit] = lights[mat[hit]]
    alb = g[..., 8:11].astype(np.float64)
    use = (hit & ~is_light)[..., None] & (g[..., 8:11] >= np.float32(1e-3))
    return np.where(use, alb, 1.0)


def _tap(a, dy, dx):
    """a[y + dy, x + dx] where that is inside the band, and the mask of where it is"""
    H, W = a.shape[:2]
    out = np.zeros_like(a)
    ok = np.zeros((H, W), bool)
    y0, y1 = max(0, -dy), min(H, H - dy)
    x0, x1 = max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        ok[y0:y1, x0:x1] = True
    return out, ok


def atrous(c0, guides, iterations, sigma_color, sigma_normal, sigma_position) -> np.ndarray:
    """c_I from c_0 (rows, width, 3) float64"""
    g = np.asarray(guides, np.float32)
    x = g[..., 0:3].astype(np.float64)
    n = g[..., 4:7].astype(np.float64)
    hit = hit_mask(g)
    c = np.asarray(c0, np.float64)
    for i in range(iterations):
        s = 1 << i
        sc = sigma_color * 2.0 ** -i
        num = np.zeros_like(c)
        den = np.zeros(c.shape[:2])
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, ok = _tap(c, dy * s, dx * s)
                xq, _ = _tap(x, dy * s, dx * s)
                nq, _ = _tap(n, dy * s, dx * s)
                hq, _ = _tap(hit, dy * s, dx * s)
                w = K[abs(dx)] * K[abs(dy)] * np.exp(-np.sum((cq - c) ** 2, -1) / (sc * sc))
                both = hit & hq
                wn = np.exp(-np.sum((nq - n) ** 2, -1) / (sigma_normal * sigma_normal))
                wx = np.exp(-np.sum(n * (xq - x), -1) ** 2 / (sigma_position * sigma_position))
                w = w * np.where(both, wn * wx, 1.0)
                w = np.where(ok & (hit == hq), w, 0.0)
                num += w[..., None] * cq
                den += w
        c = num / den[..., None]
    return c


def denoise(acc, num_accumulated, guides, iterations=5, sigma_color=4.0, sigma_normal=0.2, sigma_position=0.3, demodulate=True,
            light_materials=()):
    """(rgba float64 (rows, width, 4) = {r, 1}, pixels uint32 (rows, width)) of cgpt_denoise on an accumulator band and its guides"""
    c = radiance(acc, num_accumulated)
    if iterations == 0:
        r = c.astype(np.float64)
    else:
        m = demodulation(guides, light_materials) if demodulate else np.ones(c.shape)
        r = atrous(c.astype(np.float64) / m, guides, iterations, sigma_color, sigma_normal, sigma_position) * m
    rgba = np.concatenate([r, np.ones(r.shape[:2] + (1,))], -1)
    return rgba, pack_pixels(r)


def guides_from_hits(desc, origins, dirs, t, obj, tri) -> np.ndarray:
    """The guides of rays whose closest hits are (t, obj, tri) (e.g. the oracle's intersect_rays of its camera_rays), from a flattened
    scene description (cgpt_scene_desc): x = o + d t in float32, the normal of GetRayHitResult (a mesh or triangle object: its
    triangle's v0.normal; a sphere: normalize(x - c); a plane: its normal) and the material's albedo.  (n, 12) float32"""
    import ctypes as C
    n = t.shape[0]
    g = np.zeros((n, 12), np.float32)
    g[:, 3] = np.float32(1e34)
    gu = g.view(np.uint32)
    gu[:, 7] = NO_HIT
    gu[:, 11] = NO_HIT
    hit = obj != NO_HIT
    pos = np.asarray(origins, np.float32) + np.asarray(dirs, np.float32) * np.asarray(t, np.float32)[:, None]
    tris = None
    if desc.n_triangles:
        tris = np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_float)), shape=(desc.n_triangles * 18,)).reshape(-1, 18)
    for k in range(desc.n_objects):
        ob = desc.objects[k]
        sel = hit & (obj == k)
        if not sel.any():
            continue
        if ob.kind == 0:
            nrm = tris[ob.tri_offset + tri[sel], 3:6]
        elif ob.kind == 3:
            nrm = np.broadcast_to(tris[ob.tri_offset, 3:6], (int(sel.sum()), 3))
        elif ob.kind == 1:
            d = pos[sel] - np.asarray(ob.sphere_center, np.float32)
            length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
            nrm = d * (np.float32(1.0) / length)[:, None]
        else:
            nrm = np.broadcast_to(np.asarray(ob.plane_normal, np.float32), (int(sel.sum()), 3))
        g[sel, 0:3] = pos[sel]
        g[sel, 3] = t[sel]
        g[sel, 4:7] = nrm
        gu[sel, 7] = k
        g[sel, 8:11] = np.asarray(desc.materials[ob.mat_index].albedo, np.float32)
        gu[sel, 11] = ob.mat_index
    return g
