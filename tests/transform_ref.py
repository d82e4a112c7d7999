"""Per-object transforms (cgpt_scene_update_transforms, rt_device.hpp: xform_ray / xform_normal, shade_device.hpp: get_hit<.., XFORM>,
DESIGN.md 5.16) restated in numpy.  This file is the specification: the host and the device perform these operations, in this order.

An object-to-world matrix is 12 floats, the rows of [A | b]: world = A p + b.

Host (transform_math.h: InvertTransform), in float64 from the float32 entries:
    c00 = a11 a22 - a12 a21, c01 = a12 a20 - a10 a22, c02 = a10 a21 - a11 a20
    det = (a00 c00 + a01 c01) + a02 c02                       refused: det == 0, det not finite
    Ainv = adjugate / det, entry by entry (a division each; the adjugate's entries are two products and a difference)
    binv_i = -((Ainv_i0 b0 + Ainv_i1 b1) + Ainv_i2 b2)
    each of the 12 numbers rounded to float32 once            refused: a result that is not finite as a float32
    a zero result is stored as +0 (x + 0: 0 / det and -(0) are -0 for half of the sign flips)
The device keeps three float4 per object, {Ainv row i, binv_i}.

Device, in float32 without contraction, for a ray (o, d, t) arriving at a transformed object:
    o'_i = ((Ainv_i0 o.x + Ainv_i1 o.y) + Ainv_i2 o.z) + binv_i
    d'_i = (Ainv_i0 d.x + Ainv_i1 d.y) + Ainv_i2 d.z          not renormalised: t is the same number in both spaces
    1 / d', the axis-parallel decision and the slab operands come from d'; the mesh is walked with (o', d'); the next object sees (o, d).
The hit position stays o + d t of the world ray.  The normal of a hit on a transformed object is
    normalize(Ainv^T n),  (Ainv^T n)_j = (Ainv_0j n.x + Ainv_1j n.y) + Ainv_2j n.z,  normalize(a) = a * (1 / sqrt((a.x a.x + a.y a.y) + a.z a.z))
with n = v0.normal or, with the smooth flag, smooth_ref.smooth_normal in object space (P' = o' + d' t, direction d').  An untransformed
object's v0.normal is passed through unnormalised, as before.

The reference's absolute determinant epsilon (|a| < 0.001 in the triangle test) is applied to object-space numbers: scaling moves it.
"""
from __future__ import annotations

import numpy as np

IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)

# Model against baked geometry (tests/test_transform_reference.py measures the model; the GPU test reuses the bounds): rays that differ in
# hit / miss or in the triangle, as a share of all rays, and |dt| / t on the rest.  The model's own figures are 1 of 4096 rays (through a
# shared edge) and 2.7e-6; the bounds leave ~4x for a contracted multiply-add.
MAX_DIFFERENT = 0.005
RAY_BOUND = 1e-5


def is_identity(m) -> bool:
    return bool(np.array_equal(np.ascontiguousarray(m, np.float32).reshape(3, 4).view(np.uint32), IDENTITY.view(np.uint32)))


def invert(m):
    """The 3 x 4 float32 records {Ainv row i, binv_i} of the object-to-world matrix m (12 floats), or None where the call refuses it."""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4)
    if not np.all(np.isfinite(m)):
        return None
    a = m[:, :3].astype(np.float64)
    b = m[:, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        c00 = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
        c01 = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
        c02 = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
        det = (a[0, 0] * c00 + a[0, 1] * c01) + a[0, 2] * c02
        if det == 0.0 or not np.isfinite(det):
            return None
        inv = np.array([
            [c00 / det, (a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]) / det, (a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]) / det],
            [c01 / det, (a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]) / det, (a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]) / det],
            [c02 / det, (a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]) / det, (a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]) / det]], np.float64)
        binv = -((inv[:, 0] * b[0] + inv[:, 1] * b[1]) + inv[:, 2] * b[2])
        rec = np.concatenate([inv, binv[:, None]], 1).astype(np.float32) + np.float32(0.0)
    return rec if np.all(np.isfinite(rec)) else None


def ray_to_object(rec, o, d, dtype=np.float32):
    """(o', d') of world rays o, d (..., 3) under the records rec (3, 4); every operation in `dtype` (the device's: float32)."""
    rec = np.asarray(rec, np.float32).astype(dtype)
    o = np.asarray(o, dtype); d = np.asarray(d, dtype)
    oo = np.stack([((rec[i, 0] * o[..., 0] + rec[i, 1] * o[..., 1]) + rec[i, 2] * o[..., 2]) + rec[i, 3] for i in range(3)], -1)
    od = np.stack([(rec[i, 0] * d[..., 0] + rec[i, 1] * d[..., 1]) + rec[i, 2] * d[..., 2] for i in range(3)], -1)
    return oo.astype(dtype), od.astype(dtype)


def normal_to_world(rec, n, dtype=np.float32):
    """normalize(Ainv^T n) of object-space normals n (..., 3); every operation in `dtype` (the device's: float32)."""
    rec = np.asarray(rec, np.float32).astype(dtype)
    n = np.asarray(n, dtype)
    with np.errstate(all="ignore"):
        a = np.stack([(rec[0, j] * n[..., 0] + rec[1, j] * n[..., 1]) + rec[2, j] * n[..., 2] for j in range(3)], -1).astype(dtype)
        rcp = dtype(1.0) / np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        return (a * rcp[..., None]).astype(dtype)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def intersect_triangles(rows, o, d, tmax=1e34):
    """The reference's Moeller-Trumbore (rt_device.hpp: intersect_triangle, absolute epsilon included) of rays o, d (n, 3) against all
    triangles `rows` (m x 18 float32, original order) in float32, brute force in index order with the running closest t, as a mesh
    without a tree would be walked: (t (n,) float32, tri (n,) int64, -1 on a miss)."""
    r = np.asarray(rows, np.float32)
    v0 = r[:, 0:3]
    e1 = (r[:, 6:9] - v0).astype(np.float32); e2 = (r[:, 12:15] - v0).astype(np.float32)
    o = np.asarray(o, np.float32); d = np.asarray(d, np.float32)
    best = np.full(o.shape[0], np.float32(tmax), np.float32)
    tri = np.full(o.shape[0], -1, np.int64)
    with np.errstate(all="ignore"):
        for k in range(r.shape[0]):
            H = _cross(d, e2[k][None])
            a = _dot(e1[k][None], H)
            f = np.float32(1.0) / a
            S = o - v0[k][None]
            u = f * _dot(S, H)
            Q = _cross(S, e1[k][None])
            v = f * _dot(d, Q)
            t = f * _dot(e2[k][None], Q)
            ok = ~(np.abs(a) < np.float32(0.001)) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & (t > 0) & (t < best)
            best = np.where(ok, t, best).astype(np.float32)
            tri = np.where(ok, k, tri)
    return best, tri


def model_intersect(rows, m, o, d):
    """The model: world rays against the object-space triangles `rows` under the object-to-world matrix m."""
    oo, od = ray_to_object(invert(m), o, d)
    return intersect_triangles(rows, oo, od)


def bake_rows(rows, m):
    """The triangles `rows` with positions A p + b formed in float64 and rounded once (normals left as they are)."""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4).astype(np.float64)
    out = np.array(rows, np.float32, copy=True)
    for c in (0, 6, 12):
        out[:, c:c + 3] = (rows[:, c:c + 3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    return out


def bake_vertices(vertices, m, normals=True):
    """Vertices (n x 6) moved to the world in float64: positions A p + b; normals normalize(A^-T n)."""
    m = np.ascontiguousarray(m, np.float32).reshape(3, 4).astype(np.float64)
    out = np.array(vertices, np.float32, copy=True)
    out[:, 0:3] = (vertices[:, 0:3].astype(np.float64) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    if normals:
        n = vertices[:, 3:6].astype(np.float64) @ np.linalg.inv(m[:, :3])
        out[:, 3:6] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    return out


def compare_hits(t_a, tri_a, t_b, tri_b):
    """(share of rays that differ in hit / miss or triangle, largest |dt| / t on the rest that hit)."""
    differ = tri_a != tri_b
    same_hit = ~differ & (tri_a >= 0)
    rel = np.abs(t_a[same_hit].astype(np.float64) - t_b[same_hit].astype(np.float64)) / t_b[same_hit].astype(np.float64)
    return float(differ.mean()), float(rel.max()) if rel.size else 0.0


# ---- the transforms and rays of the model test, shared with the GPU test ------------------------------------------------------------------
MODEL_CENTER, MODEL_LEVEL = (0.2, -0.1, 0.3), 2
MODEL_SCALES = ((1.0, 1.0, 1.0), (1.5, 1.5, 1.5), (1.5, 0.75, 1.25))
MODEL_SHIFT = (3.0, -2.0, 5.0)
MODEL_RAYS = 4096


def rotation(axis, angle):
    """Rodrigues' rotation matrix, float64."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def affine(A, b):
    return np.concatenate([np.asarray(A, np.float64), np.asarray(b, np.float64)[:, None]], 1).astype(np.float32)


def model_transform(scale):
    """A = rotation by 0.7 rad about (1, 2, 3) times diag(scale), b = MODEL_SHIFT."""
    return affine(rotation((1.0, 2.0, 3.0), 0.7) @ np.diag(scale), MODEL_SHIFT)


def model_rays(m, scale, n=MODEL_RAYS, seed=7):
    """n seeded rays from a sphere of radius 8 around the moved centre, aimed into a ball of radius 1.3 max(scale): (o, d) float32,
    d normalised in float64 and rounded."""
    rng = np.random.default_rng(seed)
    m64 = np.asarray(m, np.float64)
    c = m64[:, :3] @ np.asarray(MODEL_CENTER, np.float64) + m64[:, 3]
    u = rng.standard_normal((n, 3)); u /= np.linalg.norm(u, axis=-1, keepdims=True)
    o = c + 8.0 * u
    w = rng.standard_normal((n, 3)); w /= np.linalg.norm(w, axis=-1, keepdims=True)
    target = c + 1.3 * max(scale) * w * rng.random((n, 1)) ** (1.0 / 3.0)
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


# ---- exact transforms: sign flips, under which every operation above is exact -------------------------------------------------------------
HALF_TURN = affine(np.diag([-1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))               # a half turn about y
MIRROR_Z = affine(np.diag([1.0, 1.0, -1.0]), (0.0, 0.0, 0.0))                 # a mirror (det < 0)


def flip_vertices(vertices, m):
    """Vertices (n x 6) under a sign-flip transform's inverse (its own inverse): the object-space mesh that the transform brings back.
    A flipped zero is stored as +0, as the device's arithmetic produces it."""
    s = np.diag(np.asarray(m, np.float32).reshape(3, 4)[:, :3]).astype(np.float32)
    out = np.array(vertices, np.float32, copy=True)
    out[:, 0:3] *= s; out[:, 3:6] *= s
    return out + np.float32(0.0)                                             # -0 + 0 = +0


def flip_nodes(nodes, m):
    """Exported BVH nodes (structured or (n, 8)-viewable cgpt_bvh_node: min xyz, left_first, max xyz, prim_count) under the same flip:
    on a flipped axis min' = -max, max' = -min; everything else kept."""
    s = np.diag(np.asarray(m, np.float32).reshape(3, 4)[:, :3])
    raw = np.array(nodes, copy=True).view(np.float32).reshape(-1, 8)
    out = raw.copy()
    for ax in range(3):
        if s[ax] < 0:
            out[:, ax] = -raw[:, 4 + ax] + np.float32(0.0)
            out[:, 4 + ax] = -raw[:, ax] + np.float32(0.0)
    return out
