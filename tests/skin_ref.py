"""Linear blend skinning as csrc/host/skinning.h states it (cgpth_skin_triangles, cgpt_scene_skin_mesh), in numpy.

skin_f32 is the specification: the same float32 operations in the same order, line for line, so the library must equal it bit for
bit.  skin_f64 is the model: the same formula in float64 (the normal divided by its length), with position_bound / normal_bound the
forward error of the float32 order of operations against it.

A skin is per corner: bind (n, 18) float32 triangles (v0, v1, v2, each pos.xyz + normal.xyz), joints (n, 3, 4) indices and weights
(n, 3, 4) float32 -- four influences per corner -- and matrices (n_joints, 12) float32, the rows of [A | b].
"""
import numpy as np

U = 2.0 ** -24          # the unit roundoff of float32


def _views(bind, joints, weights, matrices, dtype):
    b = np.ascontiguousarray(bind, np.float32).reshape(-1, 3, 6).astype(dtype)
    j = np.asarray(joints).reshape(-1, 3, 4).astype(np.int64)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, 3, 4).astype(dtype)
    a = np.ascontiguousarray(matrices, np.float32).reshape(-1, 12).astype(dtype)[j]      # (n, 3, 4, 12): a_k of every corner
    return b, w, a


def skin_f32(bind, joints, weights, matrices) -> np.ndarray:
    """The pose, (n, 18) float32, by the operations of skinning.h in float32."""
    b, w, a = _views(bind, joints, weights, matrices, np.float32)
    with np.errstate(all="ignore"):
        m = w[..., 0, None] * a[..., 0, :]                                    # m = w0*a0
        m = m + w[..., 1, None] * a[..., 1, :]                                # m = m + w1*a1
        m = m + w[..., 2, None] * a[..., 2, :]                                # m = m + w2*a2
        m = m + w[..., 3, None] * a[..., 3, :]                                # m = m + w3*a3
        m = m.reshape(-1, 3, 3, 4)                                            # (triangle, corner, row r, column)
        p, nrm = b[..., 0:3], b[..., 3:6]
        px, py, pz = p[..., None, 0], p[..., None, 1], p[..., None, 2]
        nx, ny, nz = nrm[..., None, 0], nrm[..., None, 1], nrm[..., None, 2]
        pos = ((m[..., 0] * px + m[..., 1] * py) + m[..., 2] * pz) + m[..., 3]   # p'_r = ((m_r0*px + m_r1*py) + m_r2*pz) + m_r3
        q = (m[..., 0] * nx + m[..., 1] * ny) + m[..., 2] * nz                # q_r = (m_r0*nx + m_r1*ny) + m_r2*nz
        l2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        rcp = np.float32(1.0) / np.sqrt(l2)                                   # 1.0f / sqrtf(l2)
        ok = np.isfinite(l2) & (l2 > 0)
        n_out = np.where(ok[..., None], q * rcp[..., None], nrm)              # else the bind normal unchanged
    assert pos.dtype == np.float32 and n_out.dtype == np.float32
    return np.concatenate([pos, n_out], axis=-1).reshape(-1, 18)


def skin_f64(bind, joints, weights, matrices):
    """The float64 model and what the bounds are made of: pos (n, 3, 3), unit normal (n, 3, 3), |q| (n, 3) of the blended normal
    before it is normalised, and the magnitude sums S_p[r] = sum_k |w_k| (sum_c |A_k,rc| |p_c| + |b_k,r|) and S_n[r] = sum_k |w_k| sum_c
    |A_k,rc| |n_c|, each (n, 3, 3)."""
    b, w, a = _views(bind, joints, weights, matrices, np.float64)
    a = a.reshape(*a.shape[:3], 3, 4)                                          # (n, corner, k, r, column)
    m = (w[..., None, None] * a).sum(axis=2)                                   # (n, corner, r, column)
    p, nrm = b[..., 0:3], b[..., 3:6]
    pos = (m[..., :3] * p[..., None, :]).sum(-1) + m[..., 3]
    q = (m[..., :3] * nrm[..., None, :]).sum(-1)
    length = np.linalg.norm(q, axis=-1)
    with np.errstate(all="ignore"):
        unit = q / length[..., None]
    aw = np.abs(w)[..., None, None] * np.abs(a)                                # |w_k| |a_k|
    s_p = ((aw[..., :3] * np.abs(p)[..., None, None, :]).sum(-1) + aw[..., 3]).sum(axis=2)
    s_n = (aw[..., :3] * np.abs(nrm)[..., None, None, :]).sum(-1).sum(axis=2)
    return pos, unit, length, s_p, s_n


def position_bound(s_p):
    """Each posed position component lies within 16 u S_p of the model.  A blended entry is four products and three sums, the row
    another three products and three sums: every term passes through at most 8 roundings, (1 + u)^8 - 1 < 16 u."""
    return 16.0 * U * s_p


def normal_bound(s_n, length):
    """Each component of the unit normal.  The blended normal q carries at most e_r = 16 u S_n[r] per row, as a position does;
    x -> x / |x| moves by at most 2 |dx| / |x|, and the float32 normalisation itself (two products and two sums under the root, the root,
    the reciprocal, one product: a relative error under 8 u on a component of magnitude <= 1) adds 8 u.  Meaningful while |e| is small
    against |q|: the caller masks the corners where 2 |e| / |q| exceeds 0.1."""
    e = np.linalg.norm(16.0 * U * s_n, axis=-1)
    with np.errstate(all="ignore"):
        rel = 2.0 * e / length
    return rel + 8.0 * U, rel
