"""Morph targets as csrc/host/morph.h states them (cgpth_morph_triangles, cgpt_scene_morph_mesh), in numpy.

morph_f32 is the specification: the same float32 operations in the same order, line for line, the skip of zero weights included, so
the library must equal it bit for bit.  morph_f64 is the model: the same formula in float64 (the normal divided by its length), with
component_bound / normal_bound the forward error of the float32 order of operations against it.

base is (n, 18) float32 triangles (v0, v1, v2, each pos.xyz + normal.xyz), deltas (n_targets, n, 18) float32 displacement records of the
same layout, weights n_targets float32.
"""
import numpy as np

U = 2.0 ** -24          # the unit roundoff of float32


def _views(base, deltas, weights, dtype):
    b = np.ascontiguousarray(base, np.float32).reshape(-1, 18)
    d = np.ascontiguousarray(deltas, np.float32).reshape(-1, b.shape[0], 18)
    w = np.ascontiguousarray(weights, np.float32).ravel()
    assert w.size == d.shape[0]
    return b.astype(dtype), d.astype(dtype), w


def morph_f32(base, deltas, weights) -> np.ndarray:
    """The pose, (n, 18) float32, by the operations of morph.h in float32."""
    b, d, w = _views(base, deltas, weights, np.float32)
    x = b.copy()                                                              # x = base
    active = False
    with np.errstate(all="ignore"):
        for k in range(w.size):                                               # ascending
            if w[k] == np.float32(0.0):                                       # +0 and -0 are both skipped
                continue
            x = x + w[k] * d[k]                                               # product rounded, then sum rounded
            active = True
        if not active:
            return x                                                          # the base triangle, bit for bit
        assert x.dtype == np.float32
        x = x.reshape(-1, 3, 6)
        q = x[..., 3:6]
        l2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        rcp = np.float32(1.0) / np.sqrt(l2)                                   # 1.0f / sqrtf(l2)
        ok = np.isfinite(l2) & (l2 > 0)
        n_out = np.where(ok[..., None], q * rcp[..., None], b.reshape(-1, 3, 6)[..., 3:6])   # else the base normal unchanged
    assert n_out.dtype == np.float32
    return np.concatenate([x[..., 0:3], n_out], axis=-1).reshape(-1, 18)


def morph_f64(base, deltas, weights):
    """The float64 model and what the bounds are made of: pos (n, 3, 3), unit normal (n, 3, 3), |q| (n, 3) of the blended normal
    before it is normalised, and the magnitude sums S = |base| + sum_k |w_k| |d_k| of the positions and of the normals, each (n, 3, 3).
    Every target takes part: a zero weight adds nothing to either."""
    b, d, w = _views(base, deltas, weights, np.float64)
    w = w.astype(np.float64)
    x = (b + np.tensordot(w, d, axes=1)).reshape(-1, 3, 6)
    s = (np.abs(b) + np.tensordot(np.abs(w), np.abs(d), axes=1)).reshape(-1, 3, 6)
    q = x[..., 3:6]
    length = np.linalg.norm(q, axis=-1)
    with np.errstate(all="ignore"):
        unit = q / length[..., None]
    return x[..., 0:3], unit, length, s[..., 0:3], s[..., 3:6]


def gamma(n):
    """gamma_n = n u / (1 - n u): what n roundings can move a term by, relatively"""
    return n * U / (1.0 - n * U)


def component_bound(s, n_targets):
    """Each blended component lies within gamma_{K+1} S of the model.  The term w_k d_k is rounded once as a product and once in each of the
    at most K sums that follow it; the base passes through the K sums: no term sees more than K + 1 roundings."""
    return gamma(n_targets + 1) * s


def normal_bound(s_n, length, n_targets):
    """Each component of the unit normal, in the form of skin_ref.normal_bound.  The blended normal q carries at most e = gamma_{K+1} S_n per
    component; x -> x / |x| moves by at most 2 |dx| / |x|, and the float32 normalisation itself (two products and two sums under the
    root, the root, the reciprocal, one product: a relative error under 8 u on a component of magnitude <= 1) adds 8 u.  Meaningful
    while |e| is small against |q|: the caller masks the corners where 2 |e| / |q| exceeds 0.1."""
    e = np.linalg.norm(component_bound(s_n, n_targets), axis=-1)
    with np.errstate(all="ignore"):
        rel = 2.0 * e / length
    return rel + 8.0 * U, rel
