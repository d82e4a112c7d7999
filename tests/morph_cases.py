"""Morph targets and weights shared by the morph tests (tests/test_morph_reference.py, test_host_morph.py, test_gpu_morph.py).

A case is (base (n, 18) float32, deltas (n_targets, n, 18) float32, weights (n_targets,) float32) for a given (n, 18) bind array.  The
base is the bind array except in `zeros_among`, which plants -0.0 components in it.
"""
import numpy as np

CASES = ("one", "mix", "zeros_among", "all_zero", "flatten", "limit")
FLATTEN_EVERY = 128                                                            # `flatten` cancels the normal of every 128th corner


def random_deltas(rng, n_targets, n, pos=0.05, nrm=0.2):
    """displacement records: position deltas of scale `pos`, normal deltas of scale `nrm`"""
    d = rng.normal(size=(n_targets, n, 3, 6))
    d[..., :3] *= pos
    d[..., 3:] *= nrm
    return d.reshape(n_targets, n, 18).astype(np.float32)


def planted(n):
    """the (triangle, float) places where `zeros_among` plants a -0.0 in the base: the x of corner 0 and the z of corner 2 of every third triangle"""
    t = np.arange(0, n, 3)
    return np.concatenate([t, t]), np.concatenate([np.zeros_like(t), np.full_like(t, 14)])


ZEROS_AMONG_W = np.float32([0.0, 0.5, -0.0, -0.25, 0.0, 1.5, -0.0, 0.75])


def make_case(name, tris, seed=0):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 18)
    n = tris.shape[0]
    rng = np.random.default_rng(seed + 131 * CASES.index(name))
    base = tris.copy()
    if name == "one":
        return base, random_deltas(rng, 1, n), np.float32([1.0])
    if name == "mix":                                                         # weights below 0 and above 1 are used as given
        return base, random_deltas(rng, 3, n), np.float32([-0.5, 0.25, 1.75])
    if name == "zeros_among":
        # The skip is observable: at the planted -0.0 components the active targets' deltas are a zero whose product with the weight is -0.0
        # (x stays -0.0), the skipped targets' deltas are 1: blending them with their +-0 weight would add a +-0 and could turn -0.0 into +0.0
        w = ZEROS_AMONG_W.copy()
        d = random_deltas(rng, w.size, n)
        t, f = planted(n)
        base[t, f] = -0.0
        for k in range(w.size):
            d[k, t, f] = 1.0 if w[k] == 0 else -np.copysign(np.float32(0.0), w[k])
        return base, d, w
    if name == "all_zero":
        return base, random_deltas(rng, 4, n), np.float32([0.0, -0.0, 0.0, -0.0])
    if name == "flatten":                                                     # normal deltas that cancel the base normal exactly: the base normal is kept
        d = random_deltas(rng, 2, n)
        d[1] = 0.0
        c = np.arange(0, 3 * n, FLATTEN_EVERY)                                # corner 0 of triangle 0 always
        dn = d[0].reshape(3 * n, 6)
        dn[c, 3:] = -base.reshape(3 * n, 6)[c, 3:]                            # weight 1: q = n + 1 * (-n) = 0
        return base, d, np.float32([1.0, 0.0])
    if name == "limit":                                                       # the target limit, every target active
        k = 256
        w = rng.uniform(0.005, 0.03, k).astype(np.float32) * np.where(rng.random(k) < 0.5, -1, 1).astype(np.float32)
        return base, random_deltas(rng, k, n), w
    raise ValueError(name)
