"""The model of per-object transforms (tests/transform_ref.py, the specification of DESIGN.md 5.16) against what can be said about it
without a device: brute-force float32 Moeller-Trumbore on geometry baked in float64, and the transforms under which it is exact."""
import numpy as np
import pytest

import smooth_ref as S
import transform_ref as T


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("scale", T.MODEL_SCALES)
def test_model_against_baked_geometry(scale):
    """Measured here: no ray differs in hit / miss, at most 1 of 4096 hits another triangle (a shared edge), |dt| / t <= 2.7e-6."""
    rows = S.triangle_rows(S.icosphere(T.MODEL_LEVEL, T.MODEL_CENTER, 1.0))
    m = T.model_transform(scale)
    o, d = T.model_rays(m, scale)
    t_model, tri_model = T.model_intersect(rows, m, o, d)
    t_baked, tri_baked = T.intersect_triangles(T.bake_rows(rows, m), o, d)
    differ, rel = T.compare_hits(t_model, tri_model, t_baked, tri_baked)
    hits = (tri_baked >= 0).mean()
    print(f"scale {scale}: {hits:.3f} of the rays hit, {differ * T.MODEL_RAYS:.0f} differ in hit / miss or triangle, max |dt| / t = {rel:.3e}")
    assert 0.3 < hits < 0.95                                      # the rays test both outcomes
    assert differ <= T.MAX_DIFFERENT and rel <= T.RAY_BOUND


def test_inverse_matches_float64_linear_algebra():
    for scale in T.MODEL_SCALES:
        m = T.model_transform(scale)
        rec = T.invert(m).astype(np.float64)
        a, b = m[:, :3].astype(np.float64), m[:, 3].astype(np.float64)
        want = np.concatenate([np.linalg.inv(a), (-np.linalg.inv(a) @ b)[:, None]], 1)
        assert np.allclose(rec, want, rtol=2e-7, atol=1e-7)
    assert np.array_equal(_bits(T.invert(T.IDENTITY)[:, :3]), _bits(T.IDENTITY[:, :3]))


@pytest.mark.parametrize("m", [np.zeros((3, 4)), [[1, 2, 3, 0], [2, 4, 6, 0], [0, 0, 1, 0]], [[1, 0, 0, np.nan], [0, 1, 0, 0], [0, 0, 1, 0]],
                               [[np.inf, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[1e-39, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]],
                               [[1e-20, 0, 0, 1e30], [0, 1, 0, 0], [0, 0, 1, 0]]])
def test_model_refuses_what_cannot_be_inverted(m):
    assert T.invert(np.array(m, np.float32)) is None


@pytest.mark.parametrize("flip", [T.HALF_TURN, T.MIRROR_Z])
def test_sign_flips_are_exact(flip):
    rec = T.invert(flip)
    s = np.diag(flip[:, :3])
    assert np.array_equal(_bits(rec), _bits(flip))                # the inverse of a sign flip is itself, its zeros +0
    rng = np.random.default_rng(11)
    o = rng.standard_normal((256, 3)).astype(np.float32); d = rng.standard_normal((256, 3)).astype(np.float32)
    oo, od = T.ray_to_object(rec, o, d)
    assert np.array_equal(_bits(oo), _bits(o * s)) and np.array_equal(_bits(od), _bits(d * s))
    # the transformed flat normal of an axis-aligned unit normal (zeros stored as +0) equals it bitwise
    for ax in range(3):
        for sign in (1.0, -1.0):
            n = np.zeros(3, np.float32); n[ax] = sign
            stored = (n * s + np.float32(0.0)).astype(np.float32)             # the object-space normal, its zeros +0
            assert np.array_equal(_bits(T.normal_to_world(rec, stored)), _bits(n)), (ax, sign)
