"""The model of the interpolated shading normal (tests/smooth_ref.py, the specification of DESIGN.md 5.14) against what can be said about
it without a device: the radial identity on an icosphere, every fallback of the rule, the float32 statement against the float64 one on
the scene of the GPU test, and the premises of the closed-form radiance case."""
import numpy as np

import integrator_ref as R
import smooth_ref as S


def _sphere_hits(center, radius, camera=S.SPHERE_CAMERA, W=64, H=64):
    mesh = S.icosphere(S.SPHERE_LEVEL, center, radius)
    rows = S.triangle_rows(mesh)
    rays = R.primary_rays(*camera, W / H, W, H).reshape(-1, 3)
    t, tri = S.intersect_mesh(rows, camera[0], rays)
    hit = np.isfinite(t)
    x = (np.asarray(camera[0]) + t[hit, None] * rays[hit]).astype(np.float32)     # a float32 position, as a guide holds it
    return rows, tri[hit], x


def test_radial_identity_in_float64():
    """P = sum w_i p_i and n_i = (p_i - c) / r give m = (P - c) / r: the interpolated normal of an icosphere with radial normals is
    normalize(P - c) exactly in real arithmetic.  float64 vertices and normals, random points of every face, a direction from outside."""
    rng = np.random.default_rng(7)
    c, r = np.array(S.SPHERE_CENTER), S.SPHERE_RADIUS
    v, i = S.icosphere(2, (0.0, 0.0, 0.0), 1.0)
    unit = v[:, :3].astype(np.float64)
    unit /= np.linalg.norm(unit, axis=-1, keepdims=True)
    tri = np.repeat(i.reshape(-1, 3), 16, 0)
    w = rng.dirichlet((1.0, 1.0, 1.0), tri.shape[0])
    p = [c + r * unit[tri[:, k]] for k in range(3)]
    n = [unit[tri[:, k]] for k in range(3)]
    P = sum(w[:, k, None] * p[k] for k in range(3))
    radial = (P - c) / np.linalg.norm(P - c, axis=-1, keepdims=True)
    ns, rule = S.smooth_normal(p[0], p[1], p[2], n[0], n[1], n[2], P, -radial)
    assert np.all(rule == S.INTERPOLATED)
    assert np.abs(ns - radial).max() < 1e-13


def test_float32_statement_on_the_guide_scene():
    """The scene of the GPU test, hits from a float64 traversal: the float32 statement is within 1e-6 of normalize(x - c) (measured
    1.2e-7, which is what leaves the GPU test's 1e-5 its factor of ~50), the flat normal is off by more than 0.1, and the model excludes
    about 1 % of the hit pixels -- the GPU test allows 3 %."""
    for center, radius in ((S.SPHERE_CENTER, S.SPHERE_RADIUS), (S.MOVED_CENTER, S.MOVED_RADIUS)):
        rows, tri, x = _sphere_hits(center, radius)
        assert tri.size > 500
        ns, rule, radial, g, keep = S.sphere_guide_model(rows, tri, x, S.SPHERE_CAMERA[0], center)
        excluded = 1.0 - keep.mean()
        d = x.astype(np.float64) - S.SPHERE_CAMERA[0]
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        n32, rule32 = S.hit_normals(rows, tri, x, d.astype(np.float32), np.float32)
        err32, err64 = np.abs(n32[keep] - radial[keep]).max(), np.abs(ns[keep] - radial[keep]).max()
        flat = np.abs(rows[tri][:, 3:6] - radial).max()
        print(f"centre {center}: {tri.size} hits, excluded {excluded:.4f}, float32 {err32:.2e}, float64 {err64:.2e}, flat {flat:.3f}")
        assert excluded <= 0.02 and np.any(rule == S.GEOMETRIC)
        assert err64 < 1e-7 and err32 < 1e-6 and n32.dtype == np.float32
        assert flat > 0.1
        fallback = rule == S.GEOMETRIC                       # there the normal is the geometric one on the outward side
        assert np.abs(ns[fallback] - g[fallback]).max() < 1e-12
        assert np.array_equal(rule32[keep], rule[keep])


TRI = dict(p0=(0.0, 0.0, 0.0), p1=(1.0, 0.0, 0.0), p2=(0.0, 0.0, -1.0))          # g = +y
P_MID = (0.25, 0.0, -0.25)


def _one(n0, n1, n2, d, P=P_MID, tri=TRI, dtype=np.float64):
    n, rule = S.smooth_normal(tri["p0"], tri["p1"], tri["p2"], n0, n1, n2, P, d, dtype)
    return n, int(rule)


def test_equal_normals_return_n0_untouched():
    n0 = np.array([0.3, 0.8, 0.1], np.float32)               # not unit length: nothing is normalised
    for dtype in (np.float32, np.float64):
        n, rule = _one(n0, n0, n0, (0.0, -1.0, 0.0), dtype=dtype)
        assert rule == S.EQUAL_NORMALS and np.array_equal(n.astype(np.float32).view(np.uint32), n0.view(np.uint32))
    # -0.0 and 0.0 are not bitwise equal: the rule interpolates
    n, rule = _one((0.0, 1.0, 0.0), (-0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0))
    assert rule == S.INTERPOLATED and np.allclose(n, (0.0, 1.0, 0.0))


def test_degenerate_triangle_returns_n0():
    for tri in (dict(p0=(0, 0, 0), p1=(0, 0, 0), p2=(0, 0, -1)), dict(p0=(0, 0, 0), p1=(1, 0, 0), p2=(2, 0, 0))):
        for dtype in (np.float32, np.float64):
            n, rule = _one((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0), tri=tri, dtype=dtype)
            assert rule == S.NO_LENGTH and np.array_equal(n, (0.0, 1.0, 0.0))
    n, rule = _one((0.0, 1.0, 0.0), (np.nan, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))
    assert rule == S.NO_LENGTH and np.array_equal(n, (0.0, 1.0, 0.0))


def test_cancelling_normals_return_n0():
    # u = v = 0.25: m = 0.5 n0 + 0.25 n1 + 0.25 n2 = 0
    for dtype in (np.float32, np.float64):
        n, rule = _one((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), dtype=dtype)
        assert rule == S.NO_LENGTH and np.array_equal(n, (0.0, 1.0, 0.0))
    # just beside it the sum has a length again, and points down: g is flipped with it
    n, rule = _one((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), P=(0.3, 0.0, -0.3))
    assert rule == S.INTERPOLATED and np.allclose(n, (0.0, -1.0, 0.0))


def test_side_flip_keeps_the_geometric_side():
    tilt = np.array([0.6, 0.8, 0.0])
    n1, n2 = (0.6, 0.8, 1e-3), (0.6, 0.8, -1e-3)             # not bitwise equal: the rule interpolates about (0.6, 0.8, 0)
    down = np.array([0.0, -1.0, 0.0])
    n, rule = _one(tilt, n1, n2, down)
    assert rule == S.INTERPOLATED and np.allclose(n, tilt, atol=1e-3)
    graze = np.array([0.9, -0.1, 0.0]) / np.linalg.norm([0.9, -0.1, 0.0])    # d.g < 0 (from above the triangle) but d.ns > 0
    assert np.dot(graze, tilt) > 0 and graze[1] < 0
    for dtype in (np.float32, np.float64):
        n, rule = _one(tilt, n1, n2, graze, dtype=dtype)
        assert rule == S.GEOMETRIC and np.allclose(n, (0.0, 1.0, 0.0))
    # vertex normals that point to the back of the winding: g is negated to their side first
    n, rule = _one(-tilt, tuple(-np.array(n1)), tuple(-np.array(n2)), -graze)
    assert rule == S.GEOMETRIC and np.allclose(n, (0.0, -1.0, 0.0))
    n, rule = _one(-tilt, tuple(-np.array(n1)), tuple(-np.array(n2)), -down)
    assert rule == S.INTERPOLATED and np.allclose(n, -tilt, atol=1e-3)
    # d.ns == 0 exactly
    n, rule = _one((0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 2.0, 0.0), (1.0, 0.0, 0.0))
    assert rule == S.GEOMETRIC and np.allclose(n, (0.0, 1.0, 0.0))


def test_radiance_case_premises_hold():
    """radiance_case asserts its own premises in float64 (light above every shading horizon, no fallback pixel, the flat normal's
    expectation outside its tolerance in at least half of the bins); here they are evaluated without a device, and the sample count is
    what Case.finish allows."""
    c, flat = S.radiance_case()
    assert 32 <= c.spp <= R.MAX_SPP and flat.spp == c.spp
    missed = [d > tol for _, _, d, tol, _ in flat.residuals(c.expected)]
    print(f"spp {c.spp}; the flat expectation misses {sum(missed)} of {len(missed)} bins")
    assert sum(missed) >= len(missed) / 2
    assert c.worst(c.expected)[0] == 0.0
