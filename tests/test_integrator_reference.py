"""The closed forms of integrator_ref.py: self-checks of the float64 model (Fresnel limits, the two irradiance formulas against brute
quadrature, the camera against the oracle's rays), then every case rendered by the CPU oracle and held to the acceptance rule of
integrator_ref.Case.check: 16 quantile bins, |mean(image) - mean(expected)| < 5 sigma_model / sqrt(pixels spp) + 1e-3 |expected| per bin
and channel, exact zeros where the estimator cannot add energy.  No GPU needed; tests/test_gpu_integrator_kat.py runs the same cases on
the device."""
import numpy as np
import pytest

import oracle as O
import integrator_ref as R


# ---- the model against itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1.33, 1.5, 1.517, 2.4])
def test_fresnel_at_normal_incidence(n):
    want = ((n - 1.0) / (n + 1.0)) ** 2
    assert abs(R.fresnel(1.0, 1.0, n) - want) < 1e-15 and abs(R.fresnel(1.0, n, 1.0) - want) < 1e-15


def test_fresnel_goes_to_one_at_grazing_incidence():
    r = R.fresnel(np.array([1e-2, 1e-4, 1e-6]), 1.0, 1.5)
    assert np.all(np.diff(r) > 0.0) and 1.0 - r[-1] < 1e-5 and r[0] > 0.9
    # from the dense side it reaches 1 at the critical angle and stays there
    crit = np.sqrt(1.0 - 1.0 / 1.5 ** 2)
    assert R.fresnel(crit + 1e-9, 1.5, 1.0) > 0.999 and R.fresnel(crit - 1e-3, 1.5, 1.0) == 1.0


def test_fresnel_is_the_same_from_either_side():
    cos_i = np.linspace(0.05, 1.0, 40)
    cos_t = R.refracted_cos(cos_i, 1.0, 1.5)
    assert np.allclose(R.fresnel(cos_i, 1.0, 1.5), R.fresnel(cos_t, 1.5, 1.0), rtol=0, atol=1e-14)


def test_sphere_formula_matches_quadrature():
    x = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, -1.0], [-3.0, 0.0, 0.5]])
    for c, r in (((0.0, 3.6, 2.2), 3.0), ((-3.0, 6.0, 0.0), 2.0), ((1.0, 2.0, 1.0), 0.5)):
        want = R.sphere_irradiance(x, c, r)
        got = R.sphere_cos_moment(x, c, r, 1, n=256)
        assert np.allclose(got, want, rtol=2e-5, atol=0), (c, r, got, want)


def test_polygon_formula_matches_quadrature():
    x = np.array([[0.0, 0.0, 0.0], [2.5, 0.0, -1.5], [-1.0, 0.0, 1.0]])
    for mesh in (R.K2_EQUAL, R.K2_UNEQUAL):
        tris = R.triangles_of(mesh)
        by_triangle = sum(R.polygon_irradiance(x, t) for t in tris)
        outline = mesh[0][:, :3].astype(np.float64)                # the four corners in order: one polygon
        assert np.allclose(by_triangle, R.polygon_irradiance(x, outline), rtol=1e-12)
        got = sum(R.triangle_cos_moment(x, t, 1, n=512) for t in tris)
        assert np.allclose(got, by_triangle, rtol=1e-4, atol=0), (got, by_triangle)
    # an infinite ceiling irradiates with pi: a 2000-unit quad at height 1 comes within its missing rim
    assert abs(R.polygon_irradiance(np.zeros((1, 3)), [(-1e3, 1, -1e3), (1e3, 1, -1e3), (1e3, 1, 1e3), (-1e3, 1, 1e3)])[0] - np.pi) < 1e-2


def test_closed_form_variances():
    """The cosine sampler with the pdf 1 / (2 pi) (SURVEY A-7): Var = 4 a^2 (1/2 - 4/9) per channel; the uniform one under the pdf
    cos / pi is a constant; brute force's uniform hemisphere: a^2 / 3."""
    cos_i = np.array([[0.7]])
    aL = R.K5_ALBEDO * R.K5_LC
    mean, var = R._k5_half("ADVANCED", 0.0, 0.0, True, False, False, cos_i)
    assert np.allclose(mean, 4.0 / 3.0 * aL) and np.allclose(var, 4.0 * aL ** 2 * (0.5 - 4.0 / 9.0))
    mean, var = R._k5_half("ADVANCED", 0.0, 0.0, False, False, False, cos_i)
    assert np.allclose(mean, aL) and np.allclose(var, 0.0, atol=1e-15)
    mean, var = R._k5_half("BRUTE_FORCE", 0.0, 0.0, True, False, False, cos_i)
    assert np.allclose(mean, aL) and np.allclose(var, aL ** 2 / 3.0)
    # the hemisphere moments behind them, by quadrature
    th = (np.arange(200000) + 0.5) / 200000 * (np.pi / 2)
    w = np.sin(th) * (np.pi / 2 / 200000)
    assert abs(np.sum(np.cos(th) ** 2 * w) - 1.0 / 3.0) < 1e-9                       # uniform: E cos^2
    assert abs(np.sum(2.0 * np.cos(th) * np.cos(th) ** 2 * w) - 0.5) < 1e-9         # cosine-weighted: E cos^2
    assert R.NEE_DRAWS * 48 * 48 >= 200_000


@pytest.mark.parametrize("name", ["K1_advanced", "K1_brute_force", "K3_advanced_depth2", "K4_advanced"])
def test_camera_model_matches_the_oracle(name):
    c = R.case(name)
    o, s = c.build()
    origin, d = o.camera_rays(c.W, c.H)
    assert np.array_equal(origin, np.broadcast_to(np.asarray(c.camera[0], np.float32), origin.shape))
    assert np.abs(d - c.rays()).max() < 5e-7
    o.close(); s.close()


def test_k4_leaves_out_at_most_the_cap():
    for name in ("K4_advanced", "K4_brute_force"):
        c = R.case(name)
        assert c.skip.mean() <= R.K4_CAP and 0.2 < c.exact_zero.mean() < 0.8, (c.skip.mean(), c.exact_zero.mean())
    assert all(R.case(n).skip is None for n in R.CASE_NAMES if not n.startswith("K4"))


# ---- every case on the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_oracle_matches_the_closed_form(name):
    c = R.case(name)
    o, s = c.build()
    try:
        origin = np.broadcast_to(np.asarray(c.camera[0], np.float32), (c.H * c.W, 3))
        t, obj, _, _ = o.intersect_rays(origin, c.rays().reshape(-1, 3).astype(np.float32))
        assert np.all(obj == c.primary_object), "every primary ray must hit the intended surface"
        assert np.allclose(t, c.primary_t.ravel(), rtol=1e-5)
        o.render(c.W, c.H, c.spp, render_mode=getattr(O, "MODE_" + c.mode), seed=R.SEED, nthreads=R.oracle_threads())
        c.check(o.accumulator(), "oracle")
    finally:
        o.close(); s.close()
