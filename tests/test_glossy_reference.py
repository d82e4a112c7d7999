"""The numpy statement of the rough specular lobe (glossy_ref.py) against anchors of its directional albedo, and the
kernels' sampler restated in float64 against the quadrature.  No GPU needed."""
import numpy as np
import pytest

import glossy_ref as G

# R(cos theta_o, alpha = roughness^2): quadrature and 2 M-sample VNDF Monte Carlo, which agree to 2e-4
ANCHORS = {
    0.3: (0.9894, 0.9751, 0.9140),
    0.6: (0.8146, 0.7821, 0.8258),
    1.0: (0.3275, 0.4507, 0.6417),
}
COS_O = (0.9, 0.5, 0.2)


@pytest.mark.parametrize("roughness", sorted(ANCHORS))
def test_directional_albedo_reproduces_the_anchors(roughness):
    got = [G.directional_albedo(c, G.alpha_of(roughness)) for c in COS_O]
    assert np.allclose(got, ANCHORS[roughness], atol=1e-3), (roughness, got)


def test_near_mirror_roughness_keeps_almost_all_energy():
    """roughness 0.1: 0.9986 - 0.9999 over the three angles, to the anchors' 1e-3"""
    got = [G.directional_albedo(c, G.alpha_of(0.1)) for c in COS_O]
    assert all(0.9986 - 1e-3 <= v <= 0.9999 + 1e-3 for v in got) and got[0] > got[2], got


def test_small_alpha_stays_accurate():
    """A uniform (theta_h, phi) grid overshoots by ~4e-4 at alpha = 0.01; the stretched variable does not exceed 1"""
    for c in (0.95, 0.5, 0.1):
        v = G.directional_albedo(c, 0.01)
        assert 0.99 < v <= 1.0 + 1e-6, (c, v)
    assert G.directional_albedo(0.5, 0.0) == 1.0


def test_vndf_sampler_with_g2_over_g1_weight_matches_the_quadrature():
    """The kernels' estimator (visible normals, weight G2/G1, zero below the horizon) converges to R"""
    for rough, c in ((0.3, 0.2), (0.6, 0.5), (1.0, 0.9), (1.0, 0.15)):
        a = G.alpha_of(rough)
        mean, se = G.vndf_estimate(c, a, 400_000, seed=7)
        want = G.directional_albedo(c, a)
        assert abs(mean - want) < 5 * se + 2e-4, (rough, c, mean, want, se)


def test_visible_normal_density_integrates_to_one():
    """D_wo(h) = G1(wo) max(0, wo.h) D(h) / (n.wo) is a density over the hemisphere of h (the sampler's pdf)"""
    for a, c in ((0.09, 0.3), (0.5, 0.7), (1.0, 0.1)):
        n_t, n_p = 4000, 512
        th = (np.arange(n_t) + 0.5) / n_t * (np.pi / 2)
        ph = (np.arange(n_p) + 0.5) / n_p * 2 * np.pi
        T, P_ = np.meshgrid(th, ph, indexing="ij")
        h = np.stack([np.sin(T) * np.cos(P_), np.sin(T) * np.sin(P_), np.cos(T)], -1)
        wo = np.array([np.sqrt(1 - c * c), 0.0, c])
        g1 = 1.0 / (1.0 + G.smith_lambda(c, a))
        dens = g1 * np.maximum(0.0, h @ wo) * G.ggx_d(h[..., 2], a) / c
        total = np.sum(dens * np.sin(T)) * (np.pi / 2 / n_t) * (2 * np.pi / n_p)
        assert abs(total - 1.0) < 5e-3, (a, c, total)
