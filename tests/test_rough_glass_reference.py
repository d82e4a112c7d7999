"""The numpy statement of the rough dielectric lobe (rough_glass_ref.py) checked against itself and against the closed
forms it must contain: the quadrature converges, the kernels' estimator (visible normals, one Fresnel draw, G2 / G1) has the quadrature's
value, alpha -> 0 is the reference's Fresnel interface, and the layered-slab simulation at alpha -> 0 is integrator_ref's K3.  No GPU needed."""
import numpy as np
import pytest

import integrator_ref as I
import rough_glass_ref as RG

SIDES = ((1.0, 1.5), (1.5, 1.0))                    # (etai, etat): from outside, from inside


@pytest.mark.parametrize("etai,etat", SIDES)
def test_two_grid_sizes_agree(etai, etat):
    for rho in (0.1, 0.6, 1.0):
        for cos_o in (0.1, 0.6, 0.75):                               # 0.75: the critical angle from inside, where the TIR edge cuts the lobe's centre
            a = RG.alpha_of(rho)
            coarse = RG.interface_rt(cos_o, a, etai, etat)
            fine = RG.interface_rt(cos_o, a, etai, etat, n_v=4096, n_phi=512)
            assert np.allclose(coarse, fine, rtol=0.0, atol=1e-4), (etai, rho, cos_o, coarse, fine)


@pytest.mark.parametrize("etai,etat", SIDES)
@pytest.mark.parametrize("rho", [0.3, 1.0])
@pytest.mark.parametrize("cos_o", [0.2, 0.6])
def test_the_estimator_has_the_quadratures_value(etai, etat, rho, cos_o):
    a = RG.alpha_of(rho)
    R, T = RG.interface_rt(cos_o, a, etai, etat, n_v=4096, n_phi=512)
    r, r_se, t, t_se, _ = RG.interface_estimate(cos_o, a, etai, etat, 2_000_000, seed=int(1000 * rho + 10 * cos_o + etai))
    assert abs(r - R) < 5.0 * r_se, (r, r_se, R)
    assert abs(t - T) < 5.0 * t_se, (t, t_se, T)
    assert R + T <= 1.0 + 1e-6                                           # single scattering only: nothing is gained


def test_alpha_to_zero_is_the_fresnel_interface():
    a = 1e-3
    for etai, etat in SIDES:
        for cos_o in (0.3, 0.6, 0.9, 0.99):
            k = 1.0 - (etai / etat) ** 2 * (1.0 - cos_o * cos_o)
            if k < 0.05:
                continue                                                 # near and beyond the critical angle: below
            F = float(I.fresnel(cos_o, etai, etat))
            R, T = RG.interface_rt(cos_o, a, etai, etat)
            assert abs(R - F) < 1e-4 and abs(T - (1.0 - F)) < 1e-4, (etai, cos_o, R, T, F)
    for cos_o in (0.2, 0.5, 0.7):                                        # cos of the critical angle from inside: 0.745
        R, T = RG.interface_rt(cos_o, a, 1.5, 1.0)
        assert abs(R - 1.0) < 1e-4 and T < 1e-4, (cos_o, R, T)


def test_tir_shares_from_inside():
    """How often a facet reflects totally at transmission roughness 0.6 from inside: why TIR must reflect."""
    for cos_o, share in ((0.2, 0.80), (0.6, 0.65), (0.95, 0.18)):
        got = RG.interface_estimate(cos_o, RG.alpha_of(0.6), 1.5, 1.0, 400_000, seed=9)[4]
        assert abs(got - share) < 0.03, (cos_o, got, share)


def test_the_slab_at_alpha_to_zero_is_k3():
    c = I.case("K3_advanced_depth9")
    for py, px in ((30, 20), (8, 40)):
        cos_i, want = float(c.key[py, px]), c.expected[py, px]
        mean, se, escaped = RG.slab(cos_i, 1e-3, I.K3_IOR, I.K3_ALBEDO, I.K3_SIGMA, 1.0, I.K3_LC, I.K3_LF, c.max_ray_depth, 1_000_000,
                                    face_half=80.0, seed=5 + py)
        assert np.all(np.abs(mean - want) < 5.0 * se), (cos_i, mean, want, se)
        assert escaped < 1e-4
