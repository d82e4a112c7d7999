"""The float64 model of resampled light sampling (ris_ref.py) against the closed forms it is used with.  No GPU needed.

The model's Monte Carlo mean must be the closed form E[c V] for every number of candidates (the estimator is unbiased, and M does not
appear in the expectation); at M = 1 it must be integrator_ref's own NEE model; and the reservoir's first-candidate rule is exercised with
u = 1.0, which numpy's generator never returns and the device's random_float can."""
import numpy as np
import pytest

import integrator_ref as R
import ris_ref as S

DRAWS_PER_PIXEL = 870            # 48 * 48 * 870 = 2 004 480 >= 2e6 draws a case
SCENES = {
    "R1": lambda: S.r1_lights(),
    "R2": lambda: S.case("R2_M4")[0].ris["lights"],
    "R3": lambda: S.case("R3_M4")[0].ris["lights"],
}
_CASE_OF = {"R1": "R1_M2", "R2": "R2_M4", "R3": "R3_M4"}


@pytest.mark.parametrize("M", [1, 2, 8, 32])
@pytest.mark.parametrize("scene", list(SCENES))
def test_monte_carlo_mean_is_the_closed_form(scene, M):
    c, _ = S.case(_CASE_OF[scene])                       # the closed form and the hit points; M does not appear in either
    x, expected = c.ris["x"].reshape(-1, 3), c.expected.reshape(-1, 3)
    assert x.shape[0] * DRAWS_PER_PIXEL >= 2_000_000
    first, cov, _ = S.moments(x, SCENES[scene](), S.ALBEDO, 1.0, M, expected, draws=DRAWS_PER_PIXEL, seed=100 + M)
    got, want = first.mean(0), expected.mean(0)
    se = np.sqrt(S.variance_of(cov).sum(0) / DRAWS_PER_PIXEL) / x.shape[0]      # of the mean over all pixels' draws
    print(scene, M, "mean", got, "closed form", want, "standard errors off", (got - want) / se)
    assert np.all(np.abs(got - want) < 5.0 * se), (scene, M, got, want, se)
    # and bin by bin, as Case.check looks at an image
    for sel in c.bins():
        s = sel.ravel()
        se_b = np.sqrt(S.variance_of(cov)[s].sum(0) / DRAWS_PER_PIXEL) / s.sum()
        assert np.all(np.abs(first[s].mean(0) - expected[s].mean(0)) < 5.0 * se_b), (scene, M)


def test_one_candidate_is_k1_nee_variance():
    """M = 1 on K1's lights: the model's variance and k1_nee_variance's are two Monte Carlo estimates of one number."""
    k1 = R.case("K1_advanced")
    lights = [S.sphere_light(l[0], l[1], l[2], l[3]) for l in R.K1_FAR[:1]]
    _, x = R._hits_on_plane(k1.rays(), k1.camera[0], 0.0)
    ours = []
    for seed in (11, 12):                                # two independent seeds: their own difference is the Monte Carlo error's scale
        _, cov, m22 = S.moments(x, lights, R.K1_ALBEDO, 1.0, 1, k1.expected, draws=R.NEE_DRAWS, seed=seed)
        var = S.variance_of(cov)
        m4 = np.stack([m22[:, 0, 0], m22[:, 1, 1], m22[:, 2, 2]], -1)
        se = np.sqrt(((m4 - var * var) / R.NEE_DRAWS).sum(0)) / var.shape[0]    # of the image mean of a pixel variance estimate
        ours.append((var.mean(0), se))
    theirs = k1.variance.reshape(-1, 3).mean(0)
    print("k1_nee_variance", theirs, "ris_ref M = 1", ours[0][0], ours[1][0], "standard error", ours[0][1])
    for mean, se in ours:
        assert np.all(np.abs(mean - theirs) < 5.0 * np.sqrt(2.0) * se), (mean, theirs, se)
    assert np.all(np.abs(ours[0][0] - ours[1][0]) < 5.0 * np.sqrt(2.0) * ours[0][1])


def test_first_candidate_rule_with_u_equal_to_one():
    """A candidate with w > 0 that finds the reservoir empty is taken even when u = 1.0 (u wsum < w is then false); a weightless candidate
    is never taken; a later candidate with u = 1.0 is not; and the sample is c_y wsum / (M w_y)."""
    res = S.Reservoir(3)
    one = np.ones(3)
    c0 = np.array([[0.0, 0.0, 0.0], [0.2, 0.1, 0.1], [0.0, 0.0, 0.0]])       # reservoir 0 and 2: w = 0; reservoir 1: w = 0.4
    assert res.update(c0, one, np.array([0.0, 1.0, 0.0])).tolist() == [False, True, False]
    c1 = np.array([[0.3, 0.3, 0.4], [3.0, 3.0, 3.0], [0.0, 0.0, 0.0]])
    assert res.update(c1, one, np.array([1.0, 1.0, 1.0])).tolist() == [True, False, False]   # 0: first with w > 0, taken at u = 1; 1: kept
    c2 = np.array([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert res.update(c2, one, np.array([0.7, 0.0, 0.0])).tolist() == [True, False, False]   # 0.7 * 4 < 3
    got = res.estimate(3)
    assert np.allclose(got[0], c2[0] * (4.0 / (3 * 3.0))) and np.allclose(got[1], c0[1] * (9.4 / (3 * 0.4))) and np.all(got[2] == 0.0)
    # without the rule, u = 1.0 would lose the light of a one-light sample
    lone = S.Reservoir(1)
    lone.update(np.array([[0.5, 0.25, 0.25]]), np.ones(1), np.array([1.0]))
    assert np.allclose(lone.estimate(1), [[0.5, 0.25, 0.25]])


def test_cases_fit_the_sample_budget_and_name_their_candidates():
    for name in S.CASE_NAMES:
        c, M = S.case(name)
        assert 32 <= c.spp <= R.MAX_SPP and 1 < M <= 32, (name, c.spp, M)
    assert {S.case(n)[1] for n in ("R1_M2", "R1_M8", "R1_M32")} == {2, 8, 32}
    assert any(S.case(n)[0].max_ray_depth > 0 for n in S.CASE_NAMES)
