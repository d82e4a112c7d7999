"""The numpy statement of the variance-guided filter (variance_ref.py; cgpt_denoise_variance_guided) against closed forms,
and how far a float32 run of it is from the float64 one on the scenes, sizes and frames of the device tests -- the measurement the
device's tolerance rests on (variance_cases.DEV32).  No GPU."""
import numpy as np
import pytest

import denoise_ref as D
import temporal_ref as T
import temporal_cases as TC
import variance_ref as V
import variance_cases as VC

PW, PH = 16, 12


def plane_camera(cx=0.0):
    return np.float32([cx, 0, 8, cx - 1, 0.75, 7, cx + 1, 0.75, 7, cx - 1, -0.75, 7])


def plane_guides(cx=0.0):
    """a fronto-parallel plane z = 0 seen from (cx, 0, 8): one pixel is one world unit, every pixel a hit of object 0 with normal +z"""
    px, py = np.meshgrid(np.arange(PW), np.arange(PH))
    x = np.stack([cx - 8.0 + px, 6.0 - py, np.zeros((PH, PW))], -1)
    g = np.zeros((PH, PW, 12), np.float32)
    g[..., 0:3] = x
    g[..., 3] = np.sqrt(np.sum((x - [cx, 0, 8]) ** 2, -1))
    g[..., 6] = 1.0
    gu = g.view(np.uint32)
    gu[..., 7] = 0
    g[..., 8:11] = 0.5
    gu[..., 11] = 1
    return g


def grey(l, n=1):
    """an accumulator of n samples whose radiance is the grey level l (luminance l: the three weights sum to 1)"""
    a = np.zeros(np.shape(l) + (4,), np.float32)
    a[..., :3] = np.asarray(l, np.float32)[..., None] * n
    return a


KW = dict(demodulate=False, light_materials=[False, False], view_dependent_materials=[False, False])


def test_luminance_weights_sum_to_one():
    assert abs(sum(V.LUMA) - 1.0) < 1e-15
    assert V.luminance(np.float64([[0.2, 0.5, 0.9]]))[0] == pytest.approx(0.2126 * 0.2 + 0.7152 * 0.5 + 0.0722 * 0.9, rel=1e-15)


def test_a_constant_image_has_no_variance_and_comes_back_unchanged():
    g = plane_guides()
    acc = np.zeros((PH, PW, 4), np.float32)
    acc[..., :3] = np.float32([0.6, 0.9, 0.3])
    rgba, px, var = V.variance_guided(acc, 2, g, iterations=5, **KW)
    assert np.all(var == 0)
    assert np.allclose(rgba[..., :3], np.float32([0.3, 0.45, 0.15]), rtol=1e-14, atol=0) and np.all(rgba[..., 3] == 1)
    assert np.array_equal(px, D.pack_pixels(acc[..., :3] / np.float32(2)))


def test_a_checker_pattern_has_the_closed_form_spatial_variance():
    g = plane_guides()
    yy, xx = np.mgrid[0:PH, 0:PW]
    a, b = 0.25, 0.75
    l = np.where((xx + yy) % 2 == 0, a, b)
    var = V.spatial_variance(grey(l)[..., :3], g)
    # an interior pixel sees 49 taps of weight 1 (a flat plane: no normal or plane distance): 25 of its own value (d = 0), 24 of the other
    want = (b - a) ** 2 * (24 / 49) * (25 / 49)
    assert np.allclose(var[3:-3, 3:-3], want, rtol=1e-12, atol=0)
    assert var[0, 0] == pytest.approx((b - a) ** 2 / 4, rel=1e-12)          # a corner: 4 x 4 taps in the band, 8 and 8
    # a miss never mixes with a hit: with the right half missing, a pixel beside the edge sees 4 columns of 7 taps
    gm = g.copy()
    gm.view(np.uint32)[:, PW // 2:, 7] = D.NO_HIT
    vm = V.spatial_variance(grey(l)[..., :3], gm)
    n_own, n_other = 14, 14                                                   # 28 taps, half of each value
    assert vm[5, PW // 2 - 1] == pytest.approx((b - a) ** 2 * (n_other / 28) * (n_own / 28), rel=1e-12)
    assert vm[5, PW // 2] == pytest.approx((b - a) ** 2 * (n_other / 28) * (n_own / 28), rel=1e-12)   # two misses: weight 1


def test_moments_over_static_frames_are_the_population_mean_and_variance():
    rng = np.random.default_rng(7)
    g, cam = plane_guides(), plane_camera()
    K, N = 5, 3
    ls = rng.uniform(0.0, 2.0, (K, PH, PW))
    accs = [grey(ls[k], N) for k in range(K)]
    l32 = np.stack([V.luminance(D.radiance(a, N).astype(np.float64)) for a in accs])   # the frames' luminances: float32 radiance
    m = V.VarianceGuided()
    for k in range(K):
        m.frame(accs[k], N, g, cam, height=PH, iterations=0, temporal=True, min_history_frames=1, **KW)
        assert np.allclose(m.moments[..., 0], l32[:k + 1].mean(0), rtol=1e-12, atol=0)
        assert np.allclose(m.moments[..., 1], l32[:k + 1].var(0), rtol=1e-9, atol=1e-15)
        assert np.all(m.moments[..., 2] == (k + 1) * N)
        assert np.allclose(m.var, l32[:k + 1].var(0) / (k + 1), rtol=1e-9, atol=1e-15)   # var_t: the variance of the mean of k + 1 frames
        assert np.all(m.used_temporal)
    # the cap: with max_history = 2 N the update is the moving form, Ke = 2 N however long the history
    m = V.VarianceGuided()
    mu = v = None
    for k in range(K):
        m.frame(accs[k], N, g, cam, height=PH, iterations=0, temporal=True, max_history=2.0 * N, **KW)
        l0 = l32[k]
        if k == 0:
            mu, v = l0, np.zeros_like(l0)
        else:
            Ke = min(k * N, 2 * N)
            mu_n = (Ke * mu + N * l0) / (Ke + N)
            v = (Ke * (v + (mu - mu_n) ** 2) + N * (l0 - mu_n) ** 2) / (Ke + N)
            mu = mu_n
        assert np.allclose(m.moments[..., 0], mu, rtol=1e-12, atol=0) and np.allclose(m.moments[..., 1], v, rtol=1e-9, atol=1e-15)
        assert np.all(m.moments[..., 2] == min((k + 1) * N, 2 * N))


def test_open_edge_stops_shrink_a_uniform_variance_by_the_squared_kernel():
    g = plane_guides()
    c = np.full((PH, PW, 3), 0.4)
    c2, var = V.passes(c, np.full((PH, PW), 0.09), g, 1)
    assert np.allclose(var[2:-2, 2:-2], 0.09 * (70 / 256) ** 2, rtol=1e-12, atol=0)   # sum h^2 = 70 / 256 per axis, sum h = 1
    assert np.allclose(c2, 0.4, rtol=1e-14, atol=0)


def test_a_luminance_step_between_noise_free_halves_is_not_blurred():
    g = plane_guides()
    l = np.where(np.arange(PW) < PW // 2, 0.2, 0.8) * np.ones((PH, 1))
    c = grey(l)[..., :3].astype(np.float64)
    out, var = V.passes(c, np.zeros((PH, PW)), g, 5)
    assert np.allclose(out, c, rtol=1e-14, atol=0) and np.all(var == 0)
    # ... while the same step inside its noise is: a variance of 1 opens the stop (sigma_l = 4 standard deviations)
    out, _ = V.passes(c, np.ones((PH, PW)), g, 5)
    assert 0.3 < out[PH // 2, PW // 2 - 1, 0] < 0.7


def test_the_estimate_switches_to_the_temporal_one_at_min_history_frames():
    rng = np.random.default_rng(8)
    g, cam = plane_guides(), plane_camera()
    m = V.VarianceGuided()
    for k in range(4):
        m.frame(grey(rng.uniform(0, 1, (PH, PW)), 2), 2, g, cam, height=PH, iterations=1, temporal=True, min_history_frames=3, **KW)
        assert np.all(m.used_temporal == (k >= 2)), k                         # Ke + N = 2 (k + 1) >= 3 x 2 from the third frame on
        want = m.moments[..., 1] * 2 / (2 * (k + 1)) if k >= 2 else m.var_s
        assert np.array_equal(m.var, want)
    assert not np.allclose(m.var, m.var_s)


def test_a_pixel_revealed_by_a_camera_move_starts_again_with_the_spatial_estimate():
    rng = np.random.default_rng(9)
    m = V.VarianceGuided()
    for k in range(3):
        m.frame(grey(rng.uniform(0, 1, (PH, PW)), 2), 2, plane_guides(0.0), plane_camera(0.0), height=PH, iterations=0, temporal=True,
                min_history_frames=2, **KW)
    a = grey(rng.uniform(0, 1, (PH, PW)), 1)
    m.frame(a, 1, plane_guides(2.0), plane_camera(2.0), height=PH, iterations=0, temporal=True, min_history_frames=2, **KW)   # two pixels to the right
    assert np.all(m.moments[:, :-2, 2] == 7) and np.all(m.used_temporal[:, :-2])
    assert np.all(m.moments[:, -2:, 2] == 1) and not np.any(m.used_temporal[:, -2:])   # newly exposed: K' = N
    assert np.array_equal(m.var[:, -2:], m.var_s[:, -2:]) and np.all(m.moments[:, -2:, 1] == 0)
    assert np.array_equal(m.moments[:, -2:, 0], V.luminance(a[..., :3].astype(np.float64))[:, -2:])
    # a cgpt_denoise_temporal call in between drops the moments of the whole frame and keeps the colour history
    hist = m.history.copy()
    m.denoise_temporal_called(hist)
    m.frame(a, 1, plane_guides(2.0), plane_camera(2.0), height=PH, iterations=0, temporal=True, min_history_frames=2, **KW)
    assert np.all(m.moments[..., 2] == 1) and not np.any(m.used_temporal) and np.all(m.history[:, :-2, 3] == 8)


# ---- a float32 run of the statement on the device tests' scenes, sizes and frames -------------------------------------------------------

def oracle_frame(o, s, view, w, h, n, seed):
    """(accumulator, guides, camera) of n samples from `view`, by the oracle"""
    o.set_camera(view[0], view[1], TC.FOV, w / h)
    s.set_camera(view[0], view[1], TC.FOV, w / h)
    o.reset_accumulator()
    o.render(w, h, n, seed=seed, nthreads=4)
    ro, rd = o.camera_rays(w, h)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    t, obj, tri, _ = o.intersect_rays(ro, rd)
    return o.accumulator(), D.guides_from_hits(s.flatten(), ro, rd, t, obj, tri).reshape(h, w, 12), T.camera_array(s.camera())


def lights_of(s):
    desc = s.flatten()
    return [bool(desc.materials[k].is_light) for k in range(desc.n_materials)]


@pytest.mark.parametrize("which", TC.SCENES)
def test_a_float32_run_stays_within_the_recorded_deviation(which):
    o, s = TC.scene_pair(which)
    lights, vd = lights_of(s), TC.view_dependent_materials(s)
    worst = {}

    def note(what, got, ref, keep=None):
        e = VC.rel_err(got, ref)
        worst[what] = max(worst.get(what, 0.0), float(e.max() if keep is None else e[keep].max()))

    for (w, h), n in (((VC.W, VC.H), 3), (VC.SMALL, 1), (VC.SMALL, 4)):
        acc, g, _ = oracle_frame(o, s, TC.BASE, w, h, n, VC.SEED)
        for it in (1, 3, 5):
            for demod in (False, True):
                kw = dict(iterations=it, demodulate=demod, light_materials=lights)
                r64, _, v64 = V.variance_guided(acc, n, g, **kw)
                r32, _, v32 = V.variance_guided(acc, n, g, dtype=np.float32, **kw)
                note("variance", v32, v64)
                note("output", r32, r64)
    # the temporal sequence, both runs from the float64 run's colour history (the device tests hand every frame the device's own)
    for mhf in VC.MIN_HISTORY:
        m64, m32 = V.VarianceGuided(), V.VarianceGuided()
        tainted = np.zeros((VC.H, VC.W), bool)
        for k, (name, n) in enumerate(VC.SEQUENCE):
            view = TC.BASE if name == "base" else TC.MOVES[name]
            acc, g, cam = oracle_frame(o, s, view, VC.W, VC.H, n, VC.SEED + k)
            kw = dict(height=VC.H, light_materials=lights, view_dependent_materials=vd, temporal=True, min_history_frames=mhf)
            prev_cam = m64.camera if m64.history is not None else cam
            r64, _ = m64.frame(acc, n, g, cam, **kw)
            r32, _ = m32.frame(acc, n, g, cam, dtype=np.float32, **kw)
            diff = (m64.taps != m32.taps) | (m64.used_temporal != m32.used_temporal)
            tainted = diff | VC.carried(tainted, g, prev_cam, cam, VC.H, m64.taps)
            print(f"{which} min_history_frames {mhf} frame {k}: {int(diff.sum())} pixels decided differently, {int(tainted.sum())} left out, "
                  f"{float(m64.used_temporal.mean()):.1%} take var_t")
            assert tainted.mean() <= VC.CAP + diff.mean()
            assert np.all(m64.used_temporal == (k >= VC.FIRST_TEMPORAL[mhf])) if name == "base" else 0.2 < m64.used_temporal.mean() < 1.0
            keep = ~tainted
            note("variance", m32.var, m64.var, keep)
            note("history", m32.history, m64.history, keep)
            if not tainted.any():
                note("output", r32, r64)
            m32.history = m64.history.copy()
    print(f"{which}: float32 against float64, in units of max(1, |ref|): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= VC.DEV32
