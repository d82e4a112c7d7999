"""The numpy model of one shade_bounce call (tests/shade_ref.py) on its own, no GPU: the RNG inversion, the float64 model against the C
oracle on the reference's lobes (the only statement that is independent of the model), and what the GPU tests of test_gpu_shade_step.py
rely on: float32 and float64 take the same branch wherever the model calls a sample decided, and few samples are undecided."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import shade_cases as CASES
import shade_ref as S

WORDS = (0, 1, 0x7FFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF)
MAX_UNDECIDED = 0.02


# ---- state_with_draw -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(9))
def test_state_with_draw_round_trips(k):
    for word in WORDS:
        s = S.state_with_draw(k, word)
        for _ in range(k + 1):
            out, s = S.pcg_next(s)
        assert out == word, (k, hex(word))


def test_state_with_draw_against_the_oracles_generator():
    L = O.lib()
    for k in range(9):
        for word in WORDS:
            state = C.c_uint32(S.state_with_draw(k, word))
            for _ in range(k + 1):
                out = L.orc_pcg_next(C.byref(state))
            assert out == word, (k, hex(word))


def test_random_float_ends():
    assert S.random_float(0) == 0.0 and S.random_float(0xFFFFFF80) == 1.0 and S.random_float(0xFFFFFFFF) == 1.0
    assert S.random_float(0xFFFFFF7F) < 1.0
    L = O.lib()
    for w in WORDS + (0x80000000, 12345678):
        assert np.float32(L.orc_u32_to_float(w)) == S.random_float(w), hex(w)


# ---- the float64 model against the oracle ----------------------------------------------------------------------------------------------------------
W = H = 16
SEED = 0x2468ACE


def _oracle_scene():
    sc = S.ModelScene()
    ground = sc.material(albedo=(0.8, 0.7, 0.6))
    mirror = sc.material(albedo=(0.9, 0.9, 0.9), specular=1.0)
    glass = sc.material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517)
    light = sc.material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True)
    sc.plane((0, 1, 0), (0, 0, 0), ground)
    sc.sphere((-1.2, 1.0, -4.0), 1.0, mirror)
    sc.sphere((1.2, 1.0, -3.5), 1.0, glass)
    sc.sphere((0.0, 5.0, -3.0), 1.0, light, light=True)
    return sc


def test_float64_model_reproduces_an_oracle_render_pixel_by_pixel():
    """A 16 x 16, one-sample RNG_PIXEL_PCG render of a diffuse ground plane with a mirror sphere, a glass sphere and a sphere light (NEE,
    roulette and the cosine-weighted lobe on, depth 5), rebuilt per pixel: orc_pcg_seed seeds the pixel, orc_intersect_rays traces the
    extend and the shadow rays, the float64 model does every bounce.  At least 95 % of the pixels never pass an undecided sample; on
    those the radiance is the oracle's accumulator to 1e-4 relative + 1e-6.  The camera looks down so that most pixels see the scene and
    none sees the ground far away: a shadow ray from 30 units off that ends near the light's rim meets the light itself before or behind
    its end by float32 rounding inside the tracer (the chord there is shorter than intersect_sphere's error), which no shade model decides."""
    sc = _oracle_scene()
    st = S.settings(max_ray_depth=5, nee=True, cosine=True, rr=True)
    o = sc.oracle_scene()
    try:
        o.set_camera((0.0, 3.5, 1.5), (0.0, -0.8, -1.0), 60.0, 1.0)
        o.set_settings(5, True, True, True)
        o.render(W, H, 1, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED)
        acc = o.accumulator()[..., :3].reshape(-1, 3).astype(np.float64)
        co, cd = o.camera_rays(W, H)
        n = W * H
        ro, rd = co.reshape(-1, 3).astype(np.float64), cd.reshape(-1, 3).astype(np.float64)
        rng = np.array([o.L.orc_pcg_seed(i, 0, SEED) for i in range(n)], np.uint32)
        thr, energy = np.ones((n, 3)), np.zeros((n, 3))
        depth, spec = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        alive, undecided = np.ones(n, bool), np.zeros(n, bool)
        seen = set()
        for _ in range(64):
            idx = np.nonzero(alive)[0]
            if not idx.size:
                break
            a = S.samples(idx.size)
            a["t"], a["obj"], a["tri"], a["bvh_depth"] = o.intersect_rays(ro[idx].astype(np.float32), rd[idx].astype(np.float32))
            a["o"], a["d"], a["throughput"], a["rng"], a["depth"], a["is_specular"] = ro[idx], rd[idx], thr[idx], rng[idx], depth[idx], spec[idx]
            m = S.shade(sc, st, a, np.float64)
            seen |= set(np.unique(m["flags"]).tolist())
            undecided[idx] |= m["undecided"]
            energy[idx] += m["energy"]
            sh = (m["flags"] & S.SHADOW) != 0
            if sh.any():
                _, hit, _, _ = o.intersect_rays(m["shadow_o"][sh].astype(np.float32), m["shadow_d"][sh].astype(np.float32), m["shadow_tmax"][sh].astype(np.float32))
                free = hit == S.NO_HIT
                energy[idx[sh][free]] += m["pending"][sh][free]
            ro[idx], rd[idx], thr[idx], rng[idx], depth[idx], spec[idx] = m["o"], m["d"], m["throughput"], m["rng"], m["depth"], m["is_specular"]
            alive[idx] = (m["flags"] & S.TERMINATE) == 0
        assert not alive.any()
    finally:
        o.close()
    keep = ~undecided
    err = np.abs(energy - acc)
    rel = float((err / np.maximum(np.abs(acc), 1e-30))[keep][acc[keep] > 0].max())
    lit = float((acc.sum(1) > 0).mean())
    print(f"kept share {keep.mean():.4f}  lit pixels {lit:.3f}  largest relative error on the kept pixels {rel:.3e}  return words seen {sorted(seen)}")
    assert keep.mean() >= 0.95
    assert lit > 0.5, "most pixels must carry radiance"
    chains = {(f >> S.CHAIN_SHIFT) & 3 for f in seen}
    assert {S.CHAIN_REFLECT, S.CHAIN_REFRACT} <= chains and any(f & S.SHADOW for f in seen) and any(f & S.ENERGY for f in seen), seen
    assert np.all(err[keep] <= 1e-4 * np.abs(acc[keep]) + 1e-6)


# ---- model sanity: what the GPU tests rely on ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES.CASES))
def test_float32_and_float64_take_the_same_branch_and_few_samples_are_undecided(case):
    """Per call: every decided sample has the same discrete outputs in float32 and float64, every float of both evaluations is finite
    there, and at most 2 % of the samples are undecided (ill-conditioned ones included) -- the cap the GPU tests rely on, from the model
    alone.  A call above the cap is listed with its cause in shade_cases.CAP_EXCEPTIONS, and a listed call must still be above it."""
    for c in CASES.calls_of(case):
        e = CASES.evaluate(c)
        m64, m32 = e["m64"], e["m32"]
        decided = ~m64["undecided"]
        same = S.same_discrete(m32, m64)
        share = float((~decided).mean())
        cause = CASES.cap_exception(c["name"])
        print(f"{c['name']:36s} samples {decided.size:5d}  undecided {int((~decided).sum()):4d} = {share:.4f} (ill-conditioned {int(m64['ill'].sum())})"
              + ("  EXCEPTION" if cause else "") + "  " + "  ".join(f"{g} {e['tol'][g]:.2e}" for g in S.GROUPS))
        assert np.all(same[decided]), (c["name"], np.nonzero(~same & decided)[0][:8])
        for m in (m64, m32):
            for g in S.GROUPS:
                for f in S.FLOATS[g]:
                    assert np.all(np.isfinite(m[f][decided])), (c["name"], f)
        if cause is None:
            assert share <= MAX_UNDECIDED, (c["name"], share)
        else:
            assert share > MAX_UNDECIDED, (c["name"], "is listed as an exception and needs none", share)


def test_the_reservoir_is_ris_refs_on_common_candidates():
    """shade_ref.Reservoir (given draws, either float type) and ris_ref.Reservoir (float64, the statistical model's) fed the same 32
    candidates -- a third of them weightless, the draws 0 and 1.0f among them: the same takes, the same survivor, the same estimate."""
    import ris_ref as R
    rng = np.random.default_rng(3)
    n, M = 500, 32
    mine, theirs = S.Reservoir(n, np.float64), R.Reservoir(n)
    ev = S.Eval(np.zeros(n, np.uint32), np.float64, 0)
    lit = np.ones(n, bool)
    for j in range(M):
        c = rng.random((n, 3)) * rng.choice([0.0, 1.0, 1e-3], (n, 1), p=[0.34, 0.33, 0.33])
        u = rng.random(n)
        u[::7], u[3::11] = 0.0, 1.0
        up = c.sum(1) > 0.0
        take = mine.update(ev, c, up, u, np.zeros((n, 3)), np.full(n, float(j)), lit)
        assert np.array_equal(take, theirs.update(c, np.ones(n), u)), j
    assert np.array_equal(mine.c_y, theirs.c_y) and np.array_equal(mine.w_y, theirs.w_y) and np.array_equal(mine.wsum, theirs.wsum)
    some = mine.wsum > 0
    assert some.all() and np.allclose(mine.pending(M), theirs.estimate(M), rtol=1e-14, atol=0)


def test_unfixed_lambda_is_not_a_number_where_the_horizon_rule_now_ends_the_lobe():
    """ggx_lambda(a2, z) at z = 1e-20 in float32: z * z underflows, the quotient is inf, and (1 + L) / (1 + L + L') is inf / inf.  The
    horizon rule (oz^2 < FLT_MIN: no energy) ends such a sample before the weight is formed: the model's GGX samples at that cosine
    terminate, finite."""
    with np.errstate(all="ignore"):
        z = np.float32(1e-20)
        lo = S._lambda(np.float32(0.25), z)
        assert np.isinf(lo) and np.isnan((np.float32(1.0) + lo) / (np.float32(1.0) + lo + lo))
    c = next(c for c in CASES.calls_of("ggx") if c["name"] == "ggx_r0.5_grazing")
    m = CASES.evaluate(c)["m64"]
    tiny = np.abs(c["samples"]["d"][:, 2]) == np.float32(1e-20)
    assert tiny.any() and np.all(m["flags"][tiny] == S.TERMINATE) and np.all(np.isfinite(m["throughput"][tiny]))
