"""The rough specular lobe on the device (cgpt_scene_update_roughness, shade_device.hpp: ggx_sample): a white-furnace check
of the estimator against the numpy statement (glossy_ref.py), bit-identity across the three render paths, roughness 0 as the mirror,
integrator agreement, the near-mirror limit, the multi-device context, checkpoint / resume and the refusals of the call."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import glossy_ref as G
from scenes import MAT_SPEC_DIFFUSE, reference_layout_pair, standin_mesh

pytestmark = pytest.mark.gpu

FLOOR_ALBEDO = (0.9, 0.7, 0.5)
KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT, P.KERNEL_AUTO)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. furnace: a glossy floor under an emissive ceiling, every primary ray on the floor ----------------------------------------
def _furnace_scene(roughness):
    s = P.Scene()
    s.add_material(P.Material(albedo=FLOOR_ALBEDO, specular=1.0, roughness=roughness))
    s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=1.0, is_light=True))
    s.add_plane((0, 1, 0), (0, 0, 0), 0)
    s.add_plane((0, -1, 0), (0, 4, 0), 1)                 # not in the light list: reached by the glossy bounce only
    return s


def _furnace_camera():
    cam = N.Camera()
    for name, v in (("pos", (0.0, 1.0, 0.0)), ("top_left", (-2.0, 0.0, -10.0)), ("top_right", (2.0, 0.0, -10.0)), ("bottom_left", (-2.0, 0.0, -0.3))):
        arr = getattr(cam, name)
        for k in range(3):
            arr[k] = v[k]
    return cam


@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_BRUTE_FORCE])
def test_furnace_matches_the_directional_albedo(mode):
    W = H = 256
    spp = 256
    cam = _furnace_camera()
    st = P.Settings(russian_roulette_enabled=False, next_event_estimation_enabled=True, render_mode=mode)
    r = P.Renderer(0)
    try:
        for rough in (0.1, 0.3, 0.6, 1.0):
            r.upload(_furnace_scene(rough))
            r.reset_accumulator()
            r.render(W, H, spp, seed=0x2468ACE, settings=st, camera=cam)
            img = r.accumulator()[..., :3].astype(np.float64) / spp
            g = r.guides(camera=cam)
            pos = g[..., 0:3].astype(np.float64)
            assert np.all(_bits(g[..., 7]) != 0xFFFFFFFF), "every primary ray must hit the floor"
            to_eye = np.array([0.0, 1.0, 0.0]) - pos
            cos_o = to_eye[..., 1] / np.linalg.norm(to_eye, axis=-1)
            assert cos_o.min() > 0.05 and cos_o.max() < 0.97
            a = G.alpha_of(rough)
            nodes = np.linspace(cos_o.min() - 1e-4, cos_o.max() + 1e-4, 40)
            table = np.array([G.directional_albedo(c, a, n_s=4096, n_phi=256) for c in nodes])
            want_r = np.interp(cos_o, nodes, table)
            edges = np.quantile(cos_o, np.linspace(0, 1, 17))
            which = np.clip(np.searchsorted(edges, cos_o, side="right") - 1, 0, 15)
            for ch in range(3):
                resid = img[..., ch] - FLOOR_ALBEDO[ch] * want_r
                for b in range(16):
                    sel = resid[which == b]
                    se = sel.std() / np.sqrt(sel.size)
                    tol = 5.0 * se + 1e-3 * FLOOR_ALBEDO[ch]
                    assert abs(sel.mean()) < tol, (mode, rough, ch, b, float(sel.mean()), float(tol), float(cos_o[which == b].mean()))
    finally:
        r.close()


# ---- 2. the render paths agree to the bit ------------------------------------------------------------------------------------------
def _glossy_layout(mesh_material=4, ground_rough=0.3, mesh_rough=0.7, aspect=1.0, settings=None, level=2):
    v, i = standin_mesh(level)
    _, s = reference_layout_pair(v, i, mesh_material, aspect=aspect, extra_materials=(MAT_SPEC_DIFFUSE,), settings=settings)
    s.set_material(1, P.Material(albedo=(1.0, 1.0, 1.0), specular=0.5, roughness=ground_rough))
    s.set_roughness(4, mesh_rough)
    return s


def _render_all(s, W, H, spp, kernels=KERNELS, first=0, counters=False, rows=None, interleave=None, knobs=None, seed=0x1357, settings=None):
    out = {}
    for k in kernels:
        r = P.Renderer(0)
        r.upload(s)
        if knobs and k in knobs:
            r.set_tuning(**knobs[k])
        if first:
            r.render(W, H, first, seed=seed, kernel=P.KERNEL_PERSISTENT, rows=rows, interleave=interleave, settings=settings)
        r.render(W, H, spp, seed=seed, kernel=k, counters=counters, rows=rows, interleave=interleave, settings=settings)
        out[k] = (r.accumulator().copy(), r.pixels().copy(), r.stats().traced_rays)
        r.close()
    return out


def _assert_same(out, what):
    ref = out[KERNELS[0]] if KERNELS[0] in out else next(iter(out.values()))
    for k, (acc, px, rays) in out.items():
        assert np.array_equal(_bits(acc), _bits(ref[0])), (what, k)
        assert np.array_equal(px, ref[1]) and rays == ref[2], (what, k)
    if "view" not in what:                                   # (a debug view writes the pixels only)
        assert ref[0][..., :3].any(), what


@pytest.mark.parametrize("mesh_material", [4, 3])
def test_kernels_agree_to_the_bit(mesh_material):
    W, H = 67, 45
    cases = []
    for mode in (P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON):
        for nee, rr in ((True, True), (False, False), (True, False)):
            cases.append(P.Settings(render_mode=mode, next_event_estimation_enabled=nee, russian_roulette_enabled=rr))
    for st in cases:
        s = _glossy_layout(mesh_material, aspect=W / H, settings=st)
        _assert_same(_render_all(s, W, H, 5, settings=st), f"mat {mesh_material} mode {st.render_mode} nee {st.next_event_estimation_enabled} rr {st.russian_roulette_enabled}")
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    s = _glossy_layout(mesh_material, aspect=W / H, settings=st)
    _assert_same(_render_all(s, W, H, 4, counters=True, settings=st), "counters")
    _assert_same(_render_all(s, W, H, 3, rows=(7, 30), settings=st), "band")
    _assert_same(_render_all(s, W, H, 3, interleave=(4, 3, 1), settings=st), "interleave")
    _assert_same(_render_all(s, W, H, 3, first=5, settings=st), "first_sample")
    _assert_same(_render_all(s, W, H, 9, knobs={P.KERNEL_WAVEFRONT: {"batch": 2, "pools": 2}}, settings=st), "several wavefront batches")
    _assert_same(_render_all(s, W, H, 1, settings=P.Settings(debug_render_mode=P.DEBUG_RAY_DEPTH)), "ray-depth view")


def test_fuzz_with_roughness():
    rng = np.random.default_rng(11)
    for case in range(8):
        W, H = int(rng.integers(9, 140)), int(rng.integers(5, 90))
        spp = int(rng.choice([1, 2, 5, 17]))
        mode = int(rng.choice([P.MODE_ADVANCED, P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON]))
        st = P.Settings(max_ray_depth=int(rng.choice([1, 3, 5, 7])), next_event_estimation_enabled=bool(rng.random() < 0.7),
                        cosine_weighted_diffuse_reflection_enabled=bool(rng.random() < 0.7), russian_roulette_enabled=bool(rng.random() < 0.6),
                        render_mode=mode)
        mat = int(rng.choice([0, 3, 4]))
        s = _glossy_layout(mat, float(rng.choice([0.0, 0.05, 0.5, 1.0])), float(rng.choice([0.0, 0.2, 0.9])), aspect=W / H, settings=st,
                           level=int(rng.choice([1, 2, 3])))
        s.set_roughness(0, float(rng.random()))
        _assert_same(_render_all(s, W, H, spp, seed=int(rng.integers(0, 2 ** 31)), first=int(rng.choice([0, 0, 3])), settings=st),
                     f"fuzz case {case}: {W}x{H} spp {spp} mode {mode} mat {mat} roughness {s.roughness().tolist()}")


# ---- 3. roughness 0 is the mirror, bit for bit --------------------------------------------------------------------------------------
def test_roughness_zero_is_todays_image():
    W, H, spp = 64, 48, 4
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    s = _glossy_layout(4, 0.0, 0.0, aspect=W / H, settings=st)
    n = s.flatten().n_materials
    for k in (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT):
        r = P.Renderer(0)
        r.upload(s)
        r.render(W, H, spp, kernel=k)
        plain = r.accumulator().copy()
        r.reset_accumulator()
        r.update_roughness(np.zeros(n, np.float32))
        r.render(W, H, spp, kernel=k)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), k
        r.reset_accumulator()
        rough = np.zeros(n, np.float32); rough[1] = 0.5; rough[4] = 0.5
        r.update_roughness(rough)
        r.render(W, H, spp, kernel=k)
        assert not np.array_equal(_bits(r.accumulator()), _bits(plain)), k
        r.reset_accumulator()
        r.update_roughness(np.zeros(n, np.float32))
        r.render(W, H, spp, kernel=k)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), k
        # upload resets roughness; update_materials keeps it
        r.update_roughness(rough)
        desc = s.flatten()
        assert r.L.cgpt_scene_upload(r._ctx, C.byref(desc)) == N.CGPT_OK
        r.reset_accumulator()
        r.render(W, H, spp, kernel=k)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), k
        r.update_roughness(rough)
        r.reset_accumulator()
        r.render(W, H, spp, kernel=k)
        glossy = r.accumulator().copy()
        r.reset_accumulator()
        desc = s.flatten()
        assert r.L.cgpt_scene_update_materials(r._ctx, desc.materials, desc.n_materials) == N.CGPT_OK
        r.render(W, H, spp, kernel=k)
        assert np.array_equal(_bits(r.accumulator()), _bits(glossy)), k
        r.close()


# ---- 4. / 5. integrators agree; the near-mirror limit ---------------------------------------------------------------------------
def _mean_image(s, W, H, spp, mode, seed=99):
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, spp, seed=seed, settings=P.Settings(render_mode=mode, russian_roulette_enabled=False))
    img = r.accumulator()[..., :3].astype(np.float64) / spp
    r.close()
    return img


def _blocks(img, b=8):
    H, W = img.shape[:2]
    return img[:H - H % b, :W - W % b].reshape(H // b, b, W // b, b, 3).transpose(0, 2, 1, 3, 4).reshape(H // b, W // b, b * b, 3)


def test_advanced_with_nee_and_brute_force_converge_to_the_same_image():
    """The reference layout with a purely glossy ground (specular 1, roughness 0.3) and a glossy mesh (specular 1, roughness 0.7).  No
    diffuse lobe: the two integrators' diffuse estimators differ on purpose (the reference's swapped pdfs, SURVEY A-7), the glossy one must
    not.  With NEE on, a light reached by a glossy bounce counts only because the bounce sets is_specular."""
    W, H, spp = 96, 64, 1024
    s = _glossy_layout(4, 0.3, 0.7, aspect=W / H)
    s.set_material(1, P.Material(albedo=(1.0, 1.0, 1.0), specular=1.0, roughness=0.3))
    s.set_material(4, P.Material(albedo=(0.8, 0.6, 0.2), specular=1.0, roughness=0.7))
    adv, brute = (_blocks(_mean_image(s, W, H, spp, m)) for m in (P.MODE_ADVANCED, P.MODE_BRUTE_FORCE))
    # the standard error of a block mean from the spread of its 64 pixel means (an over-estimate where the image varies inside a block)
    se = np.sqrt(adv.var(axis=2) + brute.var(axis=2)) / np.sqrt(adv.shape[2])
    d = np.abs(adv.mean(axis=2) - brute.mean(axis=2))
    assert np.all(d < 4.0 * se + 1e-3), (float(np.max(d - 4.0 * se)), np.argwhere(d >= 4.0 * se + 1e-3)[:5].tolist())
    assert abs(adv.mean() - brute.mean()) < 0.01 * brute.mean(), (adv.mean(), brute.mean())
    assert brute.mean() > 0.05


def test_rmse_against_the_mirror_falls_with_roughness():
    W, H, spp = 96, 64, 4096
    ref = _mean_image(_glossy_layout(4, 0.0, 0.0, aspect=W / H), W, H, spp, P.MODE_ADVANCED)
    err = []
    for rough in (0.02, 0.1, 0.3):
        img = _mean_image(_glossy_layout(4, rough, rough, aspect=W / H), W, H, spp, P.MODE_ADVANCED)
        err.append(float(np.sqrt(np.mean((img - ref) ** 2))))
    assert err[0] < err[1] < err[2], err


# ---- 6. multi-device context and checkpoint / resume -------------------------------------------------------------------------------
def test_multi_device_and_resume_are_bit_identical():
    W, H, spp = 70, 41, 6
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    s = _glossy_layout(4, aspect=W / H, settings=st)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, spp)
    single = r.accumulator().copy()
    r.close()
    for ranks in (2, 3):
        g = P.Renderer([0] * ranks, flags=P.CTX_GATHER_PEER_COPY)
        g.upload(s)
        g.render(W, H, spp // 2)
        g.render(W, H, spp - spp // 2)
        assert np.array_equal(_bits(g.accumulator()), _bits(single)), ranks
        g.reset_accumulator()
        g.render(W, H, 2)
        saved = g.accumulator().copy()
        g.close()
        b = P.Renderer([0] * (5 - ranks), flags=P.CTX_GATHER_PEER_COPY)
        b.upload(s)
        b.load_accumulator(saved, 2, W, H)
        b.render(W, H, spp - 2)
        assert np.array_equal(_bits(b.accumulator()), _bits(single)), ranks
        # the group's roughness: back to 0 on every member gives the mirror frame
        b.update_roughness(np.zeros(s.flatten().n_materials, np.float32))
        b.reset_accumulator()
        b.render(W, H, spp)
        assert not np.array_equal(_bits(b.accumulator()), _bits(single))
        b.close()
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, 2)
    r2 = P.Renderer(0)
    r2.upload(s)
    r2.load_accumulator(r.accumulator().copy(), 2, W, H)
    r2.render(W, H, spp - 2)
    assert np.array_equal(_bits(r2.accumulator()), _bits(single))
    r.close(); r2.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    W, H, spp = 40, 30, 3
    r = P.Renderer(0)
    fp = C.POINTER(C.c_float)
    v = np.full(5, 0.5, np.float32)
    assert r.L.cgpt_scene_update_roughness(r._ctx, v.ctypes.data_as(fp), 5) == N.CGPT_ERR_NO_SCENE
    s = _glossy_layout(4, aspect=W / H)
    r.upload(s)
    n = s.flatten().n_materials
    r.render(W, H, spp)
    want = r.accumulator().copy()
    bad = [np.full(n - 1, 0.5, np.float32), np.full(n + 1, 0.5, np.float32)]
    for val in (np.nan, -0.1, 1.5, np.inf):
        x = np.zeros(n, np.float32); x[2] = val; bad.append(x)
    for x in bad:
        assert r.L.cgpt_scene_update_roughness(r._ctx, x.ctypes.data_as(fp), x.size) == N.CGPT_ERR_INVALID, x
    assert r.L.cgpt_scene_update_roughness(r._ctx, None, n) == N.CGPT_ERR_INVALID
    r.reset_accumulator()
    r.render(W, H, spp)
    assert np.array_equal(_bits(r.accumulator()), _bits(want))
    r.close()
