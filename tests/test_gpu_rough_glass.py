"""The rough dielectric lobe on the device (cgpt_scene_update_transmission_roughness, shade_device.hpp: rough_glass_sample, DESIGN.md
5.11): a two-emitter furnace of one interface against the numpy statement (rough_glass_ref.py) from outside and from inside, a slab
through the wavefront trace kernel against the layered-slab simulation, bit-identity across the render paths, transmission roughness 0
as today's glass, integrator agreement, the multi-device context, checkpoint / resume, the refusals of the call and the guides."""
import ctypes as C
import functools

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import integrator_ref as I
import rough_glass_ref as RG
from scenes import MAT_SPEC_DIFFUSE, reference_layout_pair, standin_mesh

pytestmark = pytest.mark.gpu

KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT, P.KERNEL_AUTO)
IOR = 1.5
ALBEDO = np.array([0.9, 0.7, 0.5])
SIGMA = np.array([0.2, 0.5, 1.0])
L_UP, L_DOWN = np.array([1.0, 1.0, 1.0]), np.array([0.25, 0.5, 2.0])
MIXED = dict(albedo=(0.8, 0.6, 0.2), specular=0.3, roughness=0.4, refractivity=0.5, absorption=(0.2, 0.8, 0.8), ior=1.517, transmission_roughness=0.2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _camera(pos, top_left, top_right, bottom_left):
    cam = N.Camera()
    for name, v in (("pos", pos), ("top_left", top_left), ("top_right", top_right), ("bottom_left", bottom_left)):
        arr = getattr(cam, name)
        for k in range(3):
            arr[k] = v[k]
    return cam


def _pixel_dirs(cam, W, H):
    """float64 primary-ray directions of every pixel: u = px / W, v = py / H, no jitter (ref: Main.cpp:713-714)."""
    pos, tl, tr, bl = (np.array([getattr(cam, n)[k] for k in range(3)], np.float64) for n in ("pos", "top_left", "top_right", "bottom_left"))
    u = (np.arange(W) / W)[None, :, None]
    v = (np.arange(H) / H)[:, None, None]
    d = tl + u * (tr - tl) + v * (bl - tl) - pos
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- 1. furnace: one rough interface between two emitters, every primary ray on it ------------------------------------------------
def _furnace_scene(rho):
    s = P.Scene()
    s.add_material(P.Material(albedo=tuple(ALBEDO), refractivity=1.0, absorption=tuple(SIGMA), ior=IOR, transmission_roughness=rho))
    s.add_material(P.Material(emissive=tuple(L_UP), intensity=1.0, is_light=True))
    s.add_material(P.Material(emissive=tuple(L_DOWN), intensity=1.0, is_light=True))
    s.add_plane((0, 1, 0), (0, 0, 0), 0)
    s.add_plane((0, -1, 0), (0, 4, 0), 1)                 # neither emitter is in the light list: reached by the rough bounce only
    s.add_plane((0, 1, 0), (0, -4, 0), 2)
    return s


def _furnace_camera(y):
    """test_gpu_glossy.py's recipe: the screen lies in the plane y = 0 itself; y = 1 looks down at it, y = -1 up (from inside)."""
    return _camera((0.0, y, 0.0), (-2.0, 0.0, -10.0), (2.0, 0.0, -10.0), (-2.0, 0.0, -0.3))


@functools.lru_cache(maxsize=None)
def _rt_table(rho, inside, lo, hi):
    """(nodes, (n, 2) R and T) for linear interpolation in cos_o over [lo, hi]: intervals are halved until the midpoint lies within 1e-4
    of the chord (the Fresnel edge at the critical angle is sharp at a low roughness).  The 1024 x 256 grid is within 5e-5 of 8192 x 1024
    over roughness 0.1 .. 1 and cos_o 0.1 .. 0.9 from both sides (the phi count matters more than the v count), so the expected values
    carry about 1e-4 of their own, below the acceptance floor of 1e-3 of the channel's largest value."""
    a = RG.alpha_of(rho)
    etai, etat = (IOR, 1.0) if inside else (1.0, IOR)
    f = lambda c: np.array(RG.interface_rt(c, a, etai, etat, n_v=1024, n_phi=256))
    nodes = list(np.linspace(lo, hi, 17))
    vals = [f(c) for c in nodes]
    todo = [True] * (len(nodes) - 1)
    while any(todo):
        n2, v2, t2 = [nodes[0]], [vals[0]], []
        for k in range(len(nodes) - 1):
            if todo[k]:
                mid = 0.5 * (nodes[k] + nodes[k + 1])
                fm = f(mid)
                bad = bool(np.max(np.abs(fm - 0.5 * (vals[k] + vals[k + 1]))) > 1e-4) and nodes[k + 1] - nodes[k] > 1e-5
                n2 += [mid, nodes[k + 1]]; v2 += [fm, vals[k + 1]]; t2 += [bad, bad]
            else:
                n2.append(nodes[k + 1]); v2.append(vals[k + 1]); t2.append(False)
        nodes, vals, todo = n2, v2, t2
    return np.array(nodes), np.array(vals)


@pytest.mark.parametrize("inside", [False, True], ids=["from_above", "from_inside"])
@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_BRUTE_FORCE], ids=["advanced", "brute_force"])
def test_furnace_matches_reflectance_and_transmittance(mode, inside):
    """Per pixel albedo * (R L_near + T A L_far): from above L_near = L_UP, L_far = L_DOWN, no Beer; from inside (the camera below the
    plane, so dot(normal, d) > 0) L_near = L_DOWN, L_far = L_UP and A = exp(-sigma / cos_o), ray.t of the primary ray -- the Beer and
    TIR case.  Acceptance as in test_gpu_glossy.py: 16 quantile bins of cos_o, |mean residual| < 5 se + 1e-3 of the channel's largest
    expected value."""
    W = H = 128
    spp = 256
    cam = _furnace_camera(-1.0 if inside else 1.0)
    cos_o = np.abs(_pixel_dirs(cam, W, H)[..., 1])
    assert cos_o.min() > 0.05 and cos_o.max() < 0.97
    lo, hi = round(float(cos_o.min()) - 1e-3, 3), round(float(cos_o.max()) + 1e-3, 3)
    st = P.Settings(russian_roulette_enabled=False, next_event_estimation_enabled=True, render_mode=mode)
    r = P.Renderer(0)
    try:
        for rho in (0.1, 0.3, 0.6, 1.0):
            r.upload(_furnace_scene(rho))
            r.reset_accumulator()
            r.render(W, H, spp, seed=0x2468ACE, settings=st, camera=cam)
            img = r.accumulator()[..., :3].astype(np.float64) / spp
            g = r.guides(camera=cam)
            assert np.all(_bits(g[..., 7]) == 0), "every primary ray must hit the interface"
            nodes, table = _rt_table(rho, inside, lo, hi)
            R, T = np.interp(cos_o, nodes, table[:, 0]), np.interp(cos_o, nodes, table[:, 1])
            if inside:
                want = ALBEDO * (R[..., None] * L_DOWN + T[..., None] * np.exp(-SIGMA / cos_o[..., None]) * L_UP)
            else:
                want = ALBEDO * (R[..., None] * L_UP + T[..., None] * L_DOWN)
            edges = np.quantile(cos_o, np.linspace(0, 1, 17))
            which = np.clip(np.searchsorted(edges, cos_o, side="right") - 1, 0, 15)
            for ch in range(3):
                resid = img[..., ch] - want[..., ch]
                for b in range(16):
                    sel = resid[which == b]
                    se = sel.std() / np.sqrt(sel.size)
                    tol = 5.0 * se + 1e-3 * want[..., ch].max()
                    print(f"furnace mode {mode} inside {inside} rho {rho} ch {ch} bin {b:2d} cos {cos_o[which == b].mean():.3f} "
                          f"expected {want[..., ch][which == b].mean():.5f} residual {sel.mean():+.6f} tolerance {tol:.6f}")
                    assert abs(sel.mean()) < tol, (mode, inside, rho, ch, b, float(sel.mean()), float(tol), float(cos_o[which == b].mean()))
    finally:
        r.close()


# ---- 2. a slab of two rough faces through wf_trace ------------------------------------------------------------------------------------
SLAB_HALF = 20000.0        # half the faces' edge: sideways escapes of the simulation stay below 1e-4 (asserted)
SLAB_SHIFT = 3000.0        # the faces' shared diagonal lies this far (/ sqrt 2) from where the rays enter
SLAB_DEPTH = 8
SLAB_PATHS = 1_500_000


@functools.lru_cache(maxsize=None)
def _slab_simulation(rho, cos_o):
    return RG.slab(cos_o, RG.alpha_of(rho), I.K3_IOR, I.K3_ALBEDO, I.K3_SIGMA, 1.0, I.K3_LC, I.K3_LF, SLAB_DEPTH, SLAB_PATHS,
                   face_half=SLAB_HALF - SLAB_SHIFT, seed=int(1000 * rho + 100 * cos_o))


def _slab_scene(rho):
    """integrator_ref's K3 with mesh faces (the slab 0 <= y <= 1 between the emitters at y = 5 and y = -1), the faces sized for the
    simulation's escape condition."""
    s = P.Scene()
    s.add_material(P.Material(albedo=tuple(I.K3_ALBEDO), refractivity=1.0, absorption=tuple(I.K3_SIGMA), ior=I.K3_IOR, transmission_roughness=rho))
    s.add_material(P.Material(emissive=tuple(I.K3_LC), intensity=1.0, is_light=True))
    s.add_material(P.Material(emissive=tuple(I.K3_LF), intensity=1.0, is_light=True))
    x0, x1 = -SLAB_HALF + SLAB_SHIFT, SLAB_HALF + SLAB_SHIFT
    for y, ny in ((1.0, 1.0), (0.0, -1.0)):
        v, i = I.quad_mesh(y, x0, x1, -SLAB_HALF, SLAB_HALF, ny)
        s.add_mesh(P.Mesh.from_arrays(v, i), 0, P.BUILD_SAH_INTERVALS)
    s.add_plane((0, -1, 0), (0, 5, 0), 1)
    s.add_plane((0, 1, 0), (0, -1, 0), 2)
    return s


def _narrow_camera(cos_o):
    """Looks at (0, 1, 0) on the upper face from y = 4 at the incidence cos_o; the screen is small and far, so every pixel has that angle."""
    sin_o = np.sqrt(1.0 - cos_o * cos_o)
    d = np.array([sin_o, -cos_o, 0.0])
    up, right = np.array([cos_o, sin_o, 0.0]), np.array([0.0, 0.0, 1.0])
    pos = np.array([0.0, 1.0, 0.0]) - d * (3.0 / cos_o)
    c = pos + 100.0 * d
    return _camera(pos, c + 0.04 * up - 0.04 * right, c + 0.04 * up + 0.04 * right, c - 0.04 * up - 0.04 * right)


@pytest.mark.parametrize("cos_o", [0.9, 0.45])
@pytest.mark.parametrize("rho", [0.2, 0.6])
def test_slab_matches_the_layered_simulation(rho, cos_o):
    W = H = 64
    spp = 1024
    cam = _narrow_camera(cos_o)
    cos_px = -_pixel_dirs(cam, W, H)[..., 1]
    assert cos_px.max() - cos_px.min() < 2e-3 and abs(cos_px.mean() - cos_o) < 1e-3
    sim, sim_se, escaped = _slab_simulation(rho, cos_o)
    assert escaped < 1e-4, escaped
    st = P.Settings(max_ray_depth=SLAB_DEPTH, russian_roulette_enabled=False, next_event_estimation_enabled=True, render_mode=P.MODE_ADVANCED)
    r = P.Renderer(0)
    try:
        r.upload(_slab_scene(rho))
        r.render(W, H, spp, seed=0x2468ACE, settings=st, camera=cam, kernel=P.KERNEL_WAVEFRONT)
        img = r.accumulator()[..., :3].astype(np.float64) / spp
        g = r.guides(camera=cam)
        assert np.all(_bits(g[..., 7]) == 0), "every primary ray must hit the upper face"
    finally:
        r.close()
    mean = img.reshape(-1, 3).mean(axis=0)
    se = img.reshape(-1, 3).std(axis=0) / np.sqrt(W * H)
    tol = 5.0 * np.sqrt(se * se + sim_se * sim_se) + 1e-3
    print(f"slab rho {rho} cos {cos_o}: gpu {mean} simulation {sim} |d| {np.abs(mean - sim)} tolerance {tol} escaped {escaped}")
    assert np.all(np.abs(mean - sim) < tol), (rho, cos_o, mean, sim, tol)


# ---- 3. the render paths agree to the bit ----------------------------------------------------------------------------------------------
def _layout(mesh_material=3, glass_rho=0.3, aspect=1.0, settings=None, level=2):
    """The reference layout (a diffuse ground, sphere lights): material 3 is the reference's glass made rough, material 4 mixes a rough
    specular lobe, a rough dielectric lobe and a diffuse rest."""
    v, i = standin_mesh(level)
    _, s = reference_layout_pair(v, i, mesh_material, aspect=aspect, extra_materials=(MAT_SPEC_DIFFUSE,), settings=settings)
    s.set_material(4, P.Material(**MIXED))
    s.set_transmission_roughness(3, glass_rho)
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
    ref = out[KERNELS[0]]
    for k, (acc, px, rays) in out.items():
        assert np.array_equal(_bits(acc), _bits(ref[0])), (what, k)
        assert np.array_equal(px, ref[1]) and rays == ref[2], (what, k)
    if "view" not in what:                                   # (a debug view writes the pixels only)
        assert ref[0][..., :3].any(), what


@pytest.mark.parametrize("mesh_material", [3, 4])
def test_kernels_agree_to_the_bit(mesh_material):
    W, H = 67, 45
    for mode in (P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON):
        for nee, rr in ((True, True), (False, False), (True, False)):
            st = P.Settings(render_mode=mode, next_event_estimation_enabled=nee, russian_roulette_enabled=rr)
            s = _layout(mesh_material, aspect=W / H, settings=st)
            _assert_same(_render_all(s, W, H, 5, settings=st), f"mat {mesh_material} mode {mode} nee {nee} rr {rr}")
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    s = _layout(mesh_material, aspect=W / H, settings=st)
    _assert_same(_render_all(s, W, H, 4, counters=True, settings=st), "counters")
    _assert_same(_render_all(s, W, H, 3, rows=(7, 30), settings=st), "band")
    _assert_same(_render_all(s, W, H, 3, interleave=(4, 3, 1), settings=st), "interleave")
    _assert_same(_render_all(s, W, H, 3, first=5, settings=st), "first_sample")
    _assert_same(_render_all(s, W, H, 9, knobs={P.KERNEL_WAVEFRONT: {"batch": 2, "pools": 2}}, settings=st), "a short last wavefront batch")
    _assert_same(_render_all(s, W, H, 1, settings=P.Settings(debug_render_mode=P.DEBUG_RAY_DEPTH)), "ray-depth view")


def test_fuzz_with_both_roughnesses():
    rng = np.random.default_rng(13)
    for case in range(12):
        W, H = int(rng.integers(9, 140)), int(rng.integers(5, 90))
        spp = int(rng.choice([1, 2, 5, 17]))
        mode = int(rng.choice([P.MODE_ADVANCED, P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON]))
        st = P.Settings(max_ray_depth=int(rng.choice([1, 3, 5, 7])), next_event_estimation_enabled=bool(rng.random() < 0.7),
                        cosine_weighted_diffuse_reflection_enabled=bool(rng.random() < 0.7), russian_roulette_enabled=bool(rng.random() < 0.6),
                        render_mode=mode)
        mat = int(rng.choice([3, 3, 4]))
        s = _layout(mat, float(rng.choice([0.02, 0.3, 1.0])), aspect=W / H, settings=st, level=int(rng.choice([1, 2, 3])))
        n = s.flatten().n_materials
        for m in range(n):
            if rng.random() < 0.5:
                s.set_roughness(m, float(rng.random()))
            if m != 3 and rng.random() < 0.5:
                s.set_transmission_roughness(m, float(rng.random()))
        _assert_same(_render_all(s, W, H, spp, seed=int(rng.integers(0, 2 ** 31)), first=int(rng.choice([0, 0, 3])), settings=st),
                     f"fuzz case {case}: {W}x{H} spp {spp} mode {mode} mat {mat} roughness {s.roughness().tolist()} "
                     f"transmission {s.transmission_roughness().tolist()}")


# ---- 4. transmission roughness 0 is today's image, bit for bit ------------------------------------------------------------------------
def _zero_scenes(aspect, st):
    polished = _layout(3, 0.0, aspect=aspect, settings=st)                     # polished glass, no roughness anywhere
    polished.set_material(4, MAT_SPEC_DIFFUSE)
    glossy_only = _layout(3, 0.0, aspect=aspect, settings=st)                  # roughness > 0 only: lobe level 1 is still chosen
    glossy_only.set_material(4, MAT_SPEC_DIFFUSE)
    glossy_only.set_material(1, P.Material(albedo=(1.0, 1.0, 1.0), specular=0.5, roughness=0.3))
    return {"polished glass": polished, "roughness only": glossy_only}


@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_zero_is_todays_image(kernel):
    W, H, spp = 64, 48, 4
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    for name, s in _zero_scenes(W / H, st).items():
        n = s.flatten().n_materials
        r = P.Renderer(0)
        r.upload(s)
        r.render(W, H, spp, kernel=kernel)
        plain = r.accumulator().copy()
        r.reset_accumulator()
        r.update_transmission_roughness(np.zeros(n, np.float32))
        r.render(W, H, spp, kernel=kernel)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), (name, kernel)
        # nonzero values on materials without a dielectric lobe (the ground's and the blue diffuse one): lobe level 2 runs, the lobe never does
        rho = np.zeros(n, np.float32); rho[0] = 0.7; rho[1] = 0.4
        r.reset_accumulator()
        r.update_transmission_roughness(rho)
        r.render(W, H, spp, kernel=kernel)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), (name, kernel, "refractivity 0")
        # on the glass it shows, and goes away again
        rho = np.zeros(n, np.float32); rho[3] = 0.5
        r.reset_accumulator()
        r.update_transmission_roughness(rho)
        r.render(W, H, spp, kernel=kernel)
        frosted = r.accumulator().copy()
        assert not np.array_equal(_bits(frosted), _bits(plain)), (name, kernel)
        # update_materials and update_roughness keep it
        desc = s.flatten()
        assert r.L.cgpt_scene_update_materials(r._ctx, desc.materials, desc.n_materials) == N.CGPT_OK
        r.update_roughness(s.roughness(n))
        r.reset_accumulator()
        r.render(W, H, spp, kernel=kernel)
        assert np.array_equal(_bits(r.accumulator()), _bits(frosted)), (name, kernel, "kept")
        # ... and it keeps the specular lobe's roughness
        r.reset_accumulator()
        r.update_transmission_roughness(np.zeros(n, np.float32))
        r.render(W, H, spp, kernel=kernel)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), (name, kernel, "back to zero")
        # an upload resets it
        r.update_transmission_roughness(rho)
        desc = s.flatten()
        assert r.L.cgpt_scene_upload(r._ctx, C.byref(desc)) == N.CGPT_OK
        if s.roughness(n).any():
            assert r.L.cgpt_scene_update_roughness(r._ctx, s.roughness(n).ctypes.data_as(C.POINTER(C.c_float)), n) == N.CGPT_OK
        r.reset_accumulator()
        r.render(W, H, spp, kernel=kernel)
        assert np.array_equal(_bits(r.accumulator()), _bits(plain)), (name, kernel, "upload")
        r.close()


def test_roughness_leaves_the_glass_polished():
    """A material with refractivity > 0 and roughness > 0 renders polished glass: the dielectric lobe ignores `roughness`."""
    W, H, spp = 64, 48, 4
    s = _layout(3, 0.0, aspect=W / H)
    s.set_material(4, MAT_SPEC_DIFFUSE)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, spp)
    plain = r.accumulator().copy()
    s.set_roughness(3, 0.8)
    r.upload(s)
    r.reset_accumulator()
    r.render(W, H, spp)
    assert np.array_equal(_bits(r.accumulator()), _bits(plain))
    r.close()


# ---- 5. the integrators agree ----------------------------------------------------------------------------------------------------------
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
    """A purely refractive rough mesh (transmission roughness 0.5) over a mirror ground: no diffuse lobe (the two integrators' diffuse
    estimators differ on purpose, SURVEY A-7) and no smooth dielectric (its TIR differs on purpose, SURVEY A-3); the rough lobe must not
    differ.  The block-mean comparison of test_gpu_glossy.py."""
    W, H, spp = 96, 64, 1024
    s = _layout(3, 0.5, aspect=W / H)
    s.set_material(1, P.Material(albedo=(1.0, 1.0, 1.0), specular=1.0))
    adv, brute = (_blocks(_mean_image(s, W, H, spp, m)) for m in (P.MODE_ADVANCED, P.MODE_BRUTE_FORCE))
    se = np.sqrt(adv.var(axis=2) + brute.var(axis=2)) / np.sqrt(adv.shape[2])
    d = np.abs(adv.mean(axis=2) - brute.mean(axis=2))
    assert np.all(d < 4.0 * se + 1e-3), (float(np.max(d - 4.0 * se)), np.argwhere(d >= 4.0 * se + 1e-3)[:5].tolist())
    assert abs(adv.mean() - brute.mean()) < 0.01 * brute.mean(), (adv.mean(), brute.mean())
    assert brute.mean() > 0.05


# ---- 6. multi-device context and checkpoint / resume ----------------------------------------------------------------------------------
def test_multi_device_and_resume_are_bit_identical():
    W, H, spp = 70, 41, 6
    st = P.Settings(render_mode=P.MODE_COMPARISON)
    s = _layout(4, aspect=W / H, settings=st)
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
        # the group's transmission roughness: back to 0 on every member gives another frame, the one a single device gives
        zeros = np.zeros(s.flatten().n_materials, np.float32)
        b.update_transmission_roughness(zeros)
        b.reset_accumulator()
        b.render(W, H, spp)
        polished = b.accumulator().copy()
        assert not np.array_equal(_bits(polished), _bits(single))
        b.close()
        r = P.Renderer(0)
        r.upload(s)
        r.update_transmission_roughness(zeros)
        r.render(W, H, spp)
        assert np.array_equal(_bits(r.accumulator()), _bits(polished)), ranks
        r.close()
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, 2)
    r2 = P.Renderer(0)
    r2.upload(s)
    r2.load_accumulator(r.accumulator().copy(), 2, W, H)
    r2.render(W, H, spp - 2)
    assert np.array_equal(_bits(r2.accumulator()), _bits(single))
    r.close(); r2.close()


# ---- 7. / 8. refusals and the guides -----------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    W, H, spp = 40, 30, 3
    r = P.Renderer(0)
    fp = C.POINTER(C.c_float)
    v = np.full(5, 0.5, np.float32)
    assert r.L.cgpt_scene_update_transmission_roughness(r._ctx, v.ctypes.data_as(fp), 5) == N.CGPT_ERR_NO_SCENE
    s = _layout(4, aspect=W / H)
    r.upload(s)
    n = s.flatten().n_materials
    r.render(W, H, spp)
    want = r.accumulator().copy()
    bad = [np.full(n - 1, 0.5, np.float32), np.full(n + 1, 0.5, np.float32)]
    for val in (np.nan, -0.1, 1.5, np.inf, -np.inf):
        x = np.zeros(n, np.float32); x[3] = val; bad.append(x)
    for x in bad:
        assert r.L.cgpt_scene_update_transmission_roughness(r._ctx, x.ctypes.data_as(fp), x.size) == N.CGPT_ERR_INVALID, x
        assert "transmission roughness" in r.L.cgpt_last_error(r._ctx).decode()
    assert r.L.cgpt_scene_update_transmission_roughness(r._ctx, None, n) == N.CGPT_ERR_INVALID
    assert r.L.cgpt_scene_update_transmission_roughness(None, v.ctypes.data_as(fp), 5) == N.CGPT_ERR_INVALID
    r.reset_accumulator()
    r.render(W, H, spp)
    assert np.array_equal(_bits(r.accumulator()), _bits(want))
    r.close()


def test_guides_are_unchanged_by_the_call():
    W, H = 48, 36
    s = _layout(3, 0.0, aspect=W / H)
    r = P.Renderer(0)
    r.upload(s)
    r.render(W, H, 1)
    before = r.guides().copy()
    rho = np.zeros(s.flatten().n_materials, np.float32); rho[3] = 0.6
    r.update_transmission_roughness(rho)
    assert np.array_equal(_bits(r.guides()), _bits(before))
    r.reset_accumulator()
    r.render(W, H, 1)
    assert np.array_equal(_bits(r.guides()), _bits(before))
    r.close()
