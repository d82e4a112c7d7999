"""The denoiser on the device (cgpt_read_guides, cgpt_denoise; csrc/device/denoise.hip): guides against the oracle's primary hits, the
filter against its numpy statement (denoise_ref.py), invariance over render paths and multi-device contexts, no side effects, the guide
cache's invalidation, bands, refusals, and the quality it buys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V, reference_layout_pair, standin_mesh
import denoise_ref as D

pytestmark = pytest.mark.gpu

W, H = 97, 61
SEED = 0x12345678
KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT, P.KERNEL_AUTO)
DEFAULTS = (5, 4.0, 0.2, 0.3)          # iterations, sigma_color, sigma_normal, sigma_position of cgpt_denoise(params = NULL)

# an octahedron (8 triangles): the emissive lamp of the scene with every object kind
OCTA_P = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
OCTA_I = np.uint32([0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5])
TRI_P = np.float32([[-4.5, -2.5, 2.5], [-2.5, -2.5, 2.5], [-3.5, -0.5, 2.0]])
TRI_N = np.float32([0.0, 0.2, 1.0])
LAMP_MAT = P.Material(emissive=(1.0, 0.6, 0.3), intensity=6.0, is_light=True)
BIG, GROUND, LAMP, SUN, BALL, WALL, TRI = range(7)


def octahedron(center, scale):
    v = np.zeros((6, 6), np.float32)
    v[:, :3] = OCTA_P * np.float32(scale) + np.float32(center)
    v[:, 3:] = OCTA_P
    return v, OCTA_I.copy()


def all_kinds_pair(aspect):
    """meshes (the stand-in, the ground, an emissive octahedron lamp), a sphere light, a diffuse sphere, a side-wall plane and a
    stand-alone triangle -- the small objects in front of the stand-in -- in the oracle (the triangle as a one-triangle mesh: the same
    hit and normal) and in the product"""
    o, s = O.OracleScene(), P.Scene()
    for m in list(P.REFERENCE_MATERIALS) + [LAMP_MAT]:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light)
        s.add_material(m)
    v, i = standin_mesh(2)
    lv, li = octahedron((3.5, 2.0, 2.5), 0.8)
    assert o.add_mesh(v, i, 0) == s.add_mesh(P.Mesh.from_arrays(v, i), 0) == BIG
    assert o.add_mesh(GROUND_V, GROUND_I, 1) == s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), 1) == GROUND
    assert o.add_mesh(lv, li, 4) == s.add_mesh(P.Mesh.from_arrays(lv, li), 4) == LAMP
    assert o.add_sphere((10.0, 10.0, 10.0), 5.0, 2) == s.add_sphere((10.0, 10.0, 10.0), 5.0, 2) == SUN
    assert o.add_sphere((-3.5, 2.0, 2.0), 1.0, 1) == s.add_sphere((-3.5, 2.0, 2.0), 1.0, 1) == BALL
    assert o.add_plane((1.0, 0.0, 0.0), (-12.0, 0.0, 0.0), 1) == s.add_plane((1.0, 0.0, 0.0), (-12.0, 0.0, 0.0), 1) == WALL
    tv = np.zeros((3, 6), np.float32)
    tv[:, :3] = TRI_P
    tv[:, 3:] = TRI_N
    assert o.add_mesh(tv, np.uint32([0, 1, 2]), 0) == s.add_triangle(TRI_P, TRI_N, 0) == TRI
    for k in (LAMP, SUN):
        o.add_light(k)
        s.add_light(k)
    o.set_camera((0, 0, 8), (0, 0, -1), 60.0, aspect)
    s.set_camera((0, 0, 8), (0, 0, -1), 60.0, aspect)
    s.set_settings(P.Settings())
    return o, s


def light_materials(s):
    desc = s.flatten()
    return [bool(desc.materials[k].is_light) for k in range(desc.n_materials)]


def renderer(s, w=W, h=H, spp=3, kernel=P.KERNEL_AUTO, device=0, flags=0, **kw):
    r = P.Renderer(device, flags)
    r.upload(s)
    r.render(w, h, spp, seed=SEED, kernel=kernel, **kw)
    return r


def channels(px):
    return np.stack([(px >> s) & 0xFF for s in (0, 8, 16, 24)], -1).astype(np.int32)


def assert_close_to_ref(got_rgba, got_px, ref_rgba, ref_px):
    tol = 1e-4 * np.maximum(1.0, np.abs(ref_rgba))
    err = np.abs(got_rgba.astype(np.float64) - ref_rgba)
    assert np.all(err <= tol), f"max excess {float(np.max(err - tol)):.3e} at {np.unravel_index(np.argmax(err - tol), err.shape)}"
    assert np.max(np.abs(channels(got_px) - channels(ref_px))) <= 1


@pytest.fixture(scope="module")
def pairs():
    return {"reference": reference_layout_pair(*standin_mesh(2), 3, aspect=W / H), "all_kinds": all_kinds_pair(W / H)}


# ---- 1. guides against the oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["reference", "all_kinds"])
def test_guides_match_the_oracle_primary_hits(pairs, which):
    o, s = pairs[which]
    r = renderer(s, spp=1)
    try:
        got = r.guides().reshape(-1, 12)
    finally:
        r.close()
    ro, rd = o.camera_rays(W, H)
    t, obj, tri, _ = o.intersect_rays(ro.reshape(-1, 3), rd.reshape(-1, 3))
    want = D.guides_from_hits(s.flatten(), ro.reshape(-1, 3), rd.reshape(-1, 3), t, obj, tri)
    gu, wu = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(gu[:, 3], t.view(np.uint32))                     # t, bit for bit (misses: 1e34)
    assert np.array_equal(gu[:, 7], obj)                                    # obj (misses: 0xFFFFFFFF)
    assert np.array_equal(gu[:, 8:12], wu[:, 8:12])                         # albedo and material, bit for bit
    hit = obj != D.NO_HIT
    assert hit.any() and (~hit).any()
    desc = s.flatten()
    kinds = np.array([desc.objects[k].kind for k in range(desc.n_objects)])
    sphere = hit & (kinds[np.minimum(obj, desc.n_objects - 1)] == N.OBJECT_SPHERE)
    flat = hit & ~sphere
    # mesh / triangle / plane normals exact (a mesh's is its hit triangle's: the oracle's tri)
    assert np.array_equal(gu[flat, 4:7], wu[flat, 4:7])
    assert np.all(np.abs(got[sphere, 4:7] - want[sphere, 4:7]) <= 1e-6)
    assert np.all(np.abs(got[:, 0:3] - want[:, 0:3]) <= 1e-6 * np.maximum(1.0, np.abs(want[:, 0:3])))
    assert np.all(got[~hit][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]] == 0)
    assert np.all(gu[~hit, 11] == D.NO_HIT)
    if which == "all_kinds":
        assert set(np.unique(obj[hit]).tolist()) >= {BIG, GROUND, LAMP, BALL, WALL, TRI}


# ---- 2. the filter against denoise_ref ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["reference", "all_kinds"])
def test_denoise_matches_the_reference_statement(pairs, which):
    _, s = pairs[which]
    r = renderer(s, spp=3)
    try:
        acc, g, raw_px = r.accumulator(), r.guides(), r.pixels()
        lights = light_materials(s)
        for it in (0, 1, 3, 5):
            for demod in (False, True):
                for sigmas in (DEFAULTS[1:], (0.7, 0.5, 2.0)):
                    rgba, px = r.denoise(it, *sigmas, demodulate=demod)
                    ref_rgba, ref_px = D.denoise(acc, 3, g, it, *sigmas, demod, lights)
                    assert_close_to_ref(rgba, px, ref_rgba, ref_px)
                    if it == 0:                                              # the identity, bit for bit
                        c = acc[..., :3] / np.float32(3)
                        assert np.array_equal(rgba[..., :3].view(np.uint32), c.view(np.uint32))
                        assert np.all(rgba[..., 3] == 1.0)
                        assert np.array_equal(px, raw_px)
    finally:
        r.close()


def test_null_params_are_the_defaults_and_either_output_may_be_null(pairs):
    _, s = pairs["reference"]
    r = renderer(s, spp=2)
    try:
        L, cam = r.L, s.camera()
        rgba = np.empty((H, W, 4), np.float32)
        px = np.empty((H, W), np.uint32)
        assert L.cgpt_denoise(r._ctx, C.byref(cam), None, rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size,
                              px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size) == 0
        want_rgba, want_px = r.denoise(*DEFAULTS, demodulate=True)
        assert np.array_equal(rgba.view(np.uint32), want_rgba.view(np.uint32)) and np.array_equal(px, want_px)
        only_px = np.empty((H, W), np.uint32)
        assert L.cgpt_denoise(r._ctx, C.byref(cam), None, None, 0, only_px.ctypes.data_as(C.POINTER(C.c_uint32)), only_px.size) == 0
        assert np.array_equal(only_px, px)
        only_rgba = np.empty((H, W, 4), np.float32)
        assert L.cgpt_denoise(r._ctx, C.byref(cam), None, only_rgba.ctypes.data_as(C.POINTER(C.c_float)), only_rgba.size, None, 0) == 0
        assert np.array_equal(only_rgba.view(np.uint32), rgba.view(np.uint32))
    finally:
        r.close()


# ---- 3. invariance ---------------------------------------------------------------------------------------------------------------

def test_same_bytes_for_every_render_path_and_device_group(pairs):
    _, s = pairs["all_kinds"]
    outs = []
    for kernel in KERNELS:
        r = renderer(s, spp=4, kernel=kernel)
        try:
            outs.append(r.denoise())
        finally:
            r.close()
    group_guides = []
    for dev, flags in (([0, 0, 0], N.CTX_GATHER_PEER_COPY), ([0], N.CTX_FORCE_COLLECTIVE)):
        r = renderer(s, spp=4, device=dev, flags=flags)
        try:
            assert r.is_group
            outs.append(r.denoise())
            group_guides.append(r.guides())
        finally:
            r.close()
    one = renderer(s, spp=1)
    try:
        for g in group_guides:
            assert np.array_equal(g.view(np.uint32), one.guides().view(np.uint32))
    finally:
        one.close()
    for rgba, px in outs[1:]:
        assert np.array_equal(rgba.view(np.uint32), outs[0][0].view(np.uint32))
        assert np.array_equal(px, outs[0][1])


# ---- 4. no side effects ------------------------------------------------------------------------------------------------------------

def stats_bytes(r):
    st = r.stats()
    return bytes(C.string_at(C.addressof(st), C.sizeof(st)))


@pytest.mark.parametrize("group", [False, True])
def test_no_side_effects(pairs, group):
    _, s = pairs["reference"]
    dev, flags = ([0, 0, 0], N.CTX_GATHER_PEER_COPY) if group else (0, 0)
    a = renderer(s, spp=3, device=dev, flags=flags, counters=True)
    b = renderer(s, spp=3, device=dev, flags=flags, counters=True)
    try:
        before = (a.accumulator().view(np.uint32).copy(), a.pixels().copy(), a.stats().num_accumulated, stats_bytes(a))
        a.denoise()
        a.guides()
        a.denoise(iterations=0)
        after = (a.accumulator().view(np.uint32).copy(), a.pixels().copy(), a.stats().num_accumulated, stats_bytes(a))
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert before[2] == after[2] == 3
        assert before[3] == after[3]
        b.accumulator()
        b.pixels()
        a.denoise()
        for r in (a, b):                                                     # a render after a denoise = one without it
            r.render(W, H, 2, seed=SEED, counters=True)
        assert np.array_equal(a.accumulator().view(np.uint32), b.accumulator().view(np.uint32))
        assert np.array_equal(a.pixels(), b.pixels())
        sa, sb = a.stats(), b.stats()
        assert (sa.traced_rays, sa.num_accumulated, sa.kernel_launches, sa.gathers) == (sb.traced_rays, sb.num_accumulated, sb.kernel_launches, sb.gathers)
    finally:
        a.close()
        b.close()


# ---- 5. cache invalidation ---------------------------------------------------------------------------------------------------------

def fresh_guides(s):
    r = renderer(s, spp=1)
    try:
        return r.guides()
    finally:
        r.close()


def test_guides_follow_scene_and_camera_edits():
    _, s = all_kinds_pair(W / H)
    r = renderer(s, spp=1)
    try:
        prev = r.guides()
        assert np.array_equal(prev.view(np.uint32), fresh_guides(s).view(np.uint32))

        def move_sphere():
            s.update_primitive(BALL, center=(-3.0, 1.6, 2.2), radius=1.1)
            r.update_primitive(BALL, 1, center=(-3.0, 1.6, 2.2), radius=1.1)

        def change_albedo():
            s.set_material(1, P.Material(albedo=(0.3, 0.9, 0.5)))
            r.update_materials(s)

        def refit():
            v, i = standin_mesh(2)
            w = v.copy()
            w[:, :3] += np.float32([0.4, 0.3, 0.0])
            tris = P.triangles_from_arrays(w, i)
            s.refit_mesh(BIG, tris)
            r.refit_mesh(BIG, tris)

        def new_camera():
            s.set_camera((0.5, 0.3, 7.0), (0.05, -0.05, -1.0), 55.0, W / H)

        for edit in (move_sphere, change_albedo, refit, new_camera):
            edit()
            got = r.guides()
            assert not np.array_equal(got.view(np.uint32), prev.view(np.uint32)), f"{edit.__name__} changed nothing on screen"
            assert np.array_equal(got.view(np.uint32), fresh_guides(s).view(np.uint32)), edit.__name__
            prev = got
    finally:
        r.close()


# ---- 6. bands ------------------------------------------------------------------------------------------------------------------------

def test_contiguous_band_is_filtered_on_its_own(pairs):
    _, s = pairs["all_kinds"]
    rows = (10, 37)
    r = renderer(s, spp=3, rows=rows)
    full = renderer(s, spp=1)
    try:
        acc, g = r.accumulator(), r.guides()
        assert acc.shape == (27, W, 4) and g.shape == (27, W, 12)
        assert np.array_equal(g.view(np.uint32), full.guides()[rows[0]:rows[1]].view(np.uint32))   # the global rows' hits
        for demod in (False, True):
            rgba, px = r.denoise(demodulate=demod)
            ref_rgba, ref_px = D.denoise(acc, 3, g, *DEFAULTS, demod, light_materials(s))
            assert_close_to_ref(rgba, px, ref_rgba, ref_px)
    finally:
        r.close()
        full.close()


def test_interleaved_band_is_refused(pairs):
    _, s = pairs["reference"]
    r = renderer(s, spp=2, interleave=(4, 2, 1))
    try:
        for call in (r.denoise, r.guides):
            with pytest.raises(P.DeviceError) as e:
                call()
            assert e.value.code == N.CGPT_ERR_INVALID
    finally:
        r.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------

def raw_calls(r, cam, params, rgba_n=None, px_n=None, guides_n=None, rgba=True, px=True):
    """(cgpt_denoise status, cgpt_read_guides status, the three output buffers) with sentinel-filled buffers of the given sizes"""
    n = r.n_rows * r.width
    rgba_n = 4 * n if rgba_n is None else rgba_n
    px_n = n if px_n is None else px_n
    guides_n = 12 * n if guides_n is None else guides_n
    fb = np.full(max(rgba_n, 1), 7.0, np.float32)
    pb = np.full(max(px_n, 1), 7, np.uint32)
    gb = np.full(max(guides_n, 1), 7.0, np.float32)
    cp = C.byref(cam) if cam is not None else None
    pp = C.byref(params) if params is not None else None
    rc_d = r.L.cgpt_denoise(r._ctx, cp, pp, fb.ctypes.data_as(C.POINTER(C.c_float)) if rgba else None, rgba_n,
                            pb.ctypes.data_as(C.POINTER(C.c_uint32)) if px else None, px_n)
    rc_g = r.L.cgpt_read_guides(r._ctx, cp, gb.ctypes.data_as(C.POINTER(C.c_float)), guides_n)
    return rc_d, rc_g, fb, pb, gb


def untouched(*bufs):
    return all(np.all(b == 7) for b in bufs)


def test_refusals_change_nothing(pairs):
    _, s = pairs["reference"]
    cam = s.camera()
    ok = N.DenoiseParams(5, N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    r = P.Renderer(0)
    try:
        r.width, r.n_rows = W, H
        rc_d, rc_g, fb, pb, gb = raw_calls(r, cam, ok)                     # no scene
        assert (rc_d, rc_g) == (N.CGPT_ERR_NO_SCENE, N.CGPT_ERR_NO_SCENE) and untouched(fb, pb, gb)
        r.upload(s)
        rc_d, rc_g, fb, pb, gb = raw_calls(r, cam, ok)                     # a scene, no band yet
        assert (rc_d, rc_g) == (N.CGPT_ERR_INVALID, N.CGPT_ERR_INVALID) and untouched(fb, pb, gb)
    finally:
        r.close()

    r = renderer(s, spp=2, counters=True)
    try:
        def state():
            return r.accumulator().view(np.uint32).copy(), r.pixels().copy(), stats_bytes(r)

        def same(a, b):
            return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]

        before = state()
        inf, nan = float("inf"), float("nan")
        for args in ((11, 1, 4.0, 0.2, 0.3), (5, 2, 4.0, 0.2, 0.3), (5, 0x80000001, 4.0, 0.2, 0.3), (5, 1, 0.0, 0.2, 0.3),
                     (5, 1, 4.0, -0.2, 0.3), (5, 1, 4.0, 0.2, nan), (5, 1, inf, 0.2, 0.3), (5, 1, 4.0, inf, 0.3)):
            rc_d, _, fb, pb, _ = raw_calls(r, cam, N.DenoiseParams(*args))
            assert rc_d == N.CGPT_ERR_INVALID and untouched(fb, pb), args
        n = W * H
        for kw in (dict(rgba_n=4 * n - 4), dict(px_n=n + 1), dict(rgba=False, px=False)):
            rc_d, _, fb, pb, _ = raw_calls(r, cam, ok, **kw)
            assert rc_d == N.CGPT_ERR_INVALID and untouched(fb, pb), kw
        _, rc_g, _, _, gb = raw_calls(r, cam, ok, guides_n=12 * n - 12)
        assert rc_g == N.CGPT_ERR_INVALID and untouched(gb)
        rc_d, rc_g, fb, pb, gb = raw_calls(r, None, ok)                    # no camera
        assert (rc_d, rc_g) == (N.CGPT_ERR_INVALID, N.CGPT_ERR_INVALID) and untouched(fb, pb, gb)
        assert same(before, state())
        rc_d, rc_g, fb, pb, gb = raw_calls(r, cam, N.DenoiseParams(10, 0, 1e-3, 1e3, 1e-6))   # the limits are accepted
        assert (rc_d, rc_g) == (0, 0) and not untouched(fb) and not untouched(pb) and not untouched(gb)
        assert same(before, state())
        r.reset_accumulator()                                               # nothing accumulated: denoise refused, guides not
        before = state()
        rc_d, rc_g, fb, pb, _ = raw_calls(r, cam, ok)
        assert (rc_d, rc_g) == (N.CGPT_ERR_INVALID, 0) and untouched(fb, pb)
        assert same(before, state())
        r.render(W, H, 1, seed=SEED, settings=P.Settings(debug_render_mode=P.DEBUG_RAY_DEPTH))   # a debug view
        before = state()
        rc_d, rc_g, fb, pb, gb = raw_calls(r, cam, ok)
        assert (rc_d, rc_g) == (N.CGPT_ERR_INVALID, N.CGPT_ERR_INVALID) and untouched(fb, pb, gb)
        assert same(before, state())
    finally:
        r.close()


def test_works_after_write_accumulator_on_a_fresh_context(pairs):
    _, s = pairs["reference"]
    a = renderer(s, spp=3)
    b = P.Renderer(0)
    try:
        b.upload(s)
        b.load_accumulator(a.accumulator(), 3, W, H)
        ra, pa = a.denoise()
        rb, pb = b.denoise()
        assert np.array_equal(ra.view(np.uint32), rb.view(np.uint32)) and np.array_equal(pa, pb)
    finally:
        a.close()
        b.close()


# ---- 8. usefulness ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mat,limit", [(1, 0.5), (3, 1.0)])
def test_denoised_4spp_is_closer_to_1024spp_than_raw(mat, limit):
    """RMSE of radiance clamped to [0, 1] against a raw 1024-spp render, 160x120, default parameters: the diffuse reference layout
    (material 1) at most half the raw 4-spp error, the glass one (material 3) no worse (DESIGN.md 5.8 records the ratios)"""
    w, h = 160, 120
    _, s = reference_layout_pair(*standin_mesh(3), mat, aspect=w / h)
    ref = renderer(s, w, h, spp=1024)
    r = renderer(s, w, h, spp=4)
    try:
        want = np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64)
        raw = np.clip(r.accumulator()[..., :3] / np.float32(4), 0, 1).astype(np.float64)
        dn = np.clip(r.denoise()[0][..., :3], 0, 1).astype(np.float64)

        def rmse(a):
            return float(np.sqrt(np.mean((a - want) ** 2)))
        print(f"material {mat}: RMSE raw {rmse(raw):.4f} denoised {rmse(dn):.4f} ratio {rmse(dn) / rmse(raw):.3f}")
        assert rmse(dn) <= limit * rmse(raw)
    finally:
        ref.close()
        r.close()


# ---- 9. the example -------------------------------------------------------------------------------------------------------------

def test_example_writes_denoised_previews(tmp_path):
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    out = subprocess.run([exe, "--denoise", "64", "48", "8", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for name in ("preview_0004.ppm", "preview_0004_denoised.ppm", "preview_0008_denoised.ppm", "render.ppm", "render_denoised.ppm"):
        assert os.path.exists(tmp_path / name), name
    raw = (tmp_path / "render.ppm").read_bytes()
    dn = (tmp_path / "render_denoised.ppm").read_bytes()
    assert len(raw) == len(dn) and raw != dn
