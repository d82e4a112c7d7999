"""Interpolated vertex normals on the device (cgpt_scene_update_smooth_normals, shade_device.hpp: get_hit<COUNT, SMOOTH>)
against the model of tests/smooth_ref.py: the guide normal of an icosphere with radial normals against normalize(x - c), a faceted mesh
with the flag on against the flag off to the bit, the three render paths against each other to the bit on a smooth scene, the radiance
of a tilted floor against its closed form, the refit, and the refusals and state rules of the call."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import integrator_ref as R
import smooth_ref as S

pytestmark = pytest.mark.gpu

KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT)
GW = GH = 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flags_ptr(flags):
    return flags.ctypes.data_as(C.POINTER(C.c_uint32))


# ---- the icosphere scene of checks 1, 5 and 6 ------------------------------------------------------------------------------------------------
def _ball_scene(smooth=False, center=S.SPHERE_CENTER, radius=S.SPHERE_RADIUS):
    """(scene, ball object index, lamp object index): the level-1 icosphere with radial normals and a sphere light behind the camera."""
    s = P.Scene()
    diffuse = s.add_material(P.Material(albedo=(0.8, 0.7, 0.6)))
    emitter = s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=20.0, is_light=True))
    ball = s.add_mesh(P.Mesh.from_arrays(*S.icosphere(S.SPHERE_LEVEL, center, radius)), diffuse, smooth=smooth)
    lamp = s.add_sphere((6.0, 8.0, 6.0), 1.0, emitter)
    s.add_light(lamp)
    s.set_camera(*S.SPHERE_CAMERA, GW / GH)
    return s, ball, lamp


def _guides(r):
    if r.width != GW or r.num_accumulated == 0:
        r.render(GW, GH, 1)                                       # the guides are those of the rendered frame
    return r.guides().copy()


def _triangle_of(rows, x):
    """The triangle of `rows` that holds each x (n, 3): the largest smallest barycentric coordinate among those whose plane x lies in.
    Across an edge the interpolated normal is continuous, so a point on one is served by either side."""
    t = rows.astype(np.float64)
    p0, e1, e2 = t[:, 0:3], t[:, 6:9] - t[:, 0:3], t[:, 12:15] - t[:, 0:3]
    g = np.cross(e1, e2)
    gg = np.sum(g * g, -1)
    w = x[:, None, :].astype(np.float64) - p0[None]
    u = np.sum(np.cross(w, e2[None]) * g[None], -1) / gg
    v = np.sum(np.cross(e1[None], w) * g[None], -1) / gg
    off_plane = np.abs(np.sum(w * g[None], -1)) / np.sqrt(gg)
    inside = np.minimum(np.minimum(u, v), 1.0 - u - v)
    inside = np.where(off_plane < 1e-4, inside, -np.inf)
    tri = np.argmax(inside, 1)
    assert np.all(inside[np.arange(x.shape[0]), tri] > -1e-4), "a guide position lies on no triangle"
    return tri


def _compare_guides(g, ball, rows, center, who):
    """Check 1 on one guide buffer.  Returns (largest deviation on the compared pixels, share of excluded pixels)."""
    hit = g[..., 7].view(np.uint32) == ball
    assert hit.sum() > 500, who
    x, n = g[..., 0:3][hit], g[..., 4:7][hit].astype(np.float64)
    tri = _triangle_of(rows, x)
    ns, rule, radial, geo, keep = S.sphere_guide_model(rows, tri, x, S.SPHERE_CAMERA[0], center)
    excluded = 1.0 - keep.mean()
    worst = np.abs(n[keep] - radial[keep]).max()
    fallback = rule == S.GEOMETRIC
    d = x.astype(np.float64) - S.SPHERE_CAMERA[0]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    grazing = (np.abs(np.sum(d * ns, -1)) < S.GRAZING) | (np.abs(np.sum(d * geo, -1)) < S.GRAZING) | (np.abs(np.sum(d * radial, -1)) < S.GRAZING)
    to_geo, to_radial = np.abs(n - geo).max(-1), np.abs(n - radial).max(-1)
    print(f"{who}: {hit.sum()} hit pixels, excluded {excluded:.4f} ({fallback.sum()} fallback), max |n - normalize(x - c)| = {worst:.3e}, "
          f"fallback max |n - g| = {to_geo[fallback & ~grazing].max() if np.any(fallback & ~grazing) else 0.0:.3e}")
    return worst, excluded, (fallback, grazing, to_geo, to_radial)


def _assert_smooth_guides(g, ball, rows, center, who):
    worst, excluded, (fallback, grazing, to_geo, to_radial) = _compare_guides(g, ball, rows, center, who)
    assert excluded <= S.MAX_EXCLUDED, (who, excluded)
    assert worst <= S.GUIDE_BOUND, (who, worst)
    assert np.any(fallback), who
    assert np.all(to_geo[fallback & ~grazing] <= S.GUIDE_BOUND), who            # the geometric normal, on the outward side
    either = np.minimum(to_geo, to_radial)[fallback & grazing]                  # float32 may decide a grazing pixel the other way
    assert np.all(either <= S.GUIDE_BOUND), who


# ---- 1. guides against the closed form -----------------------------------------------------------------------------------------------------
def test_guide_normal_is_the_radial_direction():
    """Device maximum on this scene: see the printed figure (DESIGN.md 5.14 records it)."""
    rows = S.triangle_rows(S.icosphere(S.SPHERE_LEVEL, S.SPHERE_CENTER, S.SPHERE_RADIUS))
    s, ball, _ = _ball_scene(smooth=True)
    r = P.Renderer(0)
    try:
        r.upload(s)                                                # sends the scene's flags
        _assert_smooth_guides(_guides(r), ball, rows, S.SPHERE_CENTER, "flag on")
        r.update_smooth_normals(np.zeros(2, np.uint32))
        worst, _, _ = _compare_guides(_guides(r), ball, rows, S.SPHERE_CENTER, "flag off")
        assert worst > 0.1, "with the flag off the guide normal is the flat v0.normal: this comparison must fail by a wide margin"
    finally:
        r.close(); s.close()


# ---- 2 and 3: the material scenes ----------------------------------------------------------------------------------------------------------
DIFFUSE = dict(albedo=(0.8, 0.6, 0.3))
MIRROR = dict(albedo=(0.9, 0.9, 0.9), specular=1.0)
GGX = dict(albedo=(0.9, 0.8, 0.6), specular=0.8, roughness=0.3)
GLASS = dict(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517)
ROUGH_GLASS = dict(GLASS, transmission_roughness=0.3)


def _material_scene(materials, faceted, smooth, settings=None, aspect=1.0):
    """A row of level-1 icospheres, one per material, over a diffuse ground plane under one sphere light."""
    s = P.Scene()
    ground = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=12.0, is_light=True))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), ground)
    lamp = s.add_sphere((0.5, 5.0, 2.0), 1.5, emitter)
    s.add_light(lamp)
    n = len(materials)
    balls = []
    for k, m in enumerate(materials):
        mat = s.add_material(P.Material(**m))
        mesh = S.icosphere(1, (2.1 * (k - (n - 1) / 2.0), 0.0, -1.0), 0.95, faceted=faceted)
        balls.append(s.add_mesh(P.Mesh.from_arrays(*mesh), mat, smooth=smooth))
    s.set_camera((0.3, 1.6, 5.5), (0.0, -0.25, -1.0), 60.0, aspect)
    if settings is not None:
        s.set_settings(settings)
    return s, balls


def _render(s, W, H, spp, kernel, settings=None, counters=False, M=1):
    r = P.Renderer(0)
    try:
        if M > 1:
            r.set_nee_candidates(M)
        r.upload(s)
        r.render(W, H, spp, kernel=kernel, settings=settings, counters=counters)
        return r.accumulator().copy(), r.stats().traced_rays
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["ADVANCED", "BRUTE_FORCE"])
def test_faceted_mesh_renders_the_same_with_the_flag_on(mode):
    """Three equal normals per triangle: step 1 of the rule returns n0, so lobe level 3 (the flag on) computes what level 2 computes."""
    st = P.Settings(render_mode=getattr(P, "MODE_" + mode))
    materials = (DIFFUSE, MIRROR, GLASS, ROUGH_GLASS)
    off, _ = _material_scene(materials, faceted=True, smooth=False, settings=st)
    on, _ = _material_scene(materials, faceted=True, smooth=True, settings=st)
    assert on.smooth_normals().sum() == 4 and not off.smooth_normals().any()
    for kernel in KERNELS:
        a, rays_a = _render(off, 32, 32, 4, kernel, st)
        b, rays_b = _render(on, 32, 32, 4, kernel, st)
        assert a[..., :3].any()
        assert np.array_equal(_bits(a), _bits(b)) and rays_a == rays_b, (mode, kernel)
    off.close(); on.close()


@pytest.mark.parametrize("config", ["nee", "no_nee", "ris4"])
def test_render_paths_agree_to_the_bit_on_a_smooth_scene(config):
    st = P.Settings(next_event_estimation_enabled=config != "no_nee")
    materials = (DIFFUSE, MIRROR, GGX, GLASS)
    s, _ = _material_scene(materials, faceted=False, smooth=True, settings=st)
    flat, _ = _material_scene(materials, faceted=False, smooth=False, settings=st)
    M = 4 if config == "ris4" else 1
    for counters in (False, True):
        frames = [_render(s, 48, 48, 8, k, st, counters, M) for k in KERNELS]
        for k, (acc, rays) in zip(KERNELS, frames):
            assert np.array_equal(_bits(acc), _bits(frames[0][0])) and rays == frames[0][1], (config, counters, k)
        assert frames[0][0][..., :3].any()
        if not counters:
            plain = frames[0][0]
    assert np.array_equal(_bits(plain), _bits(frames[0][0])), "the counters change the image"
    assert not np.array_equal(_bits(plain), _bits(_render(flat, 48, 48, 8, KERNELS[0], st, False, M)[0])), "the smooth scene renders as the flat one"
    s.close(); flat.close()


# ---- 4. closed-form radiance ---------------------------------------------------------------------------------------------------------------
_radiance = {}


def _radiance_case():
    if not _radiance:
        _radiance["case"], _radiance["flat"] = S.radiance_case()
    return _radiance["case"], _radiance["flat"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_radiance_of_the_tilted_floor_matches_the_closed_form(kernel):
    """a L r^2 cos(ns(x), c^) / D^2 under Case.check (5 sigma + 1e-3, 16 bins), sample count from needed_spp (2496)."""
    c, _ = _radiance_case()
    o, s = c.build()
    o.close()
    s.set_smooth_normals(0, True)
    r = P.Renderer(0)
    try:
        r.upload(s)
        origin = np.broadcast_to(np.asarray(c.camera[0], np.float32), (c.H * c.W, 3))
        t, obj, _, _ = r.intersect_rays(origin, c.rays().reshape(-1, 3).astype(np.float32))
        assert np.all(obj == c.primary_object) and np.allclose(t, c.primary_t.ravel(), rtol=1e-5)
        r.render(c.W, c.H, c.spp, seed=R.SEED, kernel=kernel, settings=c.settings())
        acc = r.accumulator().copy()
        c.check(acc, f"kernel {kernel}")
        if "first" in _radiance:
            assert np.array_equal(_bits(acc), _bits(_radiance["first"])), kernel
        _radiance.setdefault("first", acc)
        if kernel == KERNELS[0]:                                   # and the test can tell: the flat normal's image fails the same rule
            r.update_smooth_normals(np.zeros(2, np.uint32))
            r.reset_accumulator()
            r.render(c.W, c.H, c.spp, seed=R.SEED, kernel=kernel, settings=c.settings())
            ratio, detail = c.worst(r.accumulator()[..., :3].astype(np.float64) / c.spp)
            print(f"flag off: worst residual / tolerance {ratio:.1f}")
            assert ratio > 1.0, detail
    finally:
        r.close(); s.close()


# ---- 5. refit ------------------------------------------------------------------------------------------------------------------------------
def test_refit_moves_the_normals_with_the_mesh():
    moved = S.icosphere(S.SPHERE_LEVEL, S.MOVED_CENTER, S.MOVED_RADIUS)
    s, ball, _ = _ball_scene(smooth=True)
    r = P.Renderer(0)
    try:
        r.upload(s)
        before = _guides(r)
        r.refit_mesh(ball, S.triangle_rows(moved))                # new positions, radial normals about the moved centre; no re-upload
        after = _guides(r)
        assert not np.array_equal(_bits(before), _bits(after))
        _assert_smooth_guides(after, ball, S.triangle_rows(moved), S.MOVED_CENTER, "refitted")
    finally:
        r.close(); s.close()


# ---- 6. refusals and state -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was():
    s, ball, lamp = _ball_scene()
    r = P.Renderer(0)
    L = r.L
    assert (ball, lamp) == (0, 1)
    on = np.array([1, 0], np.uint32)
    try:
        assert L.cgpt_scene_update_smooth_normals(None, _flags_ptr(on), 2) == N.CGPT_ERR_INVALID
        assert L.cgpt_scene_update_smooth_normals(r._ctx, _flags_ptr(on), 2) == N.CGPT_ERR_NO_SCENE
        r.upload(s)
        r.update_smooth_normals(on)
        smooth = _guides(r)
        for flags, n, what in ((None, 2, "expected 2"), (on, 1, "expected 2"), (on, 3, "expected 2"),
                               (np.array([2, 0], np.uint32), 2, "neither 0 nor 1"),
                               (np.array([0xFFFFFFFF, 0], np.uint32), 2, "neither 0 nor 1"),
                               (np.ones(2, np.uint32), 2, "is a light")):
            rc = L.cgpt_scene_update_smooth_normals(r._ctx, None if flags is None else _flags_ptr(flags), n)
            assert rc == N.CGPT_ERR_INVALID and what in L.cgpt_last_error(r._ctx).decode(), (flags, n, L.cgpt_last_error(r._ctx))
            assert np.array_equal(_bits(_guides(r)), _bits(smooth)), what
        only_lamp = np.zeros(2, np.uint32); only_lamp[lamp] = 1
        with pytest.raises(P.DeviceError, match="is a light"):
            r.update_smooth_normals(only_lamp)
        assert np.array_equal(_bits(_guides(r)), _bits(smooth))
    finally:
        r.close(); s.close()


def test_upload_resets_and_the_edits_keep_the_flags():
    s, ball, lamp = _ball_scene()                                  # the host scene holds no flag: upload() sends none
    rows = S.triangle_rows(S.icosphere(S.SPHERE_LEVEL, S.SPHERE_CENTER, S.SPHERE_RADIUS))
    on = np.zeros(2, np.uint32); on[ball] = 1
    r = P.Renderer(0)
    try:
        r.upload(s)
        flat = _guides(r)                                          # read the guides, set the flag, read them again: recomputed
        r.update_smooth_normals(on)
        smooth = _guides(r)
        hit = flat[..., 7].view(np.uint32) == ball
        assert np.array_equal(_bits(flat[..., 0:4]), _bits(smooth[..., 0:4])) and np.array_equal(_bits(flat[..., 7:]), _bits(smooth[..., 7:]))
        assert np.abs(flat[..., 4:7][hit] - smooth[..., 4:7][hit]).max() > 0.1
        assert np.array_equal(_bits(flat[..., 4:7][~hit]), _bits(smooth[..., 4:7][~hit]))
        _assert_smooth_guides(smooth, ball, rows, S.SPHERE_CENTER, "flag set after the upload")

        s.set_material(0, P.Material(albedo=(0.8, 0.7, 0.6), specular=0.5, roughness=0.4))
        r.update_materials(s)                                      # materials and roughness: the flags stay
        kept = _guides(r)
        assert np.array_equal(_bits(kept[..., 4:7]), _bits(smooth[..., 4:7]))
        r.update_primitive(lamp, 1, center=(6.0, 8.5, 6.0), radius=1.0)          # a primitive edit re-sends the object record
        assert np.array_equal(_bits(_guides(r)[..., 4:7]), _bits(smooth[..., 4:7]))
        r.refit_mesh(ball, rows)                                   # and so does a refit (the same triangles)
        assert np.array_equal(_bits(_guides(r)[..., 4:7]), _bits(smooth[..., 4:7]))

        s.set_material(0, P.Material(albedo=(0.8, 0.7, 0.6)))
        r.upload(s)                                                # an upload resets every flag
        assert np.array_equal(_bits(_guides(r)), _bits(flat))
        s.set_smooth_normals(ball, True)                           # and upload() sends the scene's own
        r.upload(s)
        assert np.array_equal(_bits(_guides(r)[..., 4:7]), _bits(smooth[..., 4:7]))
    finally:
        r.close(); s.close()


def test_two_rank_context_renders_the_smooth_scene_bit_identically():
    st = P.Settings()
    s, _ = _material_scene((DIFFUSE, MIRROR, GGX, GLASS), faceted=False, smooth=True, settings=st)
    flat, _ = _material_scene((DIFFUSE, MIRROR, GGX, GLASS), faceted=False, smooth=False, settings=st)
    W, H, spp = 48, 40, 6
    single, _ = _render(s, W, H, spp, P.KERNEL_AUTO, st)
    flat_acc, _ = _render(flat, W, H, spp, P.KERNEL_AUTO, st)
    assert not np.array_equal(_bits(single), _bits(flat_acc))
    g = P.Renderer([0, 0], flags=P.CTX_GATHER_PEER_COPY)
    try:
        g.upload(s)                                                # every member gets the flags
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(single))
        lights = np.ones(s.flatten().n_objects, np.uint32)         # a refusal reaches the caller and changes no member
        assert g.L.cgpt_scene_update_smooth_normals(g._ctx, _flags_ptr(lights), lights.size) == N.CGPT_ERR_INVALID
        g.reset_accumulator()
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(single))
        g.update_smooth_normals(np.zeros(lights.size, np.uint32))
        g.reset_accumulator()
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(flat_acc))
    finally:
        g.close(); s.close(); flat.close()
