"""Per-object transforms on the device (cgpt_scene_update_transforms) against the model of tests/transform_ref.py: sign-flip
transforms against the untransformed world to the bit, general affine transforms against baked geometry within the model's bounds, the
guides of a placed smooth ball against the closed form, the three render paths against each other to the bit, closed-form radiance through
transformed meshes, the state rules of the call, and a two-rank context."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import integrator_ref as R
import smooth_ref as S
import transform_ref as T
import transform_scenes as TS
from test_gpu_smooth_normals import DIFFUSE, GGX, GLASS, MIRROR, ROUGH_GLASS, _compare_guides

pytestmark = pytest.mark.gpu

KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT)
FP = C.POINTER(C.c_float)
COUNTERS = ("traced_rays", "inner_steps", "tri_tests", "bvh_depth_sum", "closest_hits")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _identity(n):
    return np.tile(T.IDENTITY, (n, 1, 1))


def _upload_flat(r, flat, matrices=None):
    """cgpt_scene_upload of an edited flattened scene into renderer r (its camera and settings stay those of r.scene), then the transforms."""
    desc, keep = flat.desc()
    r._check(r.L.cgpt_scene_upload(r._ctx, C.byref(desc)))
    del keep
    if matrices is not None:
        r.update_transforms(matrices)


def _frame(r, W, H, spp, kernel, settings=None, counters=False):
    r.reset_accumulator(); r.reset_stats()
    r.render(W, H, spp, kernel=kernel, settings=settings, counters=counters)
    st = r.stats()
    return r.accumulator().copy(), st


# ---- 1. exact: a world stored half-turned or mirrored and brought back -----------------------------------------------------------------------
MODES = {"ADVANCED": P.Settings(render_mode=P.MODE_ADVANCED), "BRUTE_FORCE": P.Settings(render_mode=P.MODE_BRUTE_FORCE),
         "COMPARISON": P.Settings(render_mode=P.MODE_COMPARISON),
         "BVH_DEPTH": P.Settings(render_mode=P.MODE_ADVANCED, debug_render_mode=P.DEBUG_BVH_DEPTH)}


@pytest.mark.parametrize("flip", ["half_turn", "mirror"])
def test_sign_flip_transforms_render_the_untransformed_world_to_the_bit(flip):
    m = T.HALF_TURN if flip == "half_turn" else T.MIRROR_Z
    s0, meshes = TS.box_world()
    flat, matrices = TS.stored_flipped(s0, meshes, m)
    r0, r1 = P.Renderer(0), P.Renderer(0)
    try:
        r0.upload(s0)
        r1.upload(s0)                                              # the camera and settings; the geometry is replaced next
        _upload_flat(r1, flat, matrices)
        for mode, st in MODES.items():
            for kernel in KERNELS:
                for counters in ((False, True) if mode == "ADVANCED" else (False,)):
                    a, sa = _frame(r0, 64, 64, 4, kernel, st, counters)
                    if mode == "BVH_DEPTH": a = r0.pixels().copy()      # a debug view writes the pixels only
                    b, sb = _frame(r1, 64, 64, 4, kernel, st, counters)
                    if mode == "BVH_DEPTH": b = r1.pixels().copy()
                    assert len(np.unique(a)) > 2 if mode == "BVH_DEPTH" else a[..., :3].any(), (mode, kernel)
                    assert np.array_equal(_bits(a), _bits(b)), (flip, mode, kernel, counters, int((_bits(a) != _bits(b)).any(-1).sum()))
                    assert sa.traced_rays == sb.traced_rays, (flip, mode, kernel, counters)
                    if counters:
                        assert [getattr(sa, c) for c in COUNTERS] == [getattr(sb, c) for c in COUNTERS], (flip, mode, kernel)
                        assert sa.inner_steps > 0 and sa.tri_tests > 0 and sa.closest_hits > 0
        # and the test can tell: without the transforms the stored world is another image
        r1.update_transforms(_identity(matrices.shape[0]))
        a, _ = _frame(r0, 64, 64, 4, KERNELS[0], MODES["ADVANCED"])
        c, _ = _frame(r1, 64, 64, 4, KERNELS[0], MODES["ADVANCED"])
        assert not np.array_equal(_bits(a), _bits(c))
    finally:
        r0.close(); r1.close(); s0.close()


def test_intersect_rays_on_a_half_turned_icosphere_returns_equal_bits():
    s0 = P.Scene()
    mat = s0.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
    ball = s0.add_mesh(P.Mesh.from_arrays(*S.icosphere(3, (0.25, -0.125, 0.5), 1.0)), mat)
    s0.set_camera((0, 0, 5), (0, 0, -1), 60.0, 1.0)
    flat, matrices = TS.stored_flipped(s0, [ball], T.HALF_TURN)
    rng = np.random.default_rng(5)
    n = 2048
    o = (rng.standard_normal((n, 3)) * 0.2 + np.array([0.25, -0.125, 0.5]) + 4.0 * np.sign(rng.standard_normal((n, 3)))).astype(np.float32)
    target = np.array([0.25, -0.125, 0.5]) + 0.7 * rng.standard_normal((n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d = d.astype(np.float32)
    # rays with exactly zero direction components: along one axis, or in one coordinate plane, through the ball
    for k in range(96):
        ax = k % 3
        o[k] = np.array([0.25, -0.125, 0.5], np.float32) + 0.5 * rng.random(3).astype(np.float32)
        if k < 48:
            d[k] = 0.0; d[k, ax] = 1.0 if k % 2 else -1.0
            o[k, ax] -= 4.0 * d[k, ax]
        else:
            d[k, ax] = 0.0
            d[k] /= np.linalg.norm(d[k])
            o[k] -= 4.0 * d[k]
    assert np.any((d == 0.0).sum(-1) == 2) and np.any((d == 0.0).sum(-1) == 1)
    r0, r1 = P.Renderer(0), P.Renderer(0)
    try:
        r0.upload(s0); r1.upload(s0)
        _upload_flat(r1, flat, matrices)
        t0, obj0, tri0, dep0 = r0.intersect_rays(o, d)
        t1, obj1, tri1, dep1 = r1.intersect_rays(o, d)
        hit = obj0 == ball
        assert 0.3 < hit.mean() < 0.99 and hit[:96].mean() > 0.5
        assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(obj0, obj1) and np.array_equal(tri0[hit], tri1[hit]) and np.array_equal(dep0, dep1)
    finally:
        r0.close(); r1.close(); s0.close()


# ---- 2. general affine transforms against baked geometry -----------------------------------------------------------------------------------
def _model_scenes(scale, padded):
    """(transformed scene, baked scene, mesh object index, matrix): the level-2 icosphere of the model test, alone or as object 35 of 40."""
    mesh = S.icosphere(T.MODEL_LEVEL, T.MODEL_CENTER, 1.0)
    m = T.model_transform(scale)
    baked = (T.bake_vertices(mesh[0], m, normals=False), mesh[1])
    out = []
    for v, i, transform in ((mesh[0], mesh[1], m), (baked[0], baked[1], None)):
        s = P.Scene()
        mat = s.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
        if padded:
            for k in range(35):
                s.add_sphere((200.0 + 3.0 * k, 300.0, 100.0), 0.5, mat)        # far from every ray
        ball = s.add_mesh(P.Mesh.from_arrays(v, i), mat, transform=transform)
        if padded:
            for k in range(4):
                s.add_sphere((200.0 + 3.0 * k, -300.0, 100.0), 0.5, mat)
        s.set_camera((0, 0, 5), (0, 0, -1), 60.0, 1.0)
        out.append(s)
    return out[0], out[1], ball, m


@pytest.mark.parametrize("padded", [False, True], ids=["alone", "object_35_of_40"])
@pytest.mark.parametrize("scale", T.MODEL_SCALES)
def test_affine_transforms_against_baked_geometry(scale, padded):
    """Held to transform_ref.MAX_DIFFERENT and RAY_BOUND; the device's figures are printed (DESIGN.md 5.16 records them)."""
    st, sb, ball, m = _model_scenes(scale, padded)
    o, d = T.model_rays(m, scale)
    r = P.Renderer(0)
    try:
        r.upload(st)                                               # sends the scene's transforms
        assert ball == (35 if padded else 0) and st.flatten().n_objects == (40 if padded else 1)
        t1, obj1, tri1, _ = r.intersect_rays(o, d)
        r.upload(sb)
        t0, obj0, tri0, _ = r.intersect_rays(o, d)
        tri1 = np.where(obj1 == ball, tri1.astype(np.int64), -1); tri0 = np.where(obj0 == ball, tri0.astype(np.int64), -1)
        assert set(np.unique(obj1)) <= {ball, 0xFFFFFFFF} and 0.3 < (tri0 >= 0).mean() < 0.95
        differ, rel = T.compare_hits(t1, tri1, t0, tri0)
        print(f"scale {scale} padded {padded}: {differ * o.shape[0]:.0f} of {o.shape[0]} rays differ in hit / miss or triangle, max |dt| / t = {rel:.3e}")
        assert differ <= T.MAX_DIFFERENT and rel <= T.RAY_BOUND
        # and the test can tell: with the transform ignored the rays aimed at the moved ball miss the stored one
        r.upload(st); r.update_transforms(_identity(st.flatten().n_objects))
        _, obj2, _, _ = r.intersect_rays(o, d)
        assert (obj2 == ball).mean() < 0.05
    finally:
        r.close(); st.close(); sb.close()


# ---- 3. guides of a placed smooth ball --------------------------------------------------------------------------------------------------------
GW = GH = 64
BALL_SCALE = 1.5
BALL_MATRIX = T.affine(T.rotation((2.0, -1.0, 0.5), 1.1) * BALL_SCALE, S.SPHERE_CENTER)     # the unit ball at the origin -> S.SPHERE_CENTER, radius 1.5


def _placed_ball_scene(matrix=BALL_MATRIX):
    s = P.Scene()
    diffuse = s.add_material(P.Material(albedo=(0.8, 0.7, 0.6)))
    emitter = s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=20.0, is_light=True))
    ball = s.add_mesh(P.Mesh.from_arrays(*S.icosphere(S.SPHERE_LEVEL, (0.0, 0.0, 0.0), 1.0)), diffuse, smooth=True, transform=matrix)
    lamp = s.add_sphere((6.0, 8.0, 6.0), 1.0, emitter)
    s.add_light(lamp)
    s.set_camera(*S.SPHERE_CAMERA, GW / GH)
    return s, ball, lamp


def _guide_model_figure():
    """The float32 model of the placed ball's guide normal, on the CPU: max |n - normalize(x - c)| over the pixels the comparison keeps."""
    v, i = S.icosphere(S.SPHERE_LEVEL, (0.0, 0.0, 0.0), 1.0)
    rows = S.triangle_rows((v, i))
    rec = T.invert(BALL_MATRIX)
    pos, view, fov = S.SPHERE_CAMERA
    d = R.primary_rays(pos, view, fov, GW / GH, GW, GH).reshape(-1, 3).astype(np.float32)
    o = np.broadcast_to(np.asarray(pos, np.float32), d.shape)
    oo, od = T.ray_to_object(rec, o, d)
    t, tri = T.intersect_triangles(rows, oo, od)
    hit = tri >= 0
    Pobj = (oo[hit] + od[hit] * t[hit][:, None]).astype(np.float32)
    n_obj, rule = S.hit_normals(rows, tri[hit], Pobj, od[hit], np.float32)
    n = T.normal_to_world(rec, n_obj.astype(np.float32)).astype(np.float64)
    x = (o[hit] + d[hit] * t[hit][:, None]).astype(np.float32)
    world_rows = S.triangle_rows((T.bake_vertices(v, BALL_MATRIX), i))
    _, rule64, radial, _, keep = S.sphere_guide_model(world_rows, tri[hit], x, pos, S.SPHERE_CENTER)
    return float(np.abs(n[keep] - radial[keep]).max()), float(1.0 - keep.mean())


def test_guides_of_a_placed_smooth_ball():
    """The bound: smooth_ref.GUIDE_BOUND (1e-5) where the float32 model stays under a quarter of it, else 4x the model's figure; the model's
    figure and the bound in force are printed."""
    model, model_excluded = _guide_model_figure()
    bound = S.GUIDE_BOUND if model <= S.GUIDE_BOUND / 4.0 else 4.0 * model
    max_excluded = S.MAX_EXCLUDED if model_excluded <= S.MAX_EXCLUDED / 4.0 else 4.0 * model_excluded
    print(f"float32 model: max |n - normalize(x - c)| = {model:.3e}, excluded {model_excluded:.4f}; bounds in force {bound:.3e}, {max_excluded:.4f}")
    v, i = S.icosphere(S.SPHERE_LEVEL, (0.0, 0.0, 0.0), 1.0)
    world_rows = S.triangle_rows((T.bake_vertices(v, BALL_MATRIX), i))
    s, ball, _ = _placed_ball_scene()
    r = P.Renderer(0)
    try:
        r.upload(s)
        r.render(GW, GH, 1)
        g = r.guides().copy()
        worst, excluded, _ = _compare_guides(g, ball, world_rows, S.SPHERE_CENTER, "placed")      # asserts that every position lies on a moved triangle
        assert worst <= bound and excluded <= max_excluded, (worst, excluded)
        hit = g[..., 7].view(np.uint32) == ball
        dist = np.linalg.norm(g[..., 0:3][hit].astype(np.float64) - S.SPHERE_CENTER, axis=-1)
        assert np.all(dist <= BALL_SCALE * (1.0 + 1e-5)) and np.all(dist >= 0.9 * BALL_SCALE)      # between the level-1 icosphere's faces and the moved sphere
        r.update_transforms(_identity(2))                          # the transform removed: the stored unit ball at the origin
        g0 = r.guides().copy()                                     # recomputed without a render
        hit0 = g0[..., 7].view(np.uint32) == ball
        radial = g0[..., 0:3][hit0].astype(np.float64) - S.SPHERE_CENTER
        radial /= np.linalg.norm(radial, axis=-1, keepdims=True)
        assert hit0.sum() > 50 and np.abs(g0[..., 4:7][hit0] - radial).max() > 0.1
    finally:
        r.close(); s.close()


# ---- 4. the three render paths agree -------------------------------------------------------------------------------------------------------------
def _five_transforms():
    rot = T.rotation((1.0, 2.0, 3.0), 0.7)
    return [rot, rot * 1.2, rot @ np.diag([1.2, 0.8, 1.0]), np.diag([1.0, 1.0, -1.0]) @ rot, None]     # rigid, uniform, non-uniform, mirrored, identity


def _transformed_material_scene(settings=None, far_spheres=0, baked=False):
    """test_gpu_smooth_normals' row of balls, all five materials, smooth normals on, every ball stored as the unit-centred icosphere and
    placed by its own transform (baked: the same world with the vertices moved on the host instead)."""
    materials = (DIFFUSE, MIRROR, GGX, GLASS, ROUGH_GLASS)
    s = P.Scene()
    ground = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=12.0, is_light=True))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), ground)
    lamp = s.add_sphere((0.5, 5.0, 2.0), 1.5, emitter)
    s.add_light(lamp)
    for k in range(far_spheres):
        s.add_sphere((300.0 + 3.0 * k, 400.0, 100.0), 0.5, ground)
    balls = []
    for k, (mat, A) in enumerate(zip(materials, _five_transforms())):
        mi = s.add_material(P.Material(**mat))
        centre = (2.1 * (k - 2.0), 0.0, -1.0)
        if A is None:
            balls.append(s.add_mesh(P.Mesh.from_arrays(*S.icosphere(1, centre, 0.95)), mi, smooth=True))
            continue
        v, i = S.icosphere(1, (0.0, 0.0, 0.0), 0.95)
        m = T.affine(A, centre)
        if baked:
            balls.append(s.add_mesh(P.Mesh.from_arrays(T.bake_vertices(v, m), i), mi, smooth=True))
        else:
            balls.append(s.add_mesh(P.Mesh.from_arrays(v, i), mi, smooth=True, transform=m))
    s.set_camera((0.3, 1.6, 5.5), (0.0, -0.25, -1.0), 60.0, 1.0)
    if settings is not None:
        s.set_settings(settings)
    return s, balls


@pytest.mark.parametrize("far_spheres", [0, 30], ids=["object_table_in_lds", "object_table_in_hbm"])
@pytest.mark.parametrize("M", [1, 4])
def test_render_paths_agree_to_the_bit_on_a_transformed_scene(M, far_spheres):
    st = P.Settings()
    s, balls = _transformed_material_scene(st, far_spheres)
    assert (s.flatten().n_objects > 31) == (far_spheres > 0)
    r = P.Renderer(0)
    try:
        r.set_nee_candidates(M)
        r.upload(s)
        plain = None
        for counters in (False, True):
            frames = [_frame(r, 48, 48, 8, k, st, counters) for k in KERNELS]
            for k, (acc, stats) in zip(KERNELS, frames):
                assert np.array_equal(_bits(acc), _bits(frames[0][0])) and stats.traced_rays == frames[0][1].traced_rays, (M, counters, k)
                assert stats.last_kernel == k
                assert stats.probe_resolved == 0                    # a transformed object turns the shade-side probe off
                if counters:
                    assert [getattr(stats, c) for c in COUNTERS] == [getattr(frames[0][1], c) for c in COUNTERS], (M, k)
            assert frames[0][0][..., :3].any()
            plain = frames[0][0] if plain is None else plain
            assert np.array_equal(_bits(plain), _bits(frames[0][0])), "the counters change the image"
        # and the test can tell: the transforms ignored give another image; the world baked on the host nearly the same one
        r.update_transforms(_identity(s.flatten().n_objects))
        ignored, _ = _frame(r, 48, 48, 8, KERNELS[0], st)
        assert not np.array_equal(_bits(plain), _bits(ignored))
        sb, _ = _transformed_material_scene(st, far_spheres, baked=True)
        r.upload(sb)
        r.render(48, 48, 1, settings=st)
        g_baked = r.guides()[..., 7].view(np.uint32).copy()
        sb.close()
        r.upload(s)
        r.render(48, 48, 1, settings=st)
        g = r.guides()[..., 7].view(np.uint32)
        assert (g == g_baked).mean() > 0.995                        # every ball is seen where its transform puts it
        for b in balls:
            assert (g == b).sum() > 20, b
    finally:
        r.close(); s.close()


# ---- 5. closed-form radiance through transformed meshes ------------------------------------------------------------------------------------------
CASE_MATRIX = T.affine(T.rotation((0.4, 1.0, -0.3), 0.9) @ np.diag([1.5, 0.6, 1.2]), (7.0, -3.0, 2.5))     # rotated, non-uniformly scaled, shifted


def _stored(mesh, m):
    """The mesh as it is stored so that m brings it back: positions A^-1 (p - b) in float64, normals A^T n (get_hit normalises)."""
    v, i = mesh
    m64 = np.asarray(m, np.float64)
    Ainv = np.linalg.inv(m64[:, :3])
    out = np.array(v, np.float32, copy=True)
    out[:, 0:3] = ((v[:, 0:3].astype(np.float64) - m64[:, 3]) @ Ainv.T).astype(np.float32)
    out[:, 3:6] = (v[:, 3:6].astype(np.float64) @ m64[:, :3]).astype(np.float32)
    return out, i


def _case_scene(c, transformed=True):
    """Case.build's P.Scene with every mesh stored in CASE_MATRIX's frame and returned by it."""
    s = P.Scene()
    for mat in c.materials:
        s.add_material(mat)
    for spec in c.objects:
        if spec[0] == "plane":
            s.add_plane(spec[1], spec[2], spec[3])
        elif spec[0] == "sphere":
            k = s.add_sphere(spec[1], spec[2], spec[3])
            if spec[4]:
                s.add_light(k)
        else:
            assert not spec[3]                                     # a transformed mesh cannot be a light
            v, i = _stored(spec[1], CASE_MATRIX)
            s.add_mesh(P.Mesh.from_arrays(v, i), spec[2], P.BUILD_SAH_INTERVALS, transform=CASE_MATRIX if transformed else None)
    pos, view, fov = c.camera
    s.set_camera(pos, view, fov, c.W / c.H)
    s.set_settings(c.settings())
    return s


_cases = {}


def _closed_form(name):
    if name not in _cases:
        _cases[name] = R.k1("ADVANCED", 2, mesh_floor=True, name=name) if name.startswith("K1") else R.k3("ADVANCED", 5, mesh_faces=True, name=name)
    return _cases[name]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["K1_advanced_two_lights_mesh_floor_transformed", "K3_advanced_depth5_mesh_transformed"])
def test_closed_form_radiance_through_transformed_meshes(name, kernel):
    """integrator_ref's K1 (mesh floor) and K3 (mesh faces) under Case.check at the case's own sample count."""
    c = _closed_form(name)
    s = _case_scene(c)
    r = P.Renderer(0)
    try:
        r.upload(s)
        origin = np.broadcast_to(np.asarray(c.camera[0], np.float32), (c.H * c.W, 3))
        t, obj, _, _ = r.intersect_rays(origin, c.rays().reshape(-1, 3).astype(np.float32))
        assert np.all(obj == c.primary_object) and np.allclose(t, c.primary_t.ravel(), rtol=1e-5)
        r.render(c.W, c.H, c.spp, seed=R.SEED, kernel=kernel, settings=c.settings())
        acc = r.accumulator().copy()
        c.check(acc, f"kernel {kernel}")
        first = _cases.setdefault(name + "/first", acc)
        assert np.array_equal(_bits(acc), _bits(first)), kernel
        if kernel == KERNELS[0]:                                   # and the test can tell: with the transforms left out the same rule fails
            r.update_transforms(_identity(s.flatten().n_objects))
            r.reset_accumulator()
            r.render(c.W, c.H, c.spp, seed=R.SEED, kernel=kernel, settings=c.settings())
            ratio, detail = c.worst(r.accumulator()[..., :3].astype(np.float64) / c.spp)
            print(f"{name}: transforms left out: worst residual / tolerance {ratio:.1f}")
            assert ratio > 1.0, detail
    finally:
        r.close(); s.close()


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------
SW = SH = 32
T1 = T.affine(T.rotation((0.0, 1.0, 0.2), 0.5), (0.4, 0.1, -0.3))
T2 = T.affine(T.rotation((1.0, 0.3, 0.0), -0.8) @ np.diag([1.1, 0.7, 1.3]), (-0.5, 0.3, 0.2))


def _state_scene(rows=None):
    """plane, lamp, a level-1 ball (object 2) and a triangle object (object 3); rows: other triangles for the ball (same topology)."""
    s = P.Scene()
    ground = s.add_material(P.Material(albedo=(0.7, 0.7, 0.7)))
    emitter = s.add_material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=12.0, is_light=True))
    paint = s.add_material(P.Material(albedo=(0.8, 0.5, 0.3)))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -1.2, 0.0), ground)
    lamp = s.add_sphere((0.5, 5.0, 2.0), 1.5, emitter)
    s.add_light(lamp)
    ball = s.add_mesh(P.Mesh.from_arrays(*S.icosphere(1, (0.0, 0.0, 0.0), 1.0)), paint)
    if rows is not None:
        s.refit_mesh(ball, rows)
    tri = s.add_triangle([(-2.5, -1.0, -1.0), (-1.0, -1.0, -1.5), (-1.8, 0.8, -1.2)], (0.2, 0.3, 0.93), paint)
    s.set_camera((0.2, 1.0, 4.5), (0.0, -0.2, -1.0), 60.0, 1.0)
    return s, lamp, ball, tri


def _matrices(n, **entries):
    m = _identity(n)
    for k, v in entries.items():
        m[int(k[1:])] = v
    return m


def _shot(r):
    acc, _ = _frame(r, SW, SH, 4, P.KERNEL_AUTO)
    return acc


def test_upload_resets_and_setting_twice_equals_setting_once():
    s, lamp, ball, tri = _state_scene()
    r, fresh = P.Renderer(0), P.Renderer(0)
    try:
        r.upload(s)
        base = _shot(r)                                             # no transform: the kernels of before
        r.update_transforms(_matrices(4, m2=T1, m3=T.MIRROR_Z))
        first = _shot(r)
        assert not np.array_equal(_bits(first), _bits(base))
        r.update_transforms(_matrices(4, m2=T2))                    # T1, then T2 ...
        fresh.upload(s); fresh.update_transforms(_matrices(4, m2=T2))
        assert np.array_equal(_bits(_shot(r)), _bits(_shot(fresh)))        # ... renders as a fresh upload with T2
        g_t2 = r.guides().copy()
        r.update_transforms(_matrices(4, m2=T1))
        g_t1 = r.guides().copy()                                    # the guides follow without a render
        assert not np.array_equal(_bits(g_t1), _bits(g_t2))
        fresh.update_transforms(_matrices(4, m2=T1)); _shot(fresh)
        assert np.array_equal(_bits(g_t1), _bits(fresh.guides()))
        r.update_transforms(_identity(4))                           # all-identity: the bits of before the feature's kernels
        assert np.array_equal(_bits(_shot(r)), _bits(base))
        r.update_transforms(_matrices(4, m2=T2))
        r.upload(s)                                                 # an upload resets every object to the identity
        assert np.array_equal(_bits(_shot(r)), _bits(base))
        s.set_transform(ball, T2)                                   # and upload() sends the scene's own
        r.upload(s)
        fresh.update_transforms(_matrices(4, m2=T2))
        assert np.array_equal(_bits(_shot(r)), _bits(_shot(fresh)))
    finally:
        r.close(); fresh.close(); s.close()


def test_the_other_edits_keep_the_transforms_and_it_keeps_theirs():
    s, lamp, ball, tri = _state_scene()
    rows = S.triangle_rows(S.icosphere(1, (0.0, 0.0, 0.0), 1.0))
    m = _matrices(4, m2=T2, m3=T1)

    def edits(r):
        s.set_material(2, P.Material(albedo=(0.6, 0.7, 0.9), specular=0.4, refractivity=0.3, roughness=0.3, transmission_roughness=0.2))
        r.update_materials(s)                                       # materials and both roughnesses
        r.update_smooth_normals(np.array([0, 0, 1, 0], np.uint32))
        r.update_primitive(lamp, 1, center=(0.5, 5.5, 2.0), radius=1.5)
        r.refit_mesh(ball, rows)                                    # the same triangles
    a, b, plain = P.Renderer(0), P.Renderer(0), P.Renderer(0)
    try:
        a.upload(s); a.update_transforms(m); edits(a)               # the transforms first, then every other edit
        b.upload(s); edits(b); b.update_transforms(m)               # the other way round
        plain.upload(s); edits(plain)
        fa, fb = _shot(a), _shot(b)
        assert np.array_equal(_bits(fa), _bits(fb))
        assert not np.array_equal(_bits(fa), _bits(_shot(plain)))
        assert np.array_equal(_bits(a.guides()), _bits(b.guides()))
    finally:
        a.close(); b.close(); plain.close(); s.close()


def test_refusals_leave_the_rendered_bits_unchanged():
    s, lamp, ball, tri = _state_scene()
    r = P.Renderer(0)
    L = r.L
    ptr = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).ctypes.data_as(FP)
    try:
        good = _matrices(4, m2=T2)
        assert L.cgpt_scene_update_transforms(None, ptr(good), 4) == N.CGPT_ERR_INVALID
        assert L.cgpt_scene_update_transforms(r._ctx, ptr(good), 4) == N.CGPT_ERR_NO_SCENE
        r.upload(s)
        r.update_transforms(good)
        before = _shot(r)
        nan = T2.copy(); nan[0, 3] = np.nan
        singular = T.affine([[1, 2, 3], [2, 4, 6], [0, 0, 1]], (0, 0, 0))
        far = T.affine(np.diag([1e-20, 1.0, 1.0]), (1e30, 0, 0))
        for matrices, n, what in ((None, 4, "expected 4"), (good, 3, "expected 4"), (good, 5, "expected 4"),
                                  (_matrices(4, m2=nan), 4, "not finite"), (_matrices(4, m2=singular), 4, "cannot be inverted"),
                                  (_matrices(4, m2=np.zeros((3, 4))), 4, "cannot be inverted"), (_matrices(4, m2=far), 4, "cannot be inverted"),
                                  (_matrices(4, m0=T1), 4, "plane"), (_matrices(4, m1=T1), 4, "sphere")):
            rc = L.cgpt_scene_update_transforms(r._ctx, None if matrices is None else ptr(matrices), n)
            assert rc == N.CGPT_ERR_INVALID and what in L.cgpt_last_error(r._ctx).decode(), (what, rc, L.cgpt_last_error(r._ctx))
            assert np.array_equal(_bits(_shot(r)), _bits(before)), what
        with pytest.raises(P.DeviceError, match="sphere"):          # the lamp is a sphere and a light: refused either way
            r.update_transforms(_matrices(4, m1=T2))
        assert np.array_equal(_bits(_shot(r)), _bits(before))
    finally:
        r.close(); s.close()
    # a mesh light
    s = P.Scene()
    paint = s.add_material(P.Material(albedo=(0.8, 0.5, 0.3)))
    emitter = s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=8.0, is_light=True))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), paint)
    panel = s.add_mesh(P.Mesh.from_arrays(*R.quad_mesh(3.0, -1.0, 1.0, -1.0, 1.0, -1.0)), emitter)
    s.add_light(panel)
    s.set_camera((0.0, 1.0, 4.0), (0.0, -0.2, -1.0), 60.0, 1.0)
    r = P.Renderer(0)
    try:
        r.upload(s)
        before = _shot(r)
        with pytest.raises(P.DeviceError, match="is a light"):
            r.update_transforms(_matrices(2, m1=T1))
        assert np.array_equal(_bits(_shot(r)), _bits(before))
    finally:
        r.close(); s.close()


def test_refit_of_a_transformed_mesh_takes_object_space_triangles():
    moved = S.triangle_rows(S.icosphere(1, (0.2, -0.1, 0.1), 0.8))           # object-space triangles, same topology
    s, lamp, ball, tri = _state_scene()
    s_moved, _, _, _ = _state_scene(rows=moved)
    m = _matrices(4, m2=T2)
    r, fresh = P.Renderer(0), P.Renderer(0)
    try:
        r.upload(s); r.update_transforms(m)
        before = _shot(r)
        r.refit_mesh(ball, moved)
        fresh.upload(s_moved); fresh.update_transforms(m)
        after = _shot(r)
        assert not np.array_equal(_bits(after), _bits(before))
        assert np.array_equal(_bits(after), _bits(_shot(fresh)))
        assert np.array_equal(_bits(r.guides()), _bits(fresh.guides()))
        # the exported tree is the object-space one
        assert np.array_equal(r.export_bvh(ball), fresh.export_bvh(ball))
        host = s_moved.bvh_export(ball)[0].view(np.float32)
        dev = r.export_bvh(ball).view(np.float32)
        assert np.allclose(dev[0, 0:3], host[0, 0:3], atol=1e-6) and np.allclose(dev[0, 4:7], host[0, 4:7], atol=1e-6)
    finally:
        r.close(); fresh.close(); s.close(); s_moved.close()


# ---- 7. two ranks -----------------------------------------------------------------------------------------------------------------------------
def test_two_rank_context_renders_the_transformed_scene_bit_identically():
    st = P.Settings()
    s, _ = _transformed_material_scene(st)
    n = s.flatten().n_objects
    W, H, spp = 48, 40, 6
    one = P.Renderer(0)
    g = P.Renderer([0, 0], flags=P.CTX_GATHER_PEER_COPY)
    try:
        one.upload(s)
        one.render(W, H, spp, settings=st)
        single = one.accumulator().copy()
        one.update_transforms(_identity(n)); one.reset_accumulator()
        one.render(W, H, spp, settings=st)
        untransformed = one.accumulator().copy()
        assert not np.array_equal(_bits(single), _bits(untransformed))
        g.upload(s)                                                # every member gets the transforms
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(single))
        bad = _identity(n); bad[1] = T1                            # the lamp: a refusal reaches the caller and changes no member
        assert g.L.cgpt_scene_update_transforms(g._ctx, bad.ctypes.data_as(FP), n) == N.CGPT_ERR_INVALID
        g.reset_accumulator()
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(single))
        g.update_transforms(_identity(n))
        g.reset_accumulator()
        g.render(W, H, spp, settings=st)
        assert np.array_equal(_bits(g.accumulator()), _bits(untransformed))
    finally:
        one.close(); g.close(); s.close()
