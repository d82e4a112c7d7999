"""Stand-alone triangle objects (CGPT_OBJECT_TRIANGLE; ref: Include/Primitives.h:84-89, Source/Primitives.cpp:292-321) on the GPU.

Oracle: the unchanged C oracle with every triangle object replaced by a one-triangle mesh.  That mesh's BVH root is a leaf, so
BVH::Traverse tests the triangle directly -- no bounds test, no bvh_depth increment -- and its shading normal is the same v0.normal:
images, t, obj_idx and bvh_depth must be bit-identical.  What differs, in a known way:
  * tri_idx of a ray whose last hit is a triangle object: Primitive::Intersect leaves payload.tri_idx alone, so it is what the
    objects BEFORE the triangle object left there (the oracle's tri_idx over that prefix of the scene);
  * tri_tests counts BVH.cpp:76-77 only: the oracle's minus one test per stand-in per IntersectScene call;
  * closest_hits counts mesh hits only (ref: Main.cpp:332): at most the oracle's.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V, rmse, standin_mesh

pytestmark = pytest.mark.gpu

KERNELS = [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT]
SEED = 0x12345678
NO_HIT = 0xFFFFFFFF


class Pair:
    """One scene built twice: in the product (triangle objects) and in the oracle (one-triangle meshes in their place)."""

    def __init__(self):
        self.o = O.OracleScene()
        self.s = P.Scene()
        self.o.set_settings()
        self.s.set_settings(P.Settings())
        self.material_ops, self.object_ops = [], []
        self.kinds = []

    def _object(self, kind, op, add):
        k = op(self.o)
        self.object_ops.append(op)
        assert add() == k == len(self.kinds)
        self.kinds.append(kind)
        return k

    def material(self, m: P.Material) -> int:
        op = lambda o: o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light)
        self.material_ops.append(op)
        k = op(self.o)
        assert self.s.add_material(m) == k
        return k

    def mesh(self, v, i, mat):
        return self._object(N.OBJECT_MESH, lambda o: o.add_mesh(v, i, mat, O.BUILD_SAH_INTERVALS),
                            lambda: self.s.add_mesh(P.Mesh.from_arrays(v, i), mat, P.BUILD_SAH_INTERVALS))

    def sphere(self, c, r, mat):
        return self._object(N.OBJECT_SPHERE, lambda o: o.add_sphere(c, r, mat), lambda: self.s.add_sphere(c, r, mat))

    def plane(self, n, p, mat):
        return self._object(N.OBJECT_PLANE, lambda o: o.add_plane(n, p, mat), lambda: self.s.add_plane(n, p, mat))

    def triangle(self, positions, normal, mat):
        p = np.asarray(positions, np.float32).reshape(3, 3)
        n = np.broadcast_to(np.asarray(normal, np.float32).reshape(-1, 3), (3, 3))
        v = np.ascontiguousarray(np.hstack([p, n]), np.float32)
        return self._object(N.OBJECT_TRIANGLE, lambda o: o.add_mesh(v, np.array([0, 1, 2], np.uint32), mat, O.BUILD_SAH_INTERVALS),
                            lambda: self.s.add_triangle(p, n, mat))

    def light(self, k):
        self.o.add_light(k)
        self.s.add_light(k)

    def camera(self, pos=(0, 0, 8), view_dir=(0, 0, -1), fov=60.0, aspect=1.0):
        self.o.set_camera(pos, view_dir, fov, aspect)
        self.s.set_camera(pos, view_dir, fov, aspect)

    def set_material(self, index, m: P.Material):
        self.o.set_material(index, m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light)
        self.s.set_material(index, m)

    @property
    def n_triangles(self):
        return self.kinds.count(N.OBJECT_TRIANGLE)

    def oracle_prefix(self, k) -> O.OracleScene:
        """the oracle scene of objects [0, k) only"""
        o = O.OracleScene()
        for op in self.material_ops:
            op(o)
        for op in self.object_ops[:k]:
            op(o)
        return o


# ---- scenes --------------------------------------------------------------------------------------------------------------

def visible_surfaces() -> Pair:
    """diffuse, specular and mirror triangles, a mesh, the ground mesh, a back plane and two sphere lights.  The mesh comes FIRST
    in object order and the red triangle sits in front of it: rays reach the triangle carrying the mesh's (non-zero) tri_idx."""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True))
    red = p.material(P.Material(albedo=(0.9, 0.2, 0.1)))
    spec = p.material(P.Material(albedo=(0.2, 0.8, 0.3), specular=0.5))
    mirror = p.material(P.Material(albedo=(0.95, 0.95, 0.95), specular=1.0))
    blue = p.material(P.Material(albedo=(0.2, 0.2, 0.8)))
    v, i = standin_mesh(2)
    p.mesh(v, i, blue)                                                                   # 0: behind the red triangle
    p.mesh(GROUND_V, GROUND_I, grey)                                                     # 1
    p.triangle([[-2.5, -1.5, 1.0], [2.5, -1.0, 1.2], [0.0, 2.5, 0.8]], (0.0, 0.1, 1.0), red)          # 2
    p.plane((0, 0, 1), (0, 0, -15), grey)                                                # 3
    p.triangle([[-7.0, -2.0, 0.5], [-3.5, -2.5, 1.5], [-5.0, 2.0, 0.0]], (0.3, 0.2, 0.93), spec)      # 4
    p.triangle([[3.5, -2.5, 1.5], [7.0, -2.0, -1.0], [5.5, 3.0, 0.0]], (-0.6, 0.1, 0.79), mirror)    # 5
    for c in ((10.0, 10.0, 10.0), (-10.0, 10.0, -10.0)):
        p.light(p.sphere(c, 5.0, light))                                                 # 6, 7
    p.camera()
    return p


def occluder() -> Pair:
    """a triangle between a diffuse plane and the only (sphere) light: NEE shadow rays end on it"""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.8, 0.8, 0.8)))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=20.0, is_light=True))
    dark = p.material(P.Material(albedo=(0.3, 0.3, 0.3)))
    p.plane((0, 1, 0), (0, -3, 0), grey)
    p.triangle([[-3.0, 1.0, 2.0], [3.0, 1.0, 2.0], [0.0, 1.0, -5.0]], (0.0, -1.0, 0.0), dark)
    p.light(p.sphere((0.0, 8.0, -1.0), 1.5, light))
    p.camera(pos=(0, 2, 9), view_dir=(0, -0.45, -0.89))
    return p


def many_objects() -> Pair:
    """48 objects, 30 of them triangle objects: past the 31-entry LDS object table and the 16-record LDS triangle mirror"""
    p = Pair()
    mats = [p.material(P.Material(albedo=a, specular=s)) for a, s in
            (((0.8, 0.3, 0.3), 0.0), ((0.3, 0.8, 0.3), 0.3), ((0.3, 0.3, 0.8), 0.0), ((0.9, 0.9, 0.9), 1.0))]
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=8.0, is_light=True))
    p.mesh(GROUND_V, GROUND_I, mats[0])
    v, i = standin_mesh(0)
    rng = np.random.default_rng(11)
    n_tri = 0
    for k in range(45):
        if k % 3 != 2:                                  # 30 triangle objects in a 6 x 5 wall, interleaved with the rest
            gx, gy = n_tri % 6, n_tri // 6
            c = np.array([-6.0 + 2.4 * gx, -2.5 + 1.6 * gy, -1.0 - 0.3 * gx], np.float32)
            tri = c + rng.uniform(-1.3, 1.3, (3, 3)).astype(np.float32)
            nrm = rng.normal(0, 1, 3) + (0, 0, 2.0)
            p.triangle(tri, nrm / np.linalg.norm(nrm), mats[n_tri % 4])
            n_tri += 1
        elif k % 9 == 2:
            p.mesh(v * np.array([0.2, 0.2, 0.2, 1, 1, 1], np.float32) + np.array([k / 5 - 4, 1.5, 2.0, 0, 0, 0], np.float32), i, mats[2])
        else:
            p.sphere((k / 4 - 5, -2.0, 2.5), 0.5, mats[k % 4])
    p.plane((0, 0, 1), (0, 0, -12), mats[1])
    p.light(p.sphere((8.0, 10.0, 8.0), 4.0, light))
    p.light(p.sphere((-8.0, 10.0, 4.0), 3.0, light))
    p.camera()
    assert len(p.kinds) >= 40 and p.n_triangles >= 20
    return p


def edge_cases() -> Pair:
    """a back-facing triangle (hit: IntersectTriangle is double-sided) and a degenerate one (|a| < 0.001: never hit) in front"""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=10.0, is_light=True))
    red = p.material(P.Material(albedo=(0.9, 0.1, 0.1)))
    p.mesh(GROUND_V, GROUND_I, grey)
    # winding and normal both face away from the camera
    p.triangle([[-3.0, -1.0, 0.0], [0.0, 3.0, 0.0], [3.0, -1.0, 0.0]], (0.0, 0.0, -1.0), red)
    # collinear vertices: a = 0 for every ray
    p.triangle([[-4.0, -2.0, 3.0], [0.0, 0.0, 3.0], [4.0, 2.0, 3.0]], (0.0, 0.0, 1.0), red)
    # a sliver whose determinant stays below the reference's absolute epsilon
    p.triangle([[-2.0, 1.0, 4.0], [2.0, 1.0, 4.0], [0.0, 1.0002, 4.0]], (0.0, 0.0, 1.0), red)
    p.light(p.sphere((0.0, 10.0, 5.0), 3.0, light))
    p.camera()
    return p


def no_meshes() -> Pair:
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=10.0, is_light=True))
    green = p.material(P.Material(albedo=(0.1, 0.8, 0.2), specular=0.2))
    p.plane((0, 1, 0), (0, -3, 0), grey)
    p.triangle([[-3.0, -2.0, 0.0], [3.0, -2.0, -1.0], [0.0, 2.5, -0.5]], (0.0, 0.0, 1.0), green)
    p.triangle([[2.0, -3.0, -3.0], [6.0, -3.0, -3.0], [4.0, 1.0, -4.0]], (0.0, 0.2, 0.98), grey)
    p.light(p.sphere((0.0, 10.0, 5.0), 4.0, light))
    p.camera()
    return p


def glass() -> Pair:
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True))
    glass_m = p.material(P.Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517))
    v, i = standin_mesh(1)
    p.mesh(v, i, grey)
    p.mesh(GROUND_V, GROUND_I, grey)
    p.triangle([[-3.0, -2.0, 1.5], [3.0, -2.0, 1.0], [0.0, 3.0, 1.2]], (0.0, 0.0, 1.0), glass_m)
    p.triangle([[-2.5, -1.8, 2.5], [2.5, -1.8, 2.8], [0.0, 2.6, 2.6]], (0.0, 0.0, -1.0), glass_m)
    for c in ((10.0, 10.0, 10.0), (-10.0, 10.0, -10.0)):
        p.light(p.sphere(c, 5.0, light))
    p.camera()
    return p


# ---- render comparison ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(0)
    yield r
    r.close()


def _oracle_render(p: Pair, W, H, spp, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE):
    p.o.reset_accumulator(); p.o.reset_stats()
    p.o.render(W, H, spp, mode, debug, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    return p.o.accumulator(), p.o.pixels(), p.o.stats()


def _render(r, p: Pair, W, H, spp, kernel, counters, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE):
    r.upload(p.s)
    r.reset_accumulator(); r.reset_stats()
    r.render(W, H, spp, seed=SEED, kernel=kernel, counters=counters, settings=P.Settings(render_mode=mode, debug_render_mode=debug))
    return r.accumulator(), r.pixels(), r.stats()


def _check_stats(p: Pair, so, sg):
    assert sg.traced_rays == so.traced_rays
    assert sg.inner_steps == so.inner_steps
    assert sg.bvh_depth_sum == so.bvh_depth_sum
    assert sg.tri_tests == so.tri_tests - p.n_triangles * so.traced_rays
    assert sg.closest_hits <= so.closest_hits


def _check_exact(r, p: Pair, W, H, spp, kernel, mode=P.MODE_ADVANCED):
    """bit-identical image through the COUNT walk (with the stats relations) and through the hot path"""
    a0, px0, so = _oracle_render(p, W, H, spp, mode)
    for counters in (True, False):
        a1, px1, sg = _render(r, p, W, H, spp, kernel, counters, mode)
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), (counters, rmse(a0, a1))
        assert np.array_equal(px0, px1)
        if counters:
            _check_stats(p, so, sg)
            assert abs(so.total_energy_received - sg.total_energy_received) <= 1e-6 * max(1.0, so.total_energy_received)
    return a0, so, sg


@pytest.mark.parametrize("kernel", KERNELS)
def test_visible_surfaces_bit_identical(renderer, kernel):
    p = visible_surfaces()
    _, so, sg = _check_exact(renderer, p, 64, 64, 4, kernel)
    assert sg.closest_hits < so.closest_hits            # the triangle objects were seen and shaded, and are no mesh hits


@pytest.mark.parametrize("kernel", KERNELS)
def test_occluding_triangle_bit_identical(renderer, kernel):
    p = occluder()
    a0, _, _ = _check_exact(renderer, p, 64, 48, 4, kernel)
    assert a0[..., :3].any()
    # the shadow is real: rays from the floor under the triangle towards the light end on the triangle (object 1)
    xz = np.stack(np.meshgrid(np.linspace(-1.0, 1.0, 8), np.linspace(-1.0, 1.0, 8)), -1).reshape(-1, 2)
    origins = np.stack([xz[:, 0], np.full(len(xz), -2.999), xz[:, 1]], 1).astype(np.float32)
    d = np.array([0.0, 8.0, -1.0], np.float32) - origins
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    renderer.upload(p.s)
    _, obj, _, _ = renderer.intersect_rays(origins, d)
    assert (obj == 1).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_many_objects_bit_identical(renderer, kernel):
    _check_exact(renderer, many_objects(), 64, 64, 3, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_back_facing_and_degenerate_triangles(renderer, kernel):
    p = edge_cases()
    _check_exact(renderer, p, 48, 48, 2, kernel)
    # primary rays: the back-facing triangle (object 1) is hit, the degenerate ones (2, 3) in front of it never are
    o, d = p.o.camera_rays(48, 48)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    renderer.upload(p.s)
    _, obj, _, _ = renderer.intersect_rays(o, d)
    assert (obj == 1).sum() > 50
    assert not np.isin(obj, [2, 3]).any()


@pytest.mark.parametrize("kernel", KERNELS)
def test_scene_without_meshes(renderer, kernel):
    p = no_meshes()
    a0, so, sg = _check_exact(renderer, p, 48, 48, 3, kernel)
    assert sg.closest_hits == 0 and sg.tri_tests == 0 and sg.inner_steps == 0
    assert a0[..., :3].any()


@pytest.mark.parametrize("kernel", KERNELS)
def test_glass_triangles(renderer, kernel):
    p = glass()
    W, H, spp = 64, 64, 4
    a0, _, so = _oracle_render(p, W, H, spp)
    for counters in (True, False):
        a1, _, sg = _render(renderer, p, W, H, spp, kernel, counters)
        assert np.array_equal(a0[..., 3], a1[..., 3])
        assert rmse(a0[..., :3] / spp, a1[..., :3] / spp) < 1e-4      # Beer's law expf is value-only (test_gpu_parity.py)
        if counters:
            _check_stats(p, so, sg)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mode", [P.MODE_COMPARISON, P.MODE_BRUTE_FORCE])
def test_render_modes_bit_identical(renderer, kernel, mode):
    _check_exact(renderer, visible_surfaces(), 48, 40, 3, kernel, mode)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views_bit_identical(renderer, kernel, debug):
    p = visible_surfaces()
    _, px0, _ = _oracle_render(p, 64, 64, 1, debug=debug)
    for counters in (True, False):
        a1, px1, _ = _render(renderer, p, 64, 64, 1, kernel, counters, debug=debug)
        assert np.array_equal(px0, px1)
        assert not a1.any()                             # debug views bypass the accumulator (ref: Main.cpp:743-746)


# ---- IntersectScene on host rays -----------------------------------------------------------------------------------------

def test_intersect_rays_carry_tri_idx_over_triangle_objects(renderer):
    p = visible_surfaces()
    renderer.upload(p.s)
    rng = np.random.default_rng(5)
    n = 20000
    origins = np.tile(np.array([0, 0, 8], np.float32), (n, 1)) + rng.normal(0, 0.5, (n, 3)).astype(np.float32)
    target = np.stack([rng.uniform(-8, 8, n), rng.uniform(-4, 4, n), rng.uniform(-10, 2, n)], 1).astype(np.float32)
    d = target - origins
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    origins[:6] = np.array([0.1, 0.2, 3.0], np.float32)
    t0, obj0, tri0, dep0 = p.o.intersect_rays(origins, d)
    t1, obj1, tri1, dep1 = renderer.intersect_rays(origins, d)
    assert np.array_equal(obj0, obj1)
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
    assert np.array_equal(dep0, dep1)
    kinds = np.array(p.kinds + [N.OBJECT_PLANE])                 # index -1 (a miss) maps to something that is no triangle object
    hit_kind = kinds[np.where(obj0 == NO_HIT, -1, obj0.astype(np.int64))]
    mesh = hit_kind == N.OBJECT_MESH
    assert mesh.sum() > n // 10
    assert np.array_equal(tri0[mesh], tri1[mesh])
    carried = 0
    for k in np.unique(obj0[hit_kind == N.OBJECT_TRIANGLE]):
        sel = obj0 == k
        if k == 0:
            want = np.zeros(sel.sum(), np.uint32)
        else:
            want = p.oracle_prefix(int(k)).intersect_rays(origins[sel], d[sel])[2]
        assert np.array_equal(tri1[sel], want), k
        carried += int((want != 0).sum())
    assert (hit_kind == N.OBJECT_TRIANGLE).sum() > n // 20
    assert carried > 0                                  # some rays reach a triangle object with an earlier mesh's index


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------

def _raw_scene(kind=N.OBJECT_TRIANGLE, tri_count=1, tri_offset=0, node_count=0, light_is_triangle=False):
    tris = (N.Triangle * 2)()
    for t, z in zip(tris, (0.0, -1.0)):
        for v, xy in zip((t.v0, t.v1, t.v2), ((-1.0, -1.0), (1.0, -1.0), (0.0, 1.0))):
            v.pos = (C.c_float * 3)(xy[0], xy[1], z); v.normal = (C.c_float * 3)(0.0, 0.0, 1.0)
    objs = (N.Object * 2)()
    objs[0].kind, objs[0].mat_index, objs[0].tri_offset, objs[0].tri_count, objs[0].node_count = kind, 0, tri_offset, tri_count, node_count
    objs[1].kind, objs[1].mat_index, objs[1].sphere_radius = N.OBJECT_SPHERE, 1, 1.0
    objs[1].sphere_center = (C.c_float * 3)(0.0, 5.0, 0.0)
    mats = (N.Material * 2)()
    mats[0].albedo = (C.c_float * 3)(0.5, 0.5, 0.5)
    mats[1].emissive = (C.c_float * 3)(1.0, 1.0, 1.0); mats[1].intensity = 5.0; mats[1].is_light = 1
    tidx = (C.c_uint32 * 2)(0, 0)
    lights = (C.c_uint32 * 1)(0 if light_is_triangle else 1)
    desc = N.SceneDesc()
    desc.objects, desc.n_objects = objs, 2
    desc.nodes, desc.n_nodes = None, 0
    desc.triangles, desc.n_triangles = tris, 2
    desc.tri_indices = tidx
    desc.materials, desc.n_materials = mats, 2
    desc.light_indices, desc.n_lights = lights, 1
    return desc, (tris, objs, mats, tidx, lights)


def test_raw_abi_validates_triangle_objects(renderer):
    L, ctx = N.lib(), renderer._ctx

    def upload(**kw):
        desc, keep = _raw_scene(**kw)
        rc = L.cgpt_scene_upload(ctx, C.byref(desc))
        return rc, L.cgpt_last_error(ctx).decode()

    assert upload()[0] == N.CGPT_OK
    assert upload(tri_offset=1)[0] == N.CGPT_OK
    rc, msg = upload(light_is_triangle=True)
    assert rc == N.CGPT_ERR_UNSUPPORTED and "Main.cpp:383" in msg, msg
    for bad in (dict(tri_count=2), dict(tri_count=0), dict(tri_offset=2), dict(node_count=1)):
        rc, msg = upload(**bad)
        assert rc == N.CGPT_ERR_INVALID, (bad, rc, msg)
    rc, msg = upload(kind=4)                            # AABB and anything past it: the reference EXCEPTs (Primitives.cpp:302-305)
    assert rc == N.CGPT_ERR_UNSUPPORTED, msg


# ---- multi-device context ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_multi_device_context_and_material_update(renderer, kernel):
    p = visible_surfaces()
    W, H, spp = 64, 48, 3
    single, _, _ = _render(renderer, p, W, H, spp, kernel, False)
    g = P.Renderer([0, 0, 0], flags=P.CTX_GATHER_PEER_COPY)
    try:
        g.upload(p.s)
        g.render(W, H, spp, seed=SEED, kernel=kernel)
        assert np.array_equal(g.accumulator().view(np.uint32), single.view(np.uint32))
        red = p.s.flatten().objects[2].mat_index                # the red triangle's own material
        assert p.kinds[2] == N.OBJECT_TRIANGLE
        p.set_material(red, P.Material(albedo=(0.1, 0.9, 0.9), specular=0.4))
        g.update_materials(p.s)
        g.reset_accumulator()
        g.render(W, H, spp, seed=SEED, kernel=kernel)
        a0, px0, _ = _oracle_render(p, W, H, spp)
        a1 = g.accumulator()
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
        assert np.array_equal(px0, g.pixels())
        assert not np.array_equal(a1.view(np.uint32), single.view(np.uint32))
    finally:
        g.close()
