"""Skinning on the device (cgpt_scene_set_skin / cgpt_scene_skin_mesh / cgpt_scene_clear_skin; csrc/device/refit.hip: skin_triangles)
against a second context that was given refit_mesh(obj, skin_triangles(...)) with the host mirror's triangles: the yardstick is never the
code under test.  The scene is tests/test_gpu_refit.py's, with a stand-alone triangle object, an octahedron that is no light and three
strip meshes around the 256-thread block edge added."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V, standin_mesh
from skin_cases import POSES, make_case, strip_mesh
from test_gpu_refit import BIG, CONFIGS, GROUND, LAMP, SUN, WALL, assert_same_frames, frames, fresh, make_scene, octahedron, random_rays

pytestmark = pytest.mark.gpu

TRI, OCTA, STRIP255, STRIP256, STRIP257 = 5, 6, 7, 8, 9
TRI_P = np.float32([[-3.0, 1.0, -1.0], [-1.5, 1.2, -1.0], [-2.2, 2.6, -0.5]])
TRI_N = np.float32([[0, 0, 1], [0.6, 0, 0.8], [0, 0.6, 0.8]])
KERNELS = CONFIGS[:4]                                                          # the three kernels and AUTO
SIZE = ((64, 64),)


def build_scene(smooth=()):
    big, lamp, octa = standin_mesh(4), octahedron((2.0, 1.0, -1.0), 0.7), octahedron((-2.0, -1.0, 0.5), 0.8)
    strips = [strip_mesh(n, origin=(-6.0, -2.5 + 0.9 * k, -2.0)) for k, n in enumerate((255, 256, 257))]
    s = make_scene(big, lamp)
    assert s.add_triangle(TRI_P, TRI_N, 3) == TRI
    assert s.add_mesh(P.Mesh.from_arrays(*octa), 0) == OCTA
    for k, m in enumerate(strips):
        assert s.add_mesh(P.Mesh.from_arrays(*m), 1) == STRIP255 + k
    for obj in smooth:
        s.set_smooth_normals(obj, True)
    binds = {BIG: P.triangles_from_arrays(*big), GROUND: P.triangles_from_arrays(GROUND_V, GROUND_I), OCTA: P.triangles_from_arrays(*octa),
             TRI: np.concatenate([TRI_P, TRI_N], axis=1).reshape(1, 18)}
    for k, m in enumerate(strips):
        binds[STRIP255 + k] = P.triangles_from_arrays(*m)
    assert [len(binds[o]) for o in (TRI, GROUND, OCTA, STRIP255, STRIP256, STRIP257, BIG)] == [1, 2, 8, 255, 256, 257, 5120]
    return s, binds


SKINNED = (BIG, GROUND, TRI, OCTA, STRIP255, STRIP256, STRIP257)
MESHES = tuple(o for o in SKINNED if o != TRI)


def install(r, binds, pose, objs=SKINNED):
    cases = {}
    for obj in objs:
        j, w, n_joints, m = make_case(pose, binds[obj], seed=obj)
        r.set_skin(obj, binds[obj], j, w, n_joints)
        cases[obj] = (j, w, m)
    return cases


def pose_both(r, want, binds, cases):
    for obj, (j, w, m) in cases.items():
        r.skin_mesh(obj, m.reshape(-1, 3, 4) if obj & 1 else m)               # both accepted shapes
        want.refit_mesh(obj, P.skin_triangles(binds[obj], j, w, m))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def pair():
    s, binds = build_scene()
    r, want = fresh(s), fresh(s)
    yield s, binds, r, want
    r.close(); want.close(); s.close()


# ---- equality with the yardstick, pose by pose -----------------------------------------------------------------------------
@pytest.mark.parametrize("pose", POSES)
def test_a_pose_equals_a_refit_of_the_mirrors_triangles(pair, pose):
    s, binds, r, want = pair
    for ctx in (r, want):
        ctx.set_top_level(False)
    cases = install(r, binds, pose)
    pose_both(r, want, binds, cases)
    for obj in MESHES:
        dev, ref = r.export_bvh(obj), want.export_bvh(obj)
        assert np.array_equal(dev, ref), f"object {obj}: {np.count_nonzero(dev != ref)} words differ"
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])        # the host scene stays at the bind pose
    o, d = random_rays(4096, 5)
    for a, b in zip(r.intersect_rays(o, d), want.intersect_rays(o, d)):
        assert np.array_equal(bits(a), bits(b))
    for top in (False, True):
        for ctx in (r, want):
            ctx.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))
        assert np.array_equal(bits(r.guides()), bits(want.guides()))
        for a, b in zip(r.intersect_rays(o, d), want.intersect_rays(o, d)):
            assert np.array_equal(bits(a), bits(b))


def test_the_joint_matrices_read_through_the_vector_cache_give_the_same_bits(pair):
    s, binds, r, want = pair
    cases = install(r, binds, "wide")
    r.set_tuning(skin_joints_lds=0)
    try:
        pose_both(r, want, binds, cases)
    finally:
        r.set_tuning(skin_joints_lds=1)
    for obj in MESHES:
        assert np.array_equal(r.export_bvh(obj), want.export_bvh(obj))
    assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:1]), frames(want, sizes=SIZE, configs=KERNELS[:1]))
    with pytest.raises(P.DeviceError, match="skin_joints_lds 2"):
        r.set_tuning(skin_joints_lds=2)


# ---- state and interplay -------------------------------------------------------------------------------------------------
def test_set_skin_alone_changes_nothing_and_a_b_a_leaves_a(pair):
    s, binds, _, _ = pair
    r = fresh(s)
    cfg = KERNELS[1:3]
    before = frames(r, sizes=SIZE, configs=cfg)
    trees = [r.export_bvh(obj) for obj in MESHES]
    a = install(r, binds, "bend")
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)            # the geometry moves at the first pose
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, trees))
    for obj, (j, w, m) in a.items():
        r.skin_mesh(obj, m)
    fa = frames(r, sizes=SIZE, configs=cfg)
    ta = [r.export_bvh(obj) for obj in MESHES]
    assert not np.array_equal(fa[0][0], before[0][0])
    b_m = {obj: make_case("half", binds[obj], seed=obj)[3] for obj in SKINNED}   # another pose of the same two-joint skins
    for obj, m in b_m.items():
        r.skin_mesh(obj, m)
    assert not np.array_equal(frames(r, sizes=SIZE, configs=cfg)[0][0], fa[0][0])
    for obj, (j, w, m) in a.items():
        r.skin_mesh(obj, m)
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), fa)
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, ta))
    # clear_skin keeps the last pose; afterwards the object has no skin; clearing again is fine
    for obj in SKINNED:
        r.clear_skin(obj)
        r.clear_skin(obj)
    r.clear_skin(99)
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), fa)
    with pytest.raises(P.DeviceError, match="has no skin"):
        r.skin_mesh(BIG, a[BIG][2])
    r.close()


def test_transforms_smooth_flags_and_materials_survive_a_pose():
    s, binds = build_scene(smooth=(BIG, TRI, STRIP257))
    turn = np.float32([[0.8, 0, 0.6, 0.4], [0, 1, 0, -0.2], [-0.6, 0, 0.8, 0.3]])
    s.set_transform(BIG, turn)
    s.set_transform(STRIP256, np.float32([[1, 0, 0, 0.5], [0, 1.5, 0, 0], [0, 0, 1, 0.2]]))
    r, want = fresh(s), fresh(s)
    s.set_material(0, P.Material(albedo=(0.9, 0.3, 0.2), specular=0.2, roughness=0.3))
    r.update_materials(s); want.update_materials(s)
    cases = install(r, binds, "four")
    pose_both(r, want, binds, cases)
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))
        assert np.array_equal(bits(r.guides()), bits(want.guides()))
    # the smooth flag matters: the posed normal pairs are read
    r.update_smooth_normals(np.zeros(10, np.uint32))
    assert not np.array_equal(frames(r, sizes=SIZE, configs=KERNELS[:1])[0][0], frames(want, sizes=SIZE, configs=KERNELS[:1])[0][0])
    r.close(); want.close(); s.close()


def test_refit_then_pose_gives_the_pose_and_a_reupload_drops_the_skin(pair):
    s, binds, _, want = pair
    r = fresh(s)
    cases = install(r, binds, "bend", objs=(BIG, OCTA))
    moved = binds[BIG].copy().reshape(-1, 3, 6); moved[..., :3] += np.float32([0.3, 0.1, -0.4])
    r.refit_mesh(BIG, moved.reshape(-1, 18))                                 # works as before and keeps the skin
    unposed = fresh(s)
    unposed.refit_mesh(BIG, moved.reshape(-1, 18))
    assert np.array_equal(r.export_bvh(BIG), unposed.export_bvh(BIG))
    unposed.close()
    yard = fresh(s)
    pose_both(r, yard, binds, cases)                                         # the next pose overwrites the refit
    assert np.array_equal(r.export_bvh(BIG), yard.export_bvh(BIG))
    assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:2]), frames(yard, sizes=SIZE, configs=KERNELS[:2]))
    yard.close()
    r.upload(s)
    with pytest.raises(P.DeviceError, match="has no skin") as e:
        r.skin_mesh(BIG, cases[BIG][2])
    assert e.value.code == N.CGPT_ERR_INVALID
    r.close()


def test_a_pose_through_one_placement_moves_every_instance():
    big = standin_mesh(2)
    tris = P.triangles_from_arrays(*big)
    shift = lambda x: np.float32([[1, 0, 0, x], [0, 1, 0, 0.2], [0, 0, 1, 0.0]])
    s = make_scene(big, octahedron((2.0, 1.0, -1.0), 0.7))
    twins = [s.add_instance(BIG, 1, transform=shift(x), smooth=bool(k)) for k, x in enumerate((-2.5, 2.5))]
    r, want = P.Renderer(0), P.Renderer(0)
    r.upload(s, instanced=True); want.upload(s, instanced=True)
    assert r.scene_footprint().n_mesh_copies < r.scene_footprint().n_mesh_objects
    fp = r.scene_footprint().device_bytes
    j, w, n_joints, m = make_case("bend", tris)
    r.set_skin(twins[1], tris, j, w, n_joints)
    assert r.scene_footprint().device_bytes == fp                           # skin buffers are not counted
    r.skin_mesh(twins[1], m)
    want.refit_mesh(twins[0], P.skin_triangles(tris, j, w, m))
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(twins[1]))
    r.close(); want.close(); s.close()


def test_a_pose_drops_the_temporal_history(pair):
    s, binds, _, _ = pair
    r = fresh(s)
    cases = install(r, binds, "bend", objs=(BIG,))
    for follow in (False, True):
        r.reset_accumulator(); r.render(64, 64, 2)
        r.denoise_temporal(iterations=1, follow_transforms=follow)
        assert r.temporal_history().shape == (64, 64, 4)
        g = r.guides()
        r.skin_mesh(BIG, cases[BIG][2] if follow else make_case("half", binds[BIG], seed=BIG)[3])
        with pytest.raises(P.DeviceError):
            r.temporal_history()                                             # refused until the next temporal call, as after a refit
        assert not np.array_equal(bits(r.guides()), bits(g))                 # and the guides are recomputed
        r.reset_accumulator(); r.render(64, 64, 2)
        r.denoise_temporal(iterations=1, follow_transforms=follow)
        assert np.all(r.temporal_history()[..., 3] == 2)                     # a history of this frame alone
    r.close()


def test_multi_device_context_poses_every_member(pair):
    s, binds, _, _ = pair
    g = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY)
    one = fresh(s)
    cases = install(g, binds, "four", objs=(BIG, GROUND, TRI))
    pose_both(g, one, binds, cases)
    assert np.array_equal(g.export_bvh(BIG), one.export_bvh(BIG))
    cfg = [(P.KERNEL_WAVEFRONT, None), (P.KERNEL_PERSISTENT, None)]
    assert_same_frames(frames(g, sizes=SIZE, configs=cfg), frames(one, sizes=SIZE, configs=cfg))
    g.clear_skin(BIG)
    with pytest.raises(P.DeviceError, match="has no skin"):
        g.skin_mesh(BIG, cases[BIG][2])
    g.close(); one.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_scene_unchanged(pair):
    s, binds, _, _ = pair
    tris = binds[BIG]
    n = len(tris)
    j, w, n_joints, m = make_case("bend", tris)
    r = P.Renderer(0)
    for call in (lambda: r.set_skin(BIG, tris, j, w, n_joints), lambda: r.skin_mesh(BIG, m)):
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_NO_SCENE and "no scene uploaded" in str(e.value)
    r.clear_skin(BIG)                                                        # nothing to free
    r.upload(s)
    cfg = [(P.KERNEL_MEGAKERNEL, None), (P.KERNEL_PERSISTENT, None)]
    before = frames(r, sizes=SIZE, configs=cfg)
    oj, ow, _, om = make_case("bend", binds[OCTA])
    bad_j = j.copy(); bad_j[n - 1, 2, 3] = 2
    nan_w = w.copy(); nan_w[7, 0, 1] = np.nan
    inf_b = tris.copy(); inf_b[3, 12] = -np.inf
    set_cases = [
        (lambda: r.set_skin(10, tris, j, w, n_joints), "out of range"),
        (lambda: r.set_skin(SUN, tris, j, w, n_joints), "is a sphere"),
        (lambda: r.set_skin(WALL, tris, j, w, n_joints), "is a plane"),
        (lambda: r.set_skin(LAMP, binds[OCTA], oj, ow, 2), "is a light"),
        (lambda: r.set_skin(BIG, binds[OCTA], oj, ow, 2), f"has {n} triangles, got 8"),
        (lambda: r.set_skin(TRI, binds[OCTA], oj, ow, 2), "has 1 triangles, got 8"),
        (lambda: r.set_skin(BIG, tris, j, w, 0), "n_joints 0 outside [1, 1024]"),
        (lambda: r.set_skin(BIG, tris, j, w, 1025), "n_joints 1025 outside"),
        (lambda: r.set_skin(BIG, tris, j, w, 1), "joint index 1 >= n_joints 1"),
        (lambda: r.set_skin(BIG, tris, bad_j, w, n_joints), "joint index 2 >= n_joints 2"),
        (lambda: r.set_skin(BIG, tris, j, nan_w, n_joints), "triangle 7: weight 1 is not finite"),
        (lambda: r.set_skin(BIG, inf_b, j, w, n_joints), "bind triangle 3: float 12 is not finite"),
    ]
    for call, msg in set_cases:
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_INVALID and msg in str(e.value), (msg, str(e.value))
    L = N.lib()
    u16, fp, TRI_PTR = C.POINTER(C.c_uint16), C.POINTER(C.c_float), C.POINTER(N.Triangle)
    for args, msg in (((None, j.ctypes.data_as(u16), w.ctypes.data_as(fp)), "bind_triangles is null"),
                      ((tris.ctypes.data_as(TRI_PTR), None, w.ctypes.data_as(fp)), "joints is null"),
                      ((tris.ctypes.data_as(TRI_PTR), j.ctypes.data_as(u16), None), "weights is null")):
        assert L.cgpt_scene_set_skin(r._ctx, BIG, *args, n, n_joints) == N.CGPT_ERR_INVALID
        assert msg in L.cgpt_last_error(r._ctx).decode()
    with pytest.raises(P.DeviceError, match="has no skin"):                  # none of the refused calls installed one
        r.skin_mesh(BIG, m)
    r.set_skin(BIG, tris, j, w, n_joints)
    nan_m = m.copy(); nan_m[1, 5] = np.nan
    pose_cases = [
        (lambda: r.skin_mesh(10, m), "out of range"),
        (lambda: r.skin_mesh(OCTA, m), "has no skin"),
        (lambda: r.skin_mesh(SUN, m), "has no skin"),
        (lambda: r.skin_mesh(BIG, m[:1]), "skin has 2 joints, got 1"),
        (lambda: r.skin_mesh(BIG, np.concatenate([m, m])), "skin has 2 joints, got 4"),
        (lambda: r.skin_mesh(BIG, nan_m), "joint 1: entry 5 is not finite"),
    ]
    for call, msg in pose_cases:
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_INVALID and msg in str(e.value), (msg, str(e.value))
    assert L.cgpt_scene_skin_mesh(r._ctx, BIG, None, 2) == N.CGPT_ERR_INVALID and "joint_matrices is null" in L.cgpt_last_error(r._ctx).decode()
    assert L.cgpt_scene_skin_mesh(None, BIG, None, 2) == N.CGPT_ERR_INVALID and L.cgpt_scene_set_skin(None, 0, None, None, None, 0, 1) == N.CGPT_ERR_INVALID
    assert np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)
    r.skin_mesh(BIG, m)                                                      # the skin that was installed before the refused poses still works
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    r.close()

