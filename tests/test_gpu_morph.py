"""Morph targets on the device (cgpt_scene_set_morph_targets / cgpt_scene_morph_mesh / cgpt_scene_clear_morph_targets; csrc/device/
refit.hip: morph_triangles), alone and fused with a skin, against a second context that was given refit_mesh(obj, ...) with the host
mirrors' triangles: the yardstick is never the code under test.  The scene is tests/test_gpu_skinning.py's."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from morph_cases import CASES, make_case
from scenes import standin_mesh
from skin_cases import make_case as skin_case
from test_gpu_refit import BIG, GROUND, LAMP, SUN, WALL, assert_same_frames, frames, fresh, make_scene, octahedron, random_rays
from test_gpu_skinning import KERNELS, MESHES, OCTA, SIZE, SKINNED, STRIP256, STRIP257, TRI, bits, build_scene

pytestmark = pytest.mark.gpu

MORPHED = SKINNED                                                              # 5120, 2, 1, 8, 255, 256 and 257 triangles


def objects_of(name):
    return (STRIP257, TRI) if name == "limit" else MORPHED                    # 256 targets on the small objects only


def install(r, binds, name, objs=None):
    cases = {}
    for obj in objs or objects_of(name):
        cases[obj] = make_case(name, binds[obj], seed=obj)
        r.set_morph_targets(obj, cases[obj][0], cases[obj][1])
    return cases


def pose_both(r, want, cases):
    for obj, (base, d, w) in cases.items():
        r.morph_mesh(obj, w)
        want.refit_mesh(obj, P.morph_triangles(base, d, w))


def assert_same_scene(r, want, objs=MESHES, configs=KERNELS, tops=(False, True)):
    o, d = random_rays(4096, 5)
    for top in tops:
        for ctx in (r, want):
            ctx.set_top_level(top)
        for obj in objs:
            if obj != TRI:
                dev, ref = r.export_bvh(obj), want.export_bvh(obj)
                assert np.array_equal(dev, ref), f"object {obj}: {np.count_nonzero(dev != ref)} words differ"
        for a, b in zip(r.intersect_rays(o, d), want.intersect_rays(o, d)):
            assert np.array_equal(bits(a), bits(b))
        assert_same_frames(frames(r, sizes=SIZE, configs=configs), frames(want, sizes=SIZE, configs=configs))
        assert np.array_equal(bits(r.guides()), bits(want.guides()))


@pytest.fixture(scope="module")
def world():
    s, binds = build_scene()
    yield s, binds
    s.close()


@pytest.fixture()
def pair(world):
    s, binds = world
    r, want = fresh(s), fresh(s)
    yield s, binds, r, want
    r.close(); want.close()


# ---- equality with the yardstick, case by case ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_a_morph_equals_a_refit_of_the_mirrors_triangles(pair, name):
    s, binds, r, want = pair
    cases = install(r, binds, name)
    pose_both(r, want, cases)
    assert_same_scene(r, want)
    moved = not np.array_equal(r.export_bvh(STRIP257), s.bvh_export(STRIP257)[0])
    assert moved == (name != "all_zero")                                      # the host scene stays where it was


@pytest.mark.parametrize("name", CASES)
def test_targets_stored_as_given_pose_to_the_same_bits(pair, name):
    s, binds, r, want = pair
    r.set_tuning(morph_leaf_order=0)                                          # read by set_morph_targets
    cases = install(r, binds, name)
    r.set_tuning(morph_leaf_order=1)                                          # the next set's: these targets stay as given
    pose_both(r, want, cases)
    assert_same_scene(r, want, configs=KERNELS[:1], tops=(False,))
    moved = not np.array_equal(r.export_bvh(STRIP257), s.bvh_export(STRIP257)[0])
    assert moved == (name != "all_zero")
    with pytest.raises(P.DeviceError, match="morph_leaf_order 2") as e:
        r.set_tuning(morph_leaf_order=2)
    assert e.value.code == N.CGPT_ERR_INVALID


@pytest.mark.parametrize("leaf_order", [0, 1])
def test_threads_that_stride_give_the_same_bits(pair, leaf_order):
    s, binds, r, want = pair
    r.set_tuning(morph_leaf_order=leaf_order)
    cases = install(r, binds, "mix", objs=(BIG,))
    pose_both(r, want, cases)
    ref = want.export_bvh(BIG)
    base_tree = s.bvh_export(BIG)[0]                                          # the base is the uploaded mesh: an all-zero pose returns to it
    for blocks in (1, 2, 1024):                                               # 5120 triangles: a thread strides 20 and 10 times, or not at all
        r.set_tuning(morph_max_blocks=blocks)
        r.morph_mesh(BIG, np.zeros(3, np.float32))
        assert np.array_equal(r.export_bvh(BIG), base_tree) and not np.array_equal(base_tree, ref)
        r.morph_mesh(BIG, cases[BIG][2])
        assert np.array_equal(r.export_bvh(BIG), ref)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[:1]), frames(want, sizes=SIZE, configs=KERNELS[:1]))
    for bad in (0, 1025):
        with pytest.raises(P.DeviceError, match=f"morph_max_blocks {bad} outside"):
            r.set_tuning(morph_max_blocks=bad)


# ---- fused with the skin ------------------------------------------------------------------------------------------------------
FUSED = (BIG, TRI, OCTA, STRIP257)


@pytest.mark.parametrize("leaf_order", [1, 0])
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("pose", ["bend", "four", "wide"])
def test_morph_and_skin_in_either_order_equal_the_composition(pair, pose, lds, leaf_order):
    s, binds, r, want = pair
    other = fresh(s)
    for ctx in (r, other):
        ctx.set_tuning(skin_joints_lds=lds, morph_leaf_order=leaf_order)      # the four fused instantiations
    morphs = {obj: make_case("mix", binds[obj], seed=obj) for obj in FUSED}
    for obj, (base, d, w) in morphs.items():
        j, sw, n_joints, m = skin_case(pose, base, seed=obj)
        for ctx in (r, other):
            ctx.set_skin(obj, binds[obj], j, sw, n_joints)
            ctx.set_morph_targets(obj, base, d)
        r.morph_mesh(obj, w); r.skin_mesh(obj, m)                             # morph, then skin
        other.skin_mesh(obj, m); other.morph_mesh(obj, w)                     # skin, then morph
        want.refit_mesh(obj, P.skin_triangles(P.morph_triangles(base, d, w), j, sw, m))
    assert_same_scene(r, want, objs=FUSED, tops=(True,))
    assert_same_scene(other, want, objs=FUSED, configs=KERNELS[1:2], tops=(False,))
    other.close()


def test_a_skin_alone_and_a_skin_after_clear_take_the_plain_path(pair):
    s, binds, r, want = pair
    base, d, w = make_case("mix", binds[BIG], seed=BIG)
    j, sw, n_joints, m = skin_case("four", binds[BIG], seed=BIG)
    r.set_skin(BIG, binds[BIG], j, sw, n_joints)
    oj, osw, on, om = skin_case("bend", binds[OCTA], seed=OCTA)               # a skinned object that never has targets
    r.set_skin(OCTA, binds[OCTA], oj, osw, on)
    r.skin_mesh(OCTA, om)
    want.refit_mesh(OCTA, P.skin_triangles(binds[OCTA], oj, osw, om))
    r.set_morph_targets(BIG, base, d)
    r.morph_mesh(BIG, w)                                                      # the skin has not been posed: the morph alone
    want.refit_mesh(BIG, P.morph_triangles(base, d, w))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(BIG))
    r.skin_mesh(BIG, m)
    want.refit_mesh(BIG, P.skin_triangles(P.morph_triangles(base, d, w), j, sw, m))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(BIG))
    r.clear_morph_targets(BIG); r.clear_morph_targets(BIG); r.clear_morph_targets(99)
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(BIG))            # the geometry stays where it is
    with pytest.raises(P.DeviceError, match="has no morph targets"):
        r.morph_mesh(BIG, w)
    r.skin_mesh(BIG, m)                                                       # back to the skin's own bind pose
    want.refit_mesh(BIG, P.skin_triangles(binds[BIG], j, sw, m))
    assert_same_scene(r, want, objs=(BIG, OCTA), configs=KERNELS[:2], tops=(False,))


# ---- state and interplay -------------------------------------------------------------------------------------------------
def test_set_alone_changes_nothing_and_a_b_a_leaves_a(pair):
    s, binds, r, _ = pair
    cfg = KERNELS[1:3]
    before = frames(r, sizes=SIZE, configs=cfg)
    trees = [r.export_bvh(obj) for obj in MESHES]
    fp = r.scene_footprint().device_bytes
    cases = install(r, binds, "mix")
    assert r.scene_footprint().device_bytes == fp                             # target buffers are not counted
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)            # the geometry moves at the first pose
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, trees))
    for obj, (base, d, w) in cases.items():
        r.morph_mesh(obj, w)
    fa = frames(r, sizes=SIZE, configs=cfg)
    ta = [r.export_bvh(obj) for obj in MESHES]
    assert not np.array_equal(fa[0][0], before[0][0])
    for obj in cases:
        r.morph_mesh(obj, np.float32([1.0, -1.0, 0.0]))
    assert not np.array_equal(frames(r, sizes=SIZE, configs=cfg)[0][0], fa[0][0])
    for obj, (base, d, w) in cases.items():
        r.morph_mesh(obj, w)
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), fa)
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, ta))
    for obj, (base, d, w) in cases.items():                                   # a second set replaces the first
        r.set_morph_targets(obj, base, d[:1])
        with pytest.raises(P.DeviceError, match="has 1 morph targets, got 3"):
            r.morph_mesh(obj, w)
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, ta))


def test_transforms_smooth_flags_and_materials_survive_a_morph():
    s, binds = build_scene(smooth=(BIG, TRI, STRIP257))
    s.set_transform(BIG, np.float32([[0.8, 0, 0.6, 0.4], [0, 1, 0, -0.2], [-0.6, 0, 0.8, 0.3]]))
    s.set_transform(STRIP256, np.float32([[1, 0, 0, 0.5], [0, 1.5, 0, 0], [0, 0, 1, 0.2]]))
    r, want = fresh(s), fresh(s)
    s.set_material(0, P.Material(albedo=(0.9, 0.3, 0.2), specular=0.2, roughness=0.3))
    r.update_materials(s); want.update_materials(s)
    pose_both(r, want, install(r, binds, "mix"))
    assert_same_scene(r, want)
    r.update_smooth_normals(np.zeros(10, np.uint32))                          # the smooth flag matters: the morphed normal pairs are read
    assert not np.array_equal(frames(r, sizes=SIZE, configs=KERNELS[:1])[0][0], frames(want, sizes=SIZE, configs=KERNELS[:1])[0][0])
    r.close(); want.close(); s.close()


def test_refit_then_morph_gives_the_morph_and_a_reupload_drops_the_targets(pair):
    s, binds, r, want = pair
    cases = install(r, binds, "mix", objs=(BIG, OCTA))
    moved = binds[BIG].copy().reshape(-1, 3, 6); moved[..., :3] += np.float32([0.3, 0.1, -0.4])
    r.refit_mesh(BIG, moved.reshape(-1, 18)); want.refit_mesh(BIG, moved.reshape(-1, 18))   # works as before and keeps the targets
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(BIG))
    pose_both(r, want, cases)                                                 # the next pose overwrites the refit
    assert_same_scene(r, want, objs=(BIG, OCTA), configs=KERNELS[:2], tops=(False,))
    r.upload(s)
    with pytest.raises(P.DeviceError, match="has no morph targets") as e:
        r.morph_mesh(BIG, cases[BIG][2])
    assert e.value.code == N.CGPT_ERR_INVALID


def test_a_morph_through_one_placement_moves_every_instance():
    big = standin_mesh(2)
    tris = P.triangles_from_arrays(*big)
    shift = lambda x: np.float32([[1, 0, 0, x], [0, 1, 0, 0.2], [0, 0, 1, 0.0]])
    s = make_scene(big, octahedron((2.0, 1.0, -1.0), 0.7))
    twins = [s.add_instance(BIG, 1, transform=shift(x), smooth=bool(k)) for k, x in enumerate((-2.5, 2.5))]
    r, want = P.Renderer(0), P.Renderer(0)
    r.upload(s, instanced=True); want.upload(s, instanced=True)
    base, d, w = make_case("mix", tris)
    r.set_morph_targets(twins[1], base, d)
    r.morph_mesh(twins[1], w)
    want.refit_mesh(twins[0], P.morph_triangles(base, d, w))
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(twins[1]))
    r.close(); want.close(); s.close()


def test_a_morph_drops_the_temporal_history(pair):
    s, binds, r, _ = pair
    base, d, w = make_case("mix", binds[BIG], seed=BIG)
    j, sw, n_joints, m = skin_case("bend", binds[BIG], seed=BIG)
    r.set_morph_targets(BIG, base, d)
    r.set_skin(BIG, binds[BIG], j, sw, n_joints)
    flags = (0, N.TEMPORAL_FOLLOW_POSES)
    steps = [lambda: r.morph_mesh(BIG, w), lambda: r.skin_mesh(BIG, m), lambda: r.morph_mesh(BIG, -w), lambda: r.skin_mesh(BIG, 0.5 * m)]
    for k, step in enumerate(steps):                                          # a morph and a pose through the fused path, without and with the flag
        follow = flags[k // 2]
        r.reset_accumulator(); r.render(64, 64, 2)
        temporal(r, follow)
        assert r.temporal_history().shape == (64, 64, 4)
        g = r.guides()
        step()
        with pytest.raises(P.DeviceError):
            r.temporal_history()                                             # refused until the next temporal call, as after a refit
        assert not np.array_equal(bits(r.guides()), bits(g))                 # and the guides are recomputed
        r.reset_accumulator(); r.render(64, 64, 2)
        temporal(r, follow)
        h = r.temporal_history()[..., 3]
        assert np.all(h[hit_mask(r)] == 2)                                   # the morphed object's pixels hold this frame alone


def test_a_refused_morph_keeps_the_guides_and_the_temporal_history(pair):
    s, binds, r, _ = pair
    base, d, w = make_case("mix", binds[BIG], seed=BIG)
    r.set_morph_targets(BIG, base, d)
    r.reset_accumulator(); r.render(64, 64, 2)
    temporal(r, 0)
    h = r.temporal_history()
    for bad in (lambda: r.morph_mesh(BIG, np.float32([1.0, np.nan, 0.0])), lambda: r.morph_mesh(BIG, w[:2]), lambda: r.morph_mesh(OCTA, w)):
        with pytest.raises(P.DeviceError):
            bad()
        assert np.array_equal(bits(r.temporal_history()), bits(h))           # nothing changed: the generations move once a pose is accepted
    r.morph_mesh(BIG, w)
    with pytest.raises(P.DeviceError):
        r.temporal_history()


def temporal(r, flags):
    r.denoise_temporal(iterations=1, follow_poses=bool(flags))


def hit_mask(r):
    mask = np.ascontiguousarray(r.guides()[..., 7]).view(np.uint32) == BIG    # guides: {x.xyz, t, n.xyz, bits(obj), ...}
    assert mask.sum() > 100
    return mask


def test_multi_device_context_morphs_every_member(pair):
    s, binds, _, one = pair
    g = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY)
    cases = install(g, binds, "mix", objs=(BIG, GROUND, TRI))
    pose_both(g, one, cases)
    assert np.array_equal(g.export_bvh(BIG), one.export_bvh(BIG))
    cfg = [(P.KERNEL_WAVEFRONT, None), (P.KERNEL_PERSISTENT, None)]
    assert_same_frames(frames(g, sizes=SIZE, configs=cfg), frames(one, sizes=SIZE, configs=cfg))
    g.clear_morph_targets(BIG)
    with pytest.raises(P.DeviceError, match="has no morph targets"):
        g.morph_mesh(BIG, cases[BIG][2])
    g.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_scene_unchanged(world):
    s, binds = world
    base, d, w = make_case("mix", binds[BIG])
    n = len(base)
    ob, od, ow = make_case("mix", binds[OCTA])
    r = P.Renderer(0)
    for call in (lambda: r.set_morph_targets(BIG, base, d), lambda: r.morph_mesh(BIG, w)):
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_NO_SCENE and "no scene uploaded" in str(e.value)
    r.clear_morph_targets(BIG)                                                # nothing to free
    r.upload(s)
    cfg = [(P.KERNEL_MEGAKERNEL, None), (P.KERNEL_PERSISTENT, None)]
    before = frames(r, sizes=SIZE, configs=cfg)
    inf_b = base.copy(); inf_b[3, 12] = -np.inf
    nan_d = d.copy(); nan_d[1, 7, 5] = np.nan
    set_cases = [
        (lambda: r.set_morph_targets(10, base, d), "out of range"),
        (lambda: r.set_morph_targets(SUN, base, d), "is a sphere"),
        (lambda: r.set_morph_targets(WALL, base, d), "is a plane"),
        (lambda: r.set_morph_targets(LAMP, ob, od), "is a light"),
        (lambda: r.set_morph_targets(BIG, ob, od), f"has {n} triangles, got 8"),
        (lambda: r.set_morph_targets(TRI, ob, od), "has 1 triangles, got 8"),
        (lambda: r.set_morph_targets(OCTA, ob, np.zeros((257, 8, 18), np.float32)), "n_targets 257 outside [1, 256]"),
        (lambda: r.set_morph_targets(BIG, inf_b, d), "base triangle 3: float 12 is not finite"),
        (lambda: r.set_morph_targets(BIG, base, nan_d), "target 1, triangle 7: float 5 is not finite"),
    ]
    for call, msg in set_cases:
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_INVALID and msg in str(e.value), (msg, str(e.value))
    L = N.lib()
    fp, tp = C.POINTER(C.c_float), C.POINTER(N.Triangle)
    for args, k, msg in (((None, d.ctypes.data_as(tp)), 3, "base_triangles is null"), ((base.ctypes.data_as(tp), None), 3, "target_deltas is null"),
                         ((base.ctypes.data_as(tp), d.ctypes.data_as(tp)), 0, "n_targets 0 outside")):
        assert L.cgpt_scene_set_morph_targets(r._ctx, BIG, *args, n, k) == N.CGPT_ERR_INVALID
        assert msg in L.cgpt_last_error(r._ctx).decode()
    with pytest.raises(P.DeviceError, match="has no morph targets"):         # none of the refused calls installed any
        r.morph_mesh(BIG, w)
    r.set_morph_targets(BIG, base, d)
    nan_w = w.copy(); nan_w[1] = np.nan
    pose_cases = [
        (lambda: r.morph_mesh(10, w), "out of range"),
        (lambda: r.morph_mesh(OCTA, w), "has no morph targets"),
        (lambda: r.morph_mesh(SUN, w), "has no morph targets"),
        (lambda: r.morph_mesh(BIG, w[:2]), "has 3 morph targets, got 2"),
        (lambda: r.morph_mesh(BIG, np.concatenate([w, w])), "has 3 morph targets, got 6"),
        (lambda: r.morph_mesh(BIG, nan_w), "morph weight 1 is not finite"),
    ]
    for call, msg in pose_cases:
        with pytest.raises(P.DeviceError) as e:
            call()
        assert e.value.code == N.CGPT_ERR_INVALID and msg in str(e.value), (msg, str(e.value))
    assert L.cgpt_scene_morph_mesh(r._ctx, BIG, None, 3) == N.CGPT_ERR_INVALID and "weights is null" in L.cgpt_last_error(r._ctx).decode()
    assert L.cgpt_scene_morph_mesh(None, BIG, None, 3) == N.CGPT_ERR_INVALID and L.cgpt_scene_set_morph_targets(None, 0, None, None, 0, 1) == N.CGPT_ERR_INVALID
    assert L.cgpt_scene_clear_morph_targets(None, 0) == N.CGPT_ERR_INVALID
    assert np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)
    r.morph_mesh(BIG, w)                                                      # the targets installed before the refused poses still work
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    r.close()
