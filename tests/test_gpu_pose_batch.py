"""Many objects posed in one call (cgpt_scene_pose_objects; csrc/device/refit.hip: PoseObjects) against a twin context
that was given the host mirrors' triangles (refit_mesh) or the single calls (morph_mesh, then skin_mesh, entry by entry): the yardstick
is never the code under test.  Every comparison is to the bit.  The scene is tests/test_gpu_skinning.py's: objects of 1, 2, 8, 255, 256,
257 and 5120 triangles -- block edges, a leaf-rooted triangle object, shallow and deep trees side by side."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from morph_cases import make_case as morph_case
from scenes import GROUND_I, GROUND_V, standin_mesh
from skin_cases import make_case as skin_case
from test_gpu_morph import assert_same_scene
from test_gpu_refit import BIG, GROUND, assert_same_frames, frames, fresh, make_scene, octahedron, random_rays
from test_gpu_skinning import KERNELS, MESHES, OCTA, SIZE, STRIP255, STRIP256, STRIP257, TRI, bits, build_scene
from test_pose_batch_plan import crowd_scene

pytestmark = pytest.mark.gpu

# object -> (pose of its skin or None, case of its morph targets or None, morph_leaf_order the targets are stored with): skin only, morph
# only and both; targets stored either way; one small object with a 1024-joint skin next to the 2- and 6-joint ones
RECIPE = {BIG: ("four", "mix", 1), GROUND: ("bend", None, 1), TRI: (None, "mix", 0), OCTA: ("wide", None, 1),
          STRIP255: (None, "one", 1), STRIP256: ("bend", "mix", 0), STRIP257: ("half", None, 1)}


def install(r, binds, recipe=RECIPE):
    cases = {}
    for obj, (pose, morph, leaf) in recipe.items():
        c = dict(base=None, d=None, w=None, j=None, sw=None, m=None)
        if morph:
            c["base"], c["d"], c["w"] = morph_case(morph, binds[obj], seed=obj)
            r.set_tuning(morph_leaf_order=leaf)                               # read by set_morph_targets
            r.set_morph_targets(obj, c["base"], c["d"])
        if pose:
            c["j"], c["sw"], n_joints, c["m"] = skin_case(pose, binds[obj], seed=obj)
            r.set_skin(obj, binds[obj], c["j"], c["sw"], n_joints)
        cases[obj] = c
    r.set_tuning(morph_leaf_order=1)
    return cases


def entries_of(cases, objs=None):
    return [(obj, cases[obj]["m"], cases[obj]["w"]) for obj in (objs or cases)]


def mirror(binds, c, obj):
    """the host mirrors' triangles of an entry: morph, then skin (the morphed base is the skin's bind pose)"""
    t = binds[obj]
    if c["w"] is not None:
        t = P.morph_triangles(c["base"], c["d"], c["w"])
    if c["m"] is not None:
        t = P.skin_triangles(t, c["j"], c["sw"], c["m"])
    return t


def one_by_one(r, entries):
    for obj, m, w in entries:
        if w is not None:
            r.morph_mesh(obj, w)
        if m is not None:
            r.skin_mesh(obj, m)


def eased(cases, a):
    """another pose of the same skins and targets: the matrices a of the way to the identity, the weights scaled"""
    ident = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    out = {}
    for obj, c in cases.items():
        out[obj] = dict(c)
        if c["m"] is not None:
            out[obj]["m"] = (np.float32(1 - a) * c["m"] + np.float32(a) * ident).astype(np.float32)
        if c["w"] is not None:
            out[obj]["w"] = (np.float32(1 - a) * c["w"]).astype(np.float32)
    return out


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


# ---- 1. against the host mirrors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, {"skin_joints_lds": 0, "morph_max_blocks": 1}])
def test_a_batch_equals_a_refit_of_the_mirrors_triangles(pair, knobs):
    s, binds, r, want = pair
    cases = install(r, binds)
    if knobs:
        r.set_tuning(**knobs)                                                 # the vector-cache kernels; one block an entry: 5120 triangles stride 20 times
    r.pose_objects(entries_of(cases))
    for obj, c in cases.items():
        want.refit_mesh(obj, mirror(binds, c, obj))
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])        # the host scene stays where it was
    assert_same_scene(r, want, tops=(True,) if knobs else (False, True))


# ---- 2. against the single calls ------------------------------------------------------------------------------------------------
def test_a_batch_equals_the_single_calls_in_any_order_and_state(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    assert install(want, binds).keys() == cases.keys()
    full = entries_of(cases)
    r.pose_objects(full); one_by_one(want, full)
    assert_same_scene(r, want, configs=KERNELS[:2], tops=(True,))
    # what an entry leaves out comes from the object's last pose: weights alone on a posed skin, matrices alone on morphed targets
    again = eased(cases, 0.5)
    partial = [(BIG, None, again[BIG]["w"]), (STRIP256, again[STRIP256]["m"], None), (TRI, None, np.zeros(3, np.float32))]
    r.pose_objects(partial); one_by_one(want, partial)
    assert_same_scene(r, want, configs=KERNELS[:1], tops=(False,))
    # a batch of one is the single call
    r.pose_objects([(OCTA, again[OCTA]["m"], None)]); want.skin_mesh(OCTA, again[OCTA]["m"])
    r.pose_objects([(STRIP255, None, again[STRIP255]["w"])]); want.morph_mesh(STRIP255, again[STRIP255]["w"])
    assert_same_scene(r, want, configs=KERNELS[:1], tops=(False,))
    # the entries in reversed order give the same bits
    r.pose_objects(full[::-1]); one_by_one(want, full)
    assert_same_scene(r, want, configs=KERNELS[1:2], tops=(True,))
    # objects not named keep their bits
    trees = {obj: r.export_bvh(obj) for obj in MESHES}
    some = [(GROUND, again[GROUND]["m"], None), (STRIP257, again[STRIP257]["m"], None)]
    r.pose_objects(some); one_by_one(want, some)
    for obj in MESHES:
        assert np.array_equal(r.export_bvh(obj), trees[obj]) == (obj not in (GROUND, STRIP257))
    assert_same_scene(r, want, configs=KERNELS[:1], tops=(True,))
    # the single calls pick up what a batch left: the weights of its last morph, the matrices of its last pose
    last = eased(cases, 0.25)
    for ctx in (r, want):
        ctx.skin_mesh(STRIP256, last[STRIP256]["m"]); ctx.morph_mesh(BIG, last[BIG]["w"])
    assert_same_scene(r, want, objs=(BIG, STRIP256), configs=KERNELS[:1], tops=(False,))
    # an all-zero weight entry leaves the base, bit for bit (STRIP255 has no skin, and its base is the uploaded mesh)
    r.pose_objects([(STRIP255, None, np.float32([-0.0]))])
    assert np.array_equal(r.export_bvh(STRIP255), s.bvh_export(STRIP255)[0])
    r.pose_objects([])                                                        # nothing happens
    assert np.array_equal(r.export_bvh(STRIP255), s.bvh_export(STRIP255)[0])


# ---- 3. the range flag is an entry's own ----------------------------------------------------------------------------------------
def test_one_entry_out_of_range_leaves_the_others_on_the_root_path(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    far = cases[STRIP257]["m"].copy()
    far[:, 3] = np.float32(8e30)                                              # a translation beyond the 1e30 the bound fold starts from (the weights sum to 0.5)
    cases[STRIP257]["m"] = far
    full = entries_of(cases)
    r.pose_objects(full); one_by_one(want, full)
    o, d = random_rays(4096, 5)
    for top in (False, True):                                                 # the top-level tree reads every object's box
        r.set_top_level(top); want.set_top_level(top)
        for obj in MESHES:
            assert np.array_equal(r.export_bvh(obj), want.export_bvh(obj)), obj
        for a, b in zip(r.intersect_rays(o, d), want.intersect_rays(o, d)):
            assert np.array_equal(bits(a), bits(b))
        for (fa, ca), (fb, cb) in zip(frames(r, sizes=SIZE, configs=KERNELS[:2]), frames(want, sizes=SIZE, configs=KERNELS[:2])):
            assert np.array_equal(fa, fb) and ca[:-1] == cb[:-1]
        assert np.array_equal(bits(r.guides()), bits(want.guides()))


# ---- 4. many entries ------------------------------------------------------------------------------------------------------------
def test_three_hundred_objects_in_one_call():
    n = 300                                                                   # crosses 256 entries: more than one block of any per-entry table
    s = crowd_scene(n)
    s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    s.set_settings(P.Settings())
    r, want = fresh(s), fresh(s)
    entries = []
    for k in range(n):
        v, i = octahedron((0.5 * (k % 20) - 5.0, 0.5 * (k // 20) - 3.0, 0.0), 0.2)
        tris = P.triangles_from_arrays(v, i)
        j, sw, n_joints, m = skin_case("bend", tris, seed=k)
        m = m.copy(); m[1, 3] += np.float32(0.01 * (k % 7))                   # each its own pose
        w = None
        for ctx in (r, want):
            ctx.set_skin(k, tris, j, sw, n_joints)
        if k % 3 == 0:                                                        # every third one morphed as well: two instantiations in one batch
            base, d, w = morph_case("one", tris, seed=k)
            for ctx in (r, want):
                ctx.set_morph_targets(k, base, d)
        entries.append((k, m, w))
    r.pose_objects(entries)
    one_by_one(want, entries)
    for k in range(n):
        assert np.array_equal(r.export_bvh(k), want.export_bvh(k)), k
    assert not np.array_equal(r.export_bvh(n - 1), s.bvh_export(n - 1)[0])
    o, d = random_rays(8192, 7, spread=2.5)
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        hits = r.intersect_rays(o, d)
        for a, b in zip(hits, want.intersect_rays(o, d)):
            assert np.array_equal(bits(a), bits(b))
    r.close(); want.close(); s.close()


# ---- 5. an instanced upload -----------------------------------------------------------------------------------------------------
def test_an_entry_through_one_placement_moves_every_instance():
    big = standin_mesh(2)
    tris = P.triangles_from_arrays(*big)
    shift = lambda x: np.float32([[1, 0, 0, x], [0, 1, 0, 0.2], [0, 0, 1, 0.0]])
    s = make_scene(big, octahedron((2.0, 1.0, -1.0), 0.7))
    twins = [s.add_instance(BIG, 1, transform=shift(x), smooth=bool(k)) for k, x in enumerate((-2.5, 2.5))]
    r, want = P.Renderer(0), P.Renderer(0)
    r.upload(s, instanced=True); want.upload(s, instanced=True)
    j, sw, n_joints, m = skin_case("bend", tris)
    base, d, w = morph_case("mix", tris)
    ground = P.triangles_from_arrays(GROUND_V, GROUND_I)
    gj, gsw, gn, gm = skin_case("bend", ground)
    for ctx in (r, want):
        ctx.set_skin(twins[1], tris, j, sw, n_joints)
        ctx.set_skin(twins[0], tris, j, sw, n_joints)
        ctx.set_morph_targets(twins[1], base, d)
        ctx.set_skin(GROUND, ground, gj, gsw, gn)
    batch = [(GROUND, gm, None), (twins[1], m, w)]
    r.pose_objects(batch); one_by_one(want, batch)
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS), frames(want, sizes=SIZE, configs=KERNELS))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(twins[0]))
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    before = r.export_bvh(BIG)
    with pytest.raises(P.DeviceError, match=f"entries 0 and 2 name objects {twins[0]} and {twins[1]} of one instanced mesh group") as e:
        r.pose_objects([(twins[0], 0.5 * m, None), (GROUND, gm, None), (twins[1], m, None)])
    assert e.value.code == N.CGPT_ERR_INVALID and np.array_equal(r.export_bvh(BIG), before)
    r.close(); want.close(); s.close()


# ---- 6. refusals are atomic -----------------------------------------------------------------------------------------------------
def test_a_refused_batch_changes_nothing(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    full = entries_of(cases)
    for ctx in (r, want):
        ctx.pose_objects(full) if ctx is r else one_by_one(ctx, full)
        ctx.reset_accumulator(); ctx.render(64, 64, 2)
        ctx.denoise_temporal_following(iterations=1, poses=True, morphs=True)
    history = r.temporal_history()
    cfg = KERNELS[1:3]
    trees, before = [r.export_bvh(obj) for obj in MESHES], frames(r, sizes=SIZE, configs=cfg)
    again = eased(cases, 0.3)
    good = entries_of(again, (BIG, STRIP256))                                 # accepted entries in front: the last one refuses the batch
    m = again[GROUND]["m"]
    nan_m = m.copy(); nan_m[1, 5] = np.nan
    refused = [((GROUND, nan_m, None), "entry 2: joint 1: entry 5 is not finite"),
               ((GROUND, m[:1], None), "entry 2: object 1's skin has 2 joints, got 1"),
               ((TRI, m, None), f"entry 2: object {TRI} has no skin"),
               ((STRIP257, None, np.float32([0.5])), f"entry 2: object {STRIP257} has no morph targets"),
               ((STRIP255, None, np.float32([np.inf])), "entry 2: morph weight 0 is not finite"),
               ((BIG, again[BIG]["m"], None), "entries 0 and 2 both name object 0"),
               ((GROUND, None, None), "entry 2: object 1: neither joint matrices nor morph weights"),
               ((99, m, None), "entry 2: object 99 out of range")]
    for bad, text in refused:
        with pytest.raises(P.DeviceError) as e:
            r.pose_objects(good + [bad])
        assert e.value.code == N.CGPT_ERR_INVALID and text in str(e.value), (text, str(e.value))
        assert np.array_equal(bits(r.temporal_history()), bits(history))      # the generations move once a batch is accepted
    L = N.lib()
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    assert L.cgpt_scene_pose_objects(r._ctx, None, 3) == N.CGPT_ERR_INVALID and "poses is null" in L.cgpt_last_error(r._ctx).decode()
    for row, text in ((N.Pose(GROUND, 2, None, 0, None), "entry 0: joint_matrices is null"), (N.Pose(BIG, 0, fp, 3, None), "entry 0: weights is null")):
        assert L.cgpt_scene_pose_objects(r._ctx, (N.Pose * 1)(row), 1) == N.CGPT_ERR_INVALID and text in L.cgpt_last_error(r._ctx).decode()
    assert L.cgpt_scene_pose_objects(r._ctx, None, 0) == N.CGPT_OK and L.cgpt_scene_pose_objects(None, None, 0) == N.CGPT_ERR_INVALID
    assert np.array_equal(bits(r.temporal_history()), bits(history))
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, trees))
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)
    outs = []
    for ctx in (r, want):                                                     # the next flagged call still uses its history, as the twin's that saw no batch
        ctx.reset_accumulator(); ctx.render(64, 64, 2)
        outs.append(ctx.denoise_temporal_following(iterations=1, poses=True, morphs=True))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(bits(r.temporal_history()), bits(want.temporal_history())) and np.any(r.temporal_history()[..., 3] > 2)
    fresh_ctx = P.Renderer(0)
    with pytest.raises(P.DeviceError, match="no scene uploaded") as e:
        fresh_ctx.pose_objects(good)
    assert e.value.code == N.CGPT_ERR_NO_SCENE
    fresh_ctx.close()


# ---- 7. the temporal stage ------------------------------------------------------------------------------------------------------
def temporal(ctx, **follow):
    ctx.reset_accumulator(); ctx.render(64, 64, 2)
    rgba, px = ctx.denoise_temporal_following(iterations=1, **follow)
    try:
        carried = bits(ctx.previous_hits())
    except P.DeviceError as e:                                                # no carry-back ran: the same refusal on both sides
        carried = str(e)
    return bits(rgba), px, bits(ctx.temporal_history()), carried


def assert_same_temporal(a, b):
    for x, y in zip(a, b):
        assert (x == y) if isinstance(x, str) or isinstance(y, str) else np.array_equal(x, y)


def test_the_temporal_stage_follows_a_batch_as_it_follows_the_single_calls(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    both = dict(poses=True, morphs=True)
    first = entries_of(cases)
    r.pose_objects(first); one_by_one(want, first)
    assert_same_temporal(temporal(r, **both), temporal(want, **both))         # stores the history both sides reproject from
    steps = [([0.2], both), ([0.4, 0.5], both), ([0.6], dict(poses=True)), ([0.7], dict(morphs=True)), ([0.1], both), ([0.3], dict())]
    for eases, follow in steps:                                               # two batches straight after one another: the stamps and generations add up
        for a in eases:
            batch = entries_of(eased(cases, a))
            r.pose_objects(batch); one_by_one(want, batch)
        got, ref = temporal(r, **follow), temporal(want, **follow)
        assert_same_temporal(got, ref)
        if follow == both:
            assert not isinstance(got[3], str) and np.any(got[2].view(np.float32)[..., 3] > 2)   # the history was used and hits were carried back
    # skin only, morph only and both kinds of entry apart, each against its single call
    for objs in ((GROUND, OCTA), (TRI, STRIP255), (BIG,)):
        batch = entries_of(eased(cases, 0.8), objs)
        r.pose_objects(batch); one_by_one(want, batch)
        assert_same_temporal(temporal(r, **both), temporal(want, **both))


# ---- 8. a two-member context ----------------------------------------------------------------------------------------------------
def test_a_multi_device_context_poses_every_member(world):
    s, binds = world
    g, one = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY), fresh(s)
    cases = install(g, binds)
    install(one, binds)
    full = entries_of(cases)
    g.pose_objects(full); one_by_one(one, full)
    for obj in MESHES:
        assert np.array_equal(g.export_bvh(obj), one.export_bvh(obj))
    cfg = [(P.KERNEL_WAVEFRONT, None), (P.KERNEL_PERSISTENT, None)]
    for top in (False, True):                                                 # the members render half the rows each
        g.set_top_level(top); one.set_top_level(top)
        assert_same_frames(frames(g, sizes=SIZE, configs=cfg), frames(one, sizes=SIZE, configs=cfg))
    with pytest.raises(P.DeviceError, match="entries 0 and 1 both name object 0"):
        g.pose_objects([full[0], full[0]])
    assert np.array_equal(g.export_bvh(BIG), one.export_bvh(BIG))
    g.close(); one.close()
