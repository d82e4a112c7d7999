"""Blended and looped clips on the device (cgpt_scene_animate_layers; csrc/device/refit.hip: animate_layers_batch)
against a twin context posed by pose_objects with the host mirror's matrices (P.animate_layers): the yardstick is never the code under
test.  Every comparison is to the bit.  The scene, skins and targets are tests/test_gpu_pose_batch.py's."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from anim_cases import CASES as CLIP_CASES, overflow
from anim_layer_cases import CASES, EMPTY, clips_of
from anim_layer_ref import WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG, clip_range
from morph_cases import make_case as morph_case
from scenes import standin_mesh
from skin_cases import make_case as skin_case
from test_gpu_animation import ANIMATED, RIGS, SHARED, free_skin
from test_gpu_morph import assert_same_scene
from test_gpu_pose_batch import assert_same_temporal, install, temporal
from test_gpu_refit import BIG, GROUND, assert_same_frames, frames, fresh, make_scene, octahedron, random_rays
from test_gpu_skinning import KERNELS, MESHES, OCTA, SIZE, STRIP255, STRIP256, TRI, bits, build_scene
from test_pose_batch_plan import crowd_scene

pytestmark = pytest.mark.gpu

CL, LO, PP = WRAP_CLAMP, WRAP_LOOP, WRAP_PINGPONG
# what an entry blends, by its position in the call: (clip 0..3, time offset, weight, wrap) per layer -- 1 to 4 layers, inactive ones among them
PATTERNS = [[(0, 0.0, 1.0, CL)],
            [(0, 0.0, 0.25, LO), (1, 0.3, 0.75, CL)],
            [(1, -0.7, 2.0, PP), (3, 0.2, 0.5, CL), (2, 1.9, 1.0, LO)],
            [(0, 0.1, 1.0, PP), (1, 0.6, 0.5, LO), (2, 0.45, 0.25, CL), (3, 3.3, 2.0, PP)],
            [(2, 0.4, 0.0, LO), (0, 0.7, 1.0, CL), (1, 0.2, 3.0, LO)],
            [(1, 0.25, 0.5, CL), (2, 0.4, 0.0, PP), (0, 2.5, 0.5, LO)],
            [(3, 0.3, 0.0, CL), (2, 4.1, 0.3, LO)]]


def rig_up(r):
    """skeletons on every animated object of r and four clips each, created: obj -> (skeleton, clip data x 4, handles x 4)"""
    out = {}
    for obj, (n, seed, shape, root) in RIGS.items():
        skeleton, clips = clips_of(n, seed, shape, root)
        out[obj] = (skeleton, clips, [r.create_clip(*c) for c in clips])
    for obj in SHARED[1:]:
        out[obj] = out[GROUND]
    for obj in ANIMATED:
        r.set_skeleton(obj, *out[obj][0])
    return out


def layers_of(rig, pattern, t):
    """(the call's layers, the mirror's) of one entry at time t"""
    skeleton, clips, handles = rig
    return [(handles[c], t + dt, w, wrap) for c, dt, w, wrap in pattern], [(clips[c], t + dt, w, wrap) for c, dt, w, wrap in pattern]


def entries_at(rigs, cases, t, objs=ANIMATED, shift=0):
    """the call's entries and the twin's: each object at its own time t + 0.11 k under its own pattern"""
    anim, posed = [], []
    for k, obj in enumerate(objs):
        dev, host = layers_of(rigs[obj], PATTERNS[(k + shift) % len(PATTERNS)], t + 0.11 * k)
        anim.append((obj, dev, cases[obj]["w"]))
        posed.append((obj, P.animate_layers(rigs[obj][0], host), cases[obj]["w"]))
    return anim, posed


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


# ---- 1. against pose_objects with the mirror's matrices ------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, {"skin_joints_lds": 0}])
def test_a_blended_batch_equals_a_batch_posed_with_the_mirrors_matrices(pair, knobs):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    rigs = rig_up(r)
    if knobs:
        r.set_tuning(**knobs); want.set_tuning(**knobs)
    anim, posed = entries_at(rigs, cases, 0.2, shift=1)                       # the entries with morph weights among them (install's)
    assert any(w is not None for _, _, w in anim) and {len(l) for _, l, _ in anim} >= {2, 3, 4}
    r.animate_layers(anim); want.pose_objects(posed)
    for obj, m, _ in posed:                                                   # the skin's last pose is what the mirror computes
        assert np.array_equal(bits(r.joint_matrices(obj)), bits(m)), obj
    assert not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    assert_same_scene(r, want, tops=(True,) if knobs else (False, True))      # through the list and through the tree
    # a second call at other times, then the single calls: they continue from the blended pose exactly as on the twin
    anim, posed = entries_at(rigs, cases, 0.55, (OCTA, STRIP256, BIG), shift=3)
    r.animate_layers(anim); want.pose_objects(posed)
    for ctx in (r, want):
        ctx.morph_mesh(BIG, np.float32(0.5) * cases[BIG]["w"])                # takes the skin's last matrices: the kernel's
        ctx.skin_mesh(STRIP256, cases[STRIP256]["m"])                         # takes the last weights
        ctx.morph_mesh(STRIP256, np.float32(0.25) * cases[STRIP256]["w"])
    assert np.array_equal(bits(r.joint_matrices(BIG)), bits(posed[2][1])) and np.array_equal(bits(r.joint_matrices(STRIP256)), bits(cases[STRIP256]["m"]))
    assert_same_scene(r, want, configs=KERNELS[1:2], tops=(False,))
    r.animate_layers([])                                                      # nothing happens
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(BIG))
    for obj in (BIG, GROUND):                                                 # the range the wraps go over is the mirror's
        for data, handle in zip(*rigs[obj][1:]):
            assert np.array_equal(bits(r.clip_range(handle)), bits(clip_range(data))) and np.array_equal(bits(P.clip_range(data)), bits(clip_range(data)))


# ---- 2. every case of the CPU tests, on the device ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_the_joint_matrices_of_every_case_are_the_mirrors(pair, name):
    s, binds, r, want = pair
    skeleton, sets = CASES[name]()
    n = len(skeleton[0])
    j, w = free_skin(binds[OCTA], n, 5)
    for ctx in (r, want):
        ctx.set_skin(OCTA, binds[OCTA], j, w, n)
    r.set_skeleton(OCTA, *skeleton)
    handles = {}
    for layers in sets:
        for clip, _, _, _ in layers:
            if id(clip) not in handles:
                handles[id(clip)] = r.create_clip(*clip)
    for k, layers in enumerate(sets):
        r.animate_layers([(OCTA, [(handles[id(c)], t, a, wrap) for c, t, a, wrap in layers], None)])
        m = P.animate_layers(skeleton, layers)
        assert np.array_equal(bits(r.joint_matrices(OCTA)), bits(m)), (name, k)
    want.skin_mesh(OCTA, m)
    assert np.array_equal(r.export_bvh(OCTA), want.export_bvh(OCTA))
    if skeleton[3] is not None:                                               # without the root: no multiply at all
        r.set_skeleton(OCTA, *skeleton[:3])
        r.animate_layers([(OCTA, [(handles[id(c)], t, a, wrap) for c, t, a, wrap in sets[3]], None)])
        assert np.array_equal(bits(r.joint_matrices(OCTA)), bits(P.animate_layers(skeleton[:3] + (None,), sets[3])))
    for h in handles.values():
        r.destroy_clip(h)


@pytest.mark.parametrize("name", ["arm", "two_roots", "j257", "j1024"])
def test_a_one_layer_clamped_call_is_animate_objects_to_the_bit(pair, name):
    s, binds, r, want = pair
    skeleton, clip, times = CLIP_CASES[name]()
    n = len(skeleton[0])
    j, w = free_skin(binds[OCTA], n, 5)
    for ctx in (r, want):
        ctx.set_skin(OCTA, binds[OCTA], j, w, n)
        ctx.set_skeleton(OCTA, *skeleton)
    handle, twin = r.create_clip(*clip), want.create_clip(*clip)
    idle = r.create_clip(*EMPTY(n))
    for k, t in enumerate(times):
        layers = [(handle, t, 0.7, CL)] if k % 2 else [(idle, 0.0, 0.0, LO), (handle, t, 1.0, CL), (idle, 1.0, 0.0, PP)]
        r.animate_layers([(OCTA, layers, None)]); want.animate_objects([(OCTA, twin, t, None)])
        assert np.array_equal(bits(r.joint_matrices(OCTA)), bits(want.joint_matrices(OCTA))), (name, t)
        assert np.array_equal(r.export_bvh(OCTA), want.export_bvh(OCTA))


# ---- 3. a crowd: 300 entries, 1 to 4 layers mixed, every character at its own times and wraps -----------------------------------
def test_three_hundred_characters_blend_their_own_layers():
    n = 300                                                                   # crosses 256 entries
    s = crowd_scene(n)
    s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    s.set_settings(P.Settings())
    r, want = fresh(s), fresh(s)
    skeleton, clips = clips_of(2, 21, "chain", True)
    rig = (skeleton, clips, [r.create_clip(*c) for c in clips])
    anim, posed = [], []
    for k in range(n):
        v, i = octahedron((0.5 * (k % 20) - 5.0, 0.5 * (k // 20) - 3.0, 0.0), 0.2)
        tris = P.triangles_from_arrays(v, i)
        j, sw, n_joints, _ = skin_case("bend", tris, seed=k)
        w = None
        for ctx in (r, want):
            ctx.set_skin(k, tris, j, sw, n_joints)
        if k % 3 == 0:                                                        # every third one morphed as well: its entry carries weights
            base, d, w = morph_case("one", tris, seed=k)
            for ctx in (r, want):
                ctx.set_morph_targets(k, base, d)
        r.set_skeleton(k, *skeleton)
        dev, host = layers_of(rig, PATTERNS[k % len(PATTERNS)], 0.013 * k - 0.6)
        anim.append((k, dev, w))
        posed.append((k, P.animate_layers(skeleton, host), w))
    r.animate_layers(anim); want.pose_objects(posed)
    for k in range(n):
        assert np.array_equal(r.export_bvh(k), want.export_bvh(k)), k
        assert np.array_equal(bits(r.joint_matrices(k)), bits(posed[k][1])), k
    assert not np.array_equal(r.export_bvh(n - 1), s.bvh_export(n - 1)[0])
    o, d = random_rays(8192, 7, spread=2.5)
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        for a, b in zip(r.intersect_rays(o, d), want.intersect_rays(o, d)):
            assert np.array_equal(bits(a), bits(b))
    r.close(); want.close(); s.close()


# ---- 4. the temporal stage ------------------------------------------------------------------------------------------------------
def test_the_temporal_stage_follows_blended_frames_as_it_follows_the_twins(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    rigs = rig_up(r)
    both = dict(poses=True, morphs=True)
    anim, posed = entries_at(rigs, cases, 0.1)
    r.animate_layers(anim); want.pose_objects(posed)
    assert_same_temporal(temporal(r, **both), temporal(want, **both))         # stores the history both sides reproject from
    for t, follow in ((0.3, dict(poses=True)), (0.5, both)):
        anim, posed = entries_at(rigs, cases, t, shift=2)
        r.animate_layers(anim); want.pose_objects(posed)
        got, ref = temporal(r, **follow), temporal(want, **follow)
        assert_same_temporal(got, ref)
    assert not isinstance(got[3], str) and np.any(got[2].view(np.float32)[..., 3] > 2)   # the history was used and hits were carried back


# ---- 5. refusals are atomic -----------------------------------------------------------------------------------------------------
def test_a_refused_call_changes_nothing(pair):
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    rigs = rig_up(r)
    anim, posed = entries_at(rigs, cases, 0.2)
    for ctx in (r, want):
        ctx.animate_layers(anim) if ctx is r else ctx.pose_objects(posed)
        ctx.reset_accumulator(); ctx.render(64, 64, 2)
        ctx.denoise_temporal_following(iterations=1, poses=True, morphs=True)
    history = r.temporal_history()
    cfg = KERNELS[1:3]
    trees, before = [r.export_bvh(obj) for obj in MESHES], frames(r, sizes=SIZE, configs=cfg)
    kept = {obj: r.joint_matrices(obj) for obj in ANIMATED}
    # an object whose composed matrices leave float's range: three chained scales of 1e30 under a three-joint skin
    j, sw, n_joints, _ = skin_case("rigid", binds[STRIP255])
    for ctx in (r, want):
        ctx.set_skin(STRIP255, binds[STRIP255], j, sw, n_joints)              # neither poses it
    far, far_clip, _ = overflow(3)
    r.set_skeleton(STRIP255, *far)
    far_handle = r.create_clip(*far_clip)
    gone = r.create_clip(*rigs[GROUND][1][0])
    r.destroy_clip(gone)
    wide = rigs[OCTA][2][0]
    good = entries_at(rigs, cases, 0.4, (BIG, STRIP256))[0]                   # accepted entries in front: the last one refuses the call
    g, g2 = rigs[GROUND][2][:2]
    ok = (g, 0.1, 1.0, LO)
    refused = [((GROUND, [ok, (99, 0.1, 1.0, CL)], None), "entry 2: layer 1: clip 99 is unknown or destroyed"),
               ((GROUND, [(0, 0.1, 0.0, CL), ok], None), "entry 2: layer 0: clip 0 is unknown or destroyed"),       # an inactive layer's clip is checked too
               ((GROUND, [ok, ok, (gone, 0.1, 0.0, CL)], None), f"entry 2: layer 2: clip {gone} is unknown or destroyed"),
               ((GROUND, [ok, (wide, 0.1, 0.0, CL)], None), f"entry 2: layer 1: clip {wide} animates 1024 joints, object {GROUND}'s skeleton has 2"),
               ((TRI, [ok], None), f"entry 2: object {TRI} has no skeleton"),
               ((99, [ok], None), "entry 2: object 99 out of range"),
               ((GROUND, [], None), "entry 2: n_layers 0 outside [1, 4]"),
               ((GROUND, [ok] * 5, None), "entry 2: n_layers 5 outside [1, 4]"),
               ((GROUND, None, None), "entry 2: layers is null"),
               ((GROUND, [ok, (g2, np.nan, 1.0, CL)], None), "entry 2: layer 1: time is not finite"),
               ((GROUND, [(g2, np.inf, 0.0, CL), ok], None), "entry 2: layer 0: time is not finite"),
               ((GROUND, [ok, (g2, 0.1, np.nan, CL)], None), "entry 2: layer 1: weight is not finite"),
               ((GROUND, [ok, ok, ok, (g2, 0.1, np.inf, CL)], None), "entry 2: layer 3: weight is not finite"),
               ((GROUND, [ok, (g2, 0.1, -0.5, CL)], None), "entry 2: layer 1: weight -0.5"),
               ((GROUND, [(g, 0.1, 0.0, LO), (g2, 0.1, 0.0, CL)], None), "entry 2: no layer has a weight above zero"),
               ((GROUND, [(g, 0.1, 3e38, LO), (g2, 0.1, 3e38, CL)], None), "entry 2: the sum of the layers' weights is not finite"),
               ((GROUND, [ok, (g2, 0.1, 1.0, 3)], None), "entry 2: layer 1: wrap mode 3 is none of CLAMP, LOOP, PINGPONG"),
               ((GROUND, [ok], np.float32([0.5])), f"entry 2: object {GROUND} has no morph targets"),
               ((BIG, [(rigs[BIG][2][0], 0.1, 1.0, CL)], None), "entries 0 and 2 both name object 0"),
               ((STRIP255, [(far_handle, 0.0, 1.0, LO)], None), f"entry 2: object {STRIP255}: a joint matrix of the blended layers is not finite"),
               ((STRIP255, [(far_handle, 0.0, 1.0, CL), (far_handle, 5.0, 1.0, PP)], None), f"entry 2: object {STRIP255}: a joint matrix of the blended layers is not finite")]
    for bad, text in refused:
        with pytest.raises(P.DeviceError) as e:
            r.animate_layers(good + [bad])
        assert e.value.code == N.CGPT_ERR_INVALID and text in str(e.value), (text, str(e.value))
        assert np.array_equal(bits(r.temporal_history()), bits(history))      # the generations move once a call is accepted
    L = N.lib()
    assert L.cgpt_scene_animate_layers(r._ctx, None, 3) == N.CGPT_ERR_INVALID and "entries is null" in L.cgpt_last_error(r._ctx).decode()
    one = (N.ClipLayer * 1)(N.ClipLayer(rigs[BIG][2][0], 0.1, 1.0, CL))
    row = N.LayeredAnimation(BIG, 1, one, 3, None)
    assert L.cgpt_scene_animate_layers(r._ctx, (N.LayeredAnimation * 1)(row), 1) == N.CGPT_ERR_INVALID and "entry 0: weights is null" in L.cgpt_last_error(r._ctx).decode()
    assert L.cgpt_scene_animate_layers(r._ctx, None, 0) == N.CGPT_OK and L.cgpt_scene_animate_layers(None, None, 0) == N.CGPT_ERR_INVALID
    b = C.c_float()
    assert L.cgpt_clip_get_range(r._ctx, gone, C.byref(b), None) == N.CGPT_ERR_INVALID and f"clip {gone} is unknown or destroyed" in L.cgpt_last_error(r._ctx).decode()
    assert L.cgpt_clip_get_range(r._ctx, g, None, None) == N.CGPT_OK and L.cgpt_clip_get_range(None, g, None, None) == N.CGPT_ERR_INVALID
    with pytest.raises(P.DeviceError, match="has not been posed"):
        r.joint_matrices(STRIP255)
    # nothing moved: records, frames, history, the skins' last poses
    assert np.array_equal(bits(r.temporal_history()), bits(history))
    assert all(np.array_equal(r.export_bvh(obj), t) for obj, t in zip(MESHES, trees))
    assert_same_frames(frames(r, sizes=SIZE, configs=cfg), before)
    assert all(np.array_equal(bits(r.joint_matrices(obj)), bits(m)) for obj, m in kept.items())
    outs = []
    for ctx in (r, want):                                                     # the next flagged call still uses its history, as the twin's that saw no refusal
        ctx.reset_accumulator(); ctx.render(64, 64, 2)
        outs.append(ctx.denoise_temporal_following(iterations=1, poses=True, morphs=True))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(bits(r.temporal_history()), bits(want.temporal_history())) and np.any(r.temporal_history()[..., 3] > 2)
    anim, posed = entries_at(rigs, cases, 0.6, shift=4)                       # and the next valid call works
    r.animate_layers(anim); want.pose_objects(posed)
    assert_same_scene(r, want, configs=KERNELS[1:2], tops=(False,))
    fresh_ctx = P.Renderer(0)
    with pytest.raises(P.DeviceError, match="no scene uploaded") as e:
        fresh_ctx.animate_layers(good)
    assert e.value.code == N.CGPT_ERR_NO_SCENE
    fresh_ctx.close()


# ---- 6. an instanced upload -----------------------------------------------------------------------------------------------------
def test_an_entry_through_one_placement_moves_every_instance():
    big = standin_mesh(2)
    tris = P.triangles_from_arrays(*big)
    shift = lambda x: np.float32([[1, 0, 0, x], [0, 1, 0, 0.2], [0, 0, 1, 0.0]])
    s = make_scene(big, octahedron((2.0, 1.0, -1.0), 0.7))
    twins = [s.add_instance(BIG, 1, transform=shift(x), smooth=bool(k)) for k, x in enumerate((-2.5, 2.5))]
    r, want = P.Renderer(0), P.Renderer(0)
    r.upload(s, instanced=True); want.upload(s, instanced=True)
    j, sw, n_joints, _ = skin_case("bend", tris)
    base, d, w = morph_case("mix", tris)
    skeleton, clips = clips_of(2, 31, "chain", False)
    for ctx in (r, want):
        ctx.set_skin(twins[1], tris, j, sw, n_joints)
        ctx.set_skin(twins[0], tris, j, sw, n_joints)
        ctx.set_morph_targets(twins[1], base, d)
    rig = (skeleton, clips, [r.create_clip(*c) for c in clips])
    r.set_skeleton(twins[0], *skeleton); r.set_skeleton(twins[1], *skeleton)
    dev, host = layers_of(rig, PATTERNS[3], 0.3)
    r.animate_layers([(twins[1], dev, w)]); want.pose_objects([(twins[1], P.animate_layers(skeleton, host), w)])
    for top in (False, True):
        r.set_top_level(top); want.set_top_level(top)
        assert_same_frames(frames(r, sizes=SIZE, configs=KERNELS[1:3]), frames(want, sizes=SIZE, configs=KERNELS[1:3]))
    assert np.array_equal(r.export_bvh(BIG), want.export_bvh(twins[0])) and not np.array_equal(r.export_bvh(BIG), s.bvh_export(BIG)[0])
    before = r.export_bvh(BIG)
    with pytest.raises(P.DeviceError, match=f"entries 0 and 1 name objects {twins[0]} and {twins[1]} of one instanced mesh group") as e:
        r.animate_layers([(twins[0], dev, None), (twins[1], dev, None)])
    assert e.value.code == N.CGPT_ERR_INVALID and np.array_equal(r.export_bvh(BIG), before)
    r.close(); want.close(); s.close()


# ---- 7. a two-member context ----------------------------------------------------------------------------------------------------
def test_a_multi_device_context_blends_on_every_member(world):
    s, binds = world
    g, one = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY), fresh(s)
    cases = install(g, binds)
    install(one, binds)
    rigs = rig_up(g)
    anim, posed = entries_at(rigs, cases, 0.25, shift=1)
    g.animate_layers(anim); one.pose_objects(posed)
    for obj in MESHES:
        assert np.array_equal(g.export_bvh(obj), one.export_bvh(obj))
    assert np.array_equal(bits(g.joint_matrices(OCTA)), bits(posed[2][1]))
    assert np.array_equal(bits(g.clip_range(rigs[BIG][2][1])), bits(clip_range(rigs[BIG][1][1])))
    cfg = [(P.KERNEL_WAVEFRONT, None), (P.KERNEL_PERSISTENT, None)]
    for top in (False, True):                                                 # the members render half the rows each
        g.set_top_level(top); one.set_top_level(top)
        assert_same_frames(frames(g, sizes=SIZE, configs=cfg), frames(one, sizes=SIZE, configs=cfg))
    with pytest.raises(P.DeviceError, match="layer 0: clip 77 is unknown or destroyed"):
        g.animate_layers([(BIG, [(77, 0.0, 1.0, CL)], None)])
    g.destroy_clip(rigs[BIG][2][0])
    with pytest.raises(P.DeviceError, match="unknown or destroyed"):
        g.animate_layers(entries_at(rigs, cases, 0.25)[0])
    assert np.array_equal(g.export_bvh(BIG), one.export_bvh(BIG))
    g.close(); one.close()


# ---- 8. a caller's stream -------------------------------------------------------------------------------------------------------
def test_a_call_on_a_callers_stream_equals_the_own_stream_result(pair):
    import torch
    s, binds, r, want = pair
    cases = install(r, binds)
    install(want, binds)
    rigs = rig_up(r)
    side = torch.cuda.Stream()
    r.set_stream(side)
    for t in (0.2, 0.45):
        anim, posed = entries_at(rigs, cases, t, shift=5)
        r.animate_layers(anim); want.pose_objects(posed)
    for obj, m, _ in posed:
        assert np.array_equal(bits(r.joint_matrices(obj)), bits(m))
    assert_same_scene(r, want, configs=KERNELS[1:2], tops=(False,))
    r.set_stream(None)


# ---- 9. the example program -----------------------------------------------------------------------------------------------------
def test_render_main_loops_and_cross_fades_the_bend(tmp_path):
    import os
    import subprocess
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    frames_at = {}
    runs = (("--animate", "0.25"), ("--animate", "2.25", "--loop"), ("--animate", "0.25", "--crossfade", "0"), ("--animate", "0.25", "--crossfade", "0.5"),
            ("--crowd", "3", "--animate", "1.5", "--loop", "--crossfade", "0.9"))
    for args in runs:
        out = subprocess.run([exe, "--bend", "30", *args, "64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert ("clip range [0, 1]" in out.stdout) == ("--loop" in args or "--crossfade" in args), out.stdout
        frames_at[args] = (tmp_path / "animate_00_raw.ppm").read_bytes()
    plain, looped, faded_0, faded_half, crowd = (frames_at[a] for a in runs)
    assert looped == plain                                                    # 2.25 wraps to 0.25 over [0, 1]: the same frame to the byte
    assert faded_0 == plain                                                   # weights (1, 0): the bend clip alone
    assert faded_half != plain and crowd != plain and crowd != faded_half     # half of each bend is another pose; a crowd is another scene
