"""CPU checks of tests/edit_model.py: the model against the host mirrors on hand-written sequences, the generator's
determinism, what the default sequences of tests/test_gpu_edit_sequences.py cover, and that they tell nine wrong models from the right
one.  No GPU is touched: the sequences are only applied to models."""
import functools

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import anim_cases
import edit_model as E
import morph_cases
import skin_cases
from edit_model import BIG, GROUND, LAMP, OCTA, STRIP255, STRIP256, STRIP257, SUN, TRI, WALL, Model, apply_to_model


@functools.lru_cache(maxsize=None)
def default_sequences():
    """((kind, context, seed, steps), operations) of the default set, generated once"""
    return tuple((spec, E.sequence_of(*spec)) for spec in E.default_set())


def run(model, ops):
    return [apply_to_model(model, op) for op in ops]


def final_bytes(kind, ops, mutant=None):
    m = Model(kind, mutant)
    run(m, ops)
    out = m.scene_bytes()
    m.close()
    return out


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_operations_and_the_same_scene():
    for spec, ops in default_sequences():
        again = E.sequence_of(*spec)
        assert len(again) == len(ops) == spec[3] and all(E.same_operation(a, b) for a, b in zip(ops, again)), spec
        assert final_bytes(spec[0], ops) == final_bytes(spec[0], again), spec
    a, b = E.random_sequence(1, 16, "plain"), E.random_sequence(2, 16, "plain")
    assert not all(E.same_operation(x, y) for x, y in zip(a, b))
    for ops in (a, b):
        assert not any(E.same_operation(x, y) for x, y in zip(ops, ops[1:]))  # never a pure repeat of the previous operation


# ---- hand-written sequences against the mirrors --------------------------------------------------------------------------------------
class Hand:
    """a plain model with two skins and two sets of targets for the octahedron at hand"""
    def __init__(self, kind="plain", obj=OCTA):
        self.m = Model(kind)
        self.obj = obj
        self.bind = self.m.binds[obj]
        self.j, self.sw, self.n, self.M = skin_cases.make_case("bend", self.bind, seed=1)
        self.j2, self.sw2, self.n2, self.M2 = skin_cases.make_case("four", self.bind, seed=2)
        self.half = skin_cases.make_case("half", self.bind, seed=3)[3]         # another pose of the two-joint skin
        self.base, self.d, self.w = morph_cases.make_case("mix", self.bind, seed=4)
        self.base2, self.d2, self.w2 = morph_cases.make_case("zeros_among", self.bind, seed=5)
        self.set_skin = ("set_skin", obj, self.bind, self.j, self.sw, self.n)
        self.set_skin2 = ("set_skin", obj, self.bind, self.j2, self.sw2, self.n2)
        self.set_morph = ("set_morph_targets", obj, self.base, self.d)
        self.set_morph2 = ("set_morph_targets", obj, self.base2, self.d2)

    def skin(self, b, M=None):
        return P.skin_triangles(b, self.j, self.sw, self.M if M is None else M)

    def morph(self, w=None):
        return P.morph_triangles(self.base, self.d, self.w if w is None else w)

    def expect(self, ops, tris, statuses=None):
        got = run(self.m, ops)
        assert got == (statuses or ["accepted"] * len(ops)), got
        now = self.m.tris[self.obj]
        assert np.array_equal(now.view(np.uint32), np.ascontiguousarray(tris, np.float32).view(np.uint32))
        twin = Model(self.m.kind)                                              # ... and the scene is a refit of exactly those triangles
        twin.scene.refit_mesh(self.obj, tris)
        assert E.scene_words(self.m.scene)[0][self.obj] == E.scene_words(twin.scene)[0][self.obj]
        twin.close()

    def close(self):
        self.m.close()


@pytest.fixture()
def h():
    hand = Hand()
    yield hand
    hand.close()


def test_a_pose_is_always_from_the_bind_pose_or_the_base(h):
    o = h.obj
    h.expect([h.set_skin], h.bind)                                            # the scene does not change until the first pose
    h.expect([("skin_mesh", o, h.M)], h.skin(h.bind))
    h.expect([("skin_mesh", o, h.half)], h.skin(h.bind, h.half))              # not from the current triangles
    h.expect([("skin_mesh", o, h.M)], h.skin(h.bind))                         # A, B, A leaves A
    h.expect([("clear_skin", o)], h.skin(h.bind))                             # the geometry stays where it is
    h.expect([h.set_morph, ("morph_mesh", o, h.w), ("morph_mesh", o, h.w * np.float32(0.5))], h.morph(h.w * np.float32(0.5)))


def test_the_morphed_base_is_the_skins_bind_pose_in_either_call_order(h):
    o = h.obj
    h.expect([h.set_skin, h.set_morph, ("skin_mesh", o, h.M)], h.skin(h.base))   # w_last is zeros before the first morph
    h.expect([("morph_mesh", o, h.w)], h.skin(h.morph()))
    h.expect([("skin_mesh", o, h.half)], h.skin(h.morph(), h.half))
    other = Hand()
    other.expect([other.set_morph, other.set_skin, ("morph_mesh", o, other.w)], other.morph())   # the morph alone while the skin has not been posed
    other.expect([("skin_mesh", o, other.half)], other.skin(other.morph(), other.half))
    other.close()


def test_a_refit_keeps_skin_and_targets_and_the_next_pose_starts_from_the_base_again(h):
    o = h.obj
    moved = h.bind.copy(); moved[:, 0::6] += np.float32(0.4)
    h.expect([h.set_skin, h.set_morph, ("morph_mesh", o, h.w), ("skin_mesh", o, h.M)], h.skin(h.morph()))
    h.expect([("refit_mesh", o, moved)], moved)
    assert np.float32(h.m.last_area).view(np.uint32) == np.float32(h.m.scene.bvh_info(o).total_area).view(np.uint32)
    h.expect([("skin_mesh", o, h.half)], h.skin(h.morph(), h.half))
    h.expect([("refit_mesh", o, moved), ("morph_mesh", o, h.w2[:3])], h.skin(h.morph(h.w2[:3]), h.half))


def test_set_skin_forgets_the_pose_and_drops_the_skeleton(h):
    o = h.obj
    skeleton, clip, _ = anim_cases.rig(h.n, 3, "chain")
    ops = [h.set_skin, h.set_morph, ("create_clip", 0) + tuple(clip), ("set_skeleton", o) + tuple(skeleton), ("animate_objects", [(o, 0, 0.4, h.w)])]
    h.expect(ops, h.skin(h.morph(), P.animate_joints(skeleton, clip, 0.4)))
    assert np.array_equal(h.m.posed_skins()[o].view(np.uint32), P.animate_joints(skeleton, clip, 0.4).view(np.uint32))
    same_count = ("set_skin", o, h.bind, *skin_cases.make_case("half", h.bind, seed=9)[:3])
    h.expect([same_count, ("morph_mesh", o, h.w)], h.morph())                 # a replaced skin of the same joint count: no matrices kept
    assert o not in h.m.posed_skins()
    before = h.m.state_bytes()
    h.expect([("animate_objects", [(o, 0, 0.4, None)])], h.morph(), ["refused"])   # the skeleton went with the skin
    assert h.m.state_bytes() == before and h.m.last_refusal == "no_skin_or_targets"
    h.expect([h.set_skin2, ("morph_mesh", o, h.w)], h.morph())                # ... and of another joint count


def test_set_morph_targets_resets_the_weights_and_clear_gives_the_skin_its_own_bind_pose_back(h):
    o = h.obj
    h.expect([h.set_skin, h.set_morph, ("morph_mesh", o, h.w), ("skin_mesh", o, h.M)], h.skin(h.morph()))
    again = ("set_morph_targets", o, h.base, h.d * np.float32(2.0))           # as many targets as before
    h.expect([again], h.skin(h.morph()))                                      # installing changes nothing
    h.expect([("skin_mesh", o, h.half)], h.skin(h.base, h.half))              # zeros, not the old weights
    h.expect([("morph_mesh", o, h.w)], h.skin(P.morph_triangles(h.base, h.d * np.float32(2.0), h.w), h.half))
    kept = h.m.tris[o].copy()
    h.expect([("clear_morph_targets", o)], kept)                              # the geometry stays where it is
    h.expect([("skin_mesh", o, h.M)], h.skin(h.bind))                         # the skin's own bind pose, not the morphed base
    h.expect([h.set_morph2, ("morph_mesh", o, h.w2), ("clear_skin", o)], h.skin(P.morph_triangles(h.base2, h.d2, h.w2)))
    h.expect([("morph_mesh", o, h.w2 * np.float32(0.5))], P.morph_triangles(h.base2, h.d2, h.w2 * np.float32(0.5)))   # the morph alone


def test_a_batch_is_morph_mesh_then_skin_mesh_of_every_entry_and_takes_what_is_left_out_from_the_last_pose(h):
    o = h.obj
    h.expect([h.set_skin, h.set_morph, ("pose_objects", [(o, h.M, h.w)])], h.skin(h.morph()))
    h.expect([("pose_objects", [(o, None, h.w * np.float32(0.5))])], h.skin(h.morph(h.w * np.float32(0.5))))   # the matrices of the last pose
    h.expect([("pose_objects", [(o, h.half, None)])], h.skin(h.morph(h.w * np.float32(0.5)), h.half))         # the weights of the last morph
    h.expect([("morph_mesh", o, h.w)], h.skin(h.morph(), h.half))                                             # the single calls pick up what a batch left
    before = h.m.state_bytes()
    for bad, kind in (([(o, h.M, None), (o, h.half, None)], "named_twice"), ([(o, h.M, None), (99, h.M, None)], "out_of_range"),
                      ([(o, h.M[:1], None)], "matrix_count"), ([(o, None, h.w[:2])], "weight_count"), ([(GROUND, h.M, None)], "no_skin_or_targets"),
                      ([(o, None, None)], "no_skin_or_targets"), ([(o, np.full_like(h.M, np.inf), None)], "not_finite")):
        assert apply_to_model(h.m, ("pose_objects", bad)) == "refused" and h.m.last_refusal == kind, kind
        assert h.m.state_bytes() == before                                    # a refused call changes nothing


def test_the_batch_tests_sequences_restated_as_operations():
    """test_gpu_pose_batch.test_a_batch_equals_the_single_calls_in_any_order_and_state, on two models: batches against single calls"""
    from test_gpu_pose_batch import RECIPE, eased
    batch, single = Model("plain"), Model("plain")
    cases, install = {}, []
    for obj, (pose, morph, leaf) in RECIPE.items():
        c = dict(m=None, w=None)
        if morph:
            base, d, c["w"] = morph_cases.make_case(morph, batch.binds[obj], seed=obj)
            install += [("set_tuning", "morph_leaf_order", leaf), ("set_morph_targets", obj, base, d)]
        if pose:
            j, sw, n_joints, c["m"] = skin_cases.make_case(pose, batch.binds[obj], seed=obj)
            install.append(("set_skin", obj, batch.binds[obj], j, sw, n_joints))
        cases[obj] = c
    full = [(obj, c["m"], c["w"]) for obj, c in cases.items()]
    again = eased(cases, 0.5)
    partial = [(BIG, None, again[BIG]["w"]), (STRIP256, again[STRIP256]["m"], None), (TRI, None, np.zeros(3, np.float32))]
    some = [(GROUND, again[GROUND]["m"], None), (STRIP257, again[STRIP257]["m"], None)]
    last = eased(cases, 0.25)
    tail = [("skin_mesh", STRIP256, last[STRIP256]["m"]), ("morph_mesh", BIG, last[BIG]["w"]), ("pose_objects", [(STRIP255, None, np.float32([-0.0]))]), ("pose_objects", [])]
    steps = [(full, full), (partial, partial), ([(OCTA, again[OCTA]["m"], None)], None), ([(STRIP255, None, again[STRIP255]["w"])], None), (full[::-1], full), (some, some)]

    def one_by_one(entries):
        return [op for obj, m, w in entries for op in ([("morph_mesh", obj, w)] if w is not None else []) + ([("skin_mesh", obj, m)] if m is not None else [])]
    assert set(run(batch, install) + run(single, install)) == {"accepted"}
    for entries, singles in steps:
        assert set(run(batch, [("pose_objects", entries)])) == {"accepted"}
        assert set(run(single, one_by_one(singles if singles is not None else entries))) == {"accepted"}
        assert batch.state_bytes() == single.state_bytes()
    assert set(run(batch, tail) + run(single, tail)) == {"accepted"} and batch.state_bytes() == single.state_bytes()
    assert np.array_equal(batch.tris[STRIP255].view(np.uint32), batch.binds[STRIP255].view(np.uint32))   # an all-zero entry leaves the base, bit for bit
    batch.close(); single.close()


def test_a_rebuild_is_the_mirrors_rebuild_over_the_current_triangles_and_keeps_skins_and_targets(h):
    o = h.obj
    ops = [h.set_skin, h.set_morph, ("skin_mesh", o, h.M), ("rebuild_mesh", o, P.BUILD_NAIVE), ("morph_mesh", o, h.w), ("rebuild_mesh", o, P.BUILD_SAH_BINNED)]
    h_twin = Model("plain")
    h_twin.scene.refit_mesh(o, h.skin(h.base)); h_twin.scene.rebuild_bvh(o, P.BUILD_NAIVE)
    h_twin.scene.refit_mesh(o, h.skin(h.morph())); h_twin.scene.rebuild_bvh(o, P.BUILD_SAH_BINNED)
    assert run(h.m, ops) == ["accepted"] * 6
    assert E.scene_words(h.m.scene)[0][o] == E.scene_words(h_twin.scene)[0][o]
    assert E.scene_words(h.m.scene)[0][o] != h.m.uploaded[o] and h.m.differing_meshes() == [o]
    before = h.m.state_bytes()
    for obj in (TRI, SUN, WALL, 10):                                          # a triangle object, a sphere, a plane, no object
        assert apply_to_model(h.m, ("rebuild_mesh", obj, P.BUILD_NAIVE)) == "refused" and h.m.state_bytes() == before
    h_twin.close()


def test_an_upload_drops_skins_targets_and_skeletons_and_keeps_clips_the_switch_and_tuning(h):
    o = h.obj
    skeleton, clip, _ = anim_cases.rig(h.n, 3, "chain")
    ops = [("set_top_level", True), ("set_tuning", "morph_leaf_order", 0), ("create_clip", 0) + tuple(clip), h.set_skin, h.set_morph, ("set_skeleton", o) + tuple(skeleton),
           ("animate_objects", [(o, 0, 0.2, h.w)]), ("upload",)]
    posed = h.skin(h.morph(), P.animate_joints(skeleton, clip, 0.2))
    h.expect(ops, posed)                                                      # the geometry is the scene's: an upload keeps it
    assert not h.m.skins and not h.m.morphs and h.m.top_level and h.m.tuning["morph_leaf_order"] == 0 and h.m.clips[0] is not None
    h.expect([("skin_mesh", o, h.M), ("morph_mesh", o, h.w), ("set_skeleton", o) + tuple(skeleton)], posed, ["refused"] * 3)
    h.expect([h.set_skin, ("animate_objects", [(o, 0, 0.2, None)])], posed, ["accepted", "refused"])   # a new skin has no skeleton yet
    h.expect([("set_skeleton", o) + tuple(skeleton), ("animate_objects", [(o, 0, 0.7, None)])], h.skin(h.bind, P.animate_joints(skeleton, clip, 0.7)))
    h.expect([("destroy_clip", 0), ("animate_objects", [(o, 0, 0.7, None)])], h.skin(h.bind, P.animate_joints(skeleton, clip, 0.7)), ["accepted", "refused"])
    assert h.m.last_refusal == "destroyed_clip"


def test_an_edit_through_one_placement_moves_every_placement_of_the_copy():
    hand = Hand("instanced", obj=11)                                          # the second placement of the octahedron
    m = hand.m
    assert m.members(11) == [OCTA, 10, 11] and m.members(STRIP256) == [STRIP256, 12, 13] and m.members(BIG) == [BIG]
    hand.expect([hand.set_skin, ("skin_mesh", 11, hand.M)], hand.skin(hand.bind))
    words = E.scene_words(m.scene)[0]
    for k in (OCTA, 10):
        assert np.array_equal(m.tris[k], m.tris[11]) and words[k][1] == words[11][1] and words[k] != m.uploaded[k]
    assert apply_to_model(m, ("pose_objects", [(11, hand.M, None), (GROUND, None, None)])) == "refused"
    assert apply_to_model(m, ("set_skin", 10, hand.bind, hand.j, hand.sw, hand.n)) == "accepted"
    assert apply_to_model(m, ("pose_objects", [(11, hand.M, None), (10, hand.half, None)])) == "refused" and m.last_refusal == "named_twice"
    assert apply_to_model(m, ("rebuild_mesh", 10, P.BUILD_NAIVE)) == "accepted"
    assert [E.scene_words(m.scene)[0][k][1] for k in (OCTA, 10)] == [E.scene_words(m.scene)[0][11][1]] * 2
    hand.close()


def test_the_other_edits_go_through_the_scenes_own_setters():
    m = Model("plain")
    xf = np.tile(E.IDENTITY, (m.n_objects, 1)); xf[BIG] = np.float32([0.9, 0, 0.1, 0.2, 0, 1.1, 0, -0.1, -0.1, 0, 0.9, 0.3])
    mats = list(m.materials); mats[0] = P.Material(albedo=(0.9, 0.3, 0.2), specular=0.2, roughness=0.3)
    smooth = np.zeros(m.n_objects, np.uint32); smooth[[BIG, TRI]] = 1
    ops = [("update_transforms", xf), ("update_materials", mats), ("update_roughness", np.float32([0.3, 0.5, 0, 0, 0])), ("update_transmission_roughness", np.float32([0, 0, 0, 0.25, 0])),
           ("update_smooth_normals", smooth), ("update_primitive", SUN, 2, dict(center=(-6.0, 9.0, 4.0), radius=3.5)),
           ("update_primitive", WALL, 1, dict(normal=(0.0, 0.6, 0.8), point=(0.0, 0.0, -12.0)))]
    states = [m.state_bytes()]
    for op in ops:
        assert apply_to_model(m, op) == "accepted"
        states.append(m.state_bytes())
    assert len(set(states)) == len(states)                                    # each of them is visible in the scene's bytes
    assert np.array_equal(m.scene.transforms()[BIG].ravel(), xf[BIG]) and m.scene.roughness().tolist() == [np.float32(0.3), 0.5, 0, 0, 0]
    assert m.scene.transmission_roughness()[3] == 0.25 and m.scene.smooth_normals().tolist() == smooth.tolist()
    assert tuple(m.scene.flatten().objects[SUN].sphere_center) == (-6.0, 9.0, 4.0)
    m.close()


# ---- what the default sequences cover -------------------------------------------------------------------------------------------------
PAIRS = ("rebuild>morph_mesh/leaf0", "rebuild>morph_mesh/leaf1", "rebuild>skin_mesh", "rebuild>refit>rebuild_other_option", "set_morph_targets>skin_mesh",
         "clear_morph_targets>skin_mesh", "refit>skin_mesh", "set_skin_of_another_joint_count>morph_mesh", "clear_skin>morph_mesh",
         "animate>entry_with_weights_only", "animate>skin_mesh", "upload>set_skin+set_skeleton+animate_with_an_older_clip", "update_transforms>pose_under_top_level",
         "refused_batch>accepted_batch_over_the_same_objects")


def analyse(kind, ops, knobs=None):
    """what one sequence covers: accepted operations by kind, refusal kinds, steps refused or without effect, the share of mesh objects
    that differ from the upload at the end, and the ordered pairs of PAIRS that occur on one object with no other geometry edit of that
    object in between.  A geometry edit is a refit, a rebuild or a pose; the rest (set_skin, clear_*, update_transforms, ...) are marks."""
    m = Model(kind)
    m.tuning.update(knobs or {})
    accepted, refusals, pairs, weak = {}, set(), set(), 0
    geo = {}                                                                   # group -> [(event, detail, step)] geometry edits of its copy
    marks = {}                                                                 # group -> [(mark, object)] since its last geometry edit
    morph_at, morph_leaf, skin_at, clip_at = {}, {}, {}, {}
    upload_at, refused_batch = -1, None
    for i, op in enumerate(ops):
        name = op[0]
        before = m.state_bytes()
        had_skin = {o: s["n_joints"] for o, s in m.skins.items()}
        had_morph = set(m.morphs)
        status = apply_to_model(m, op)
        if status == "refused":
            refusals.add(m.last_refusal)
            weak += 1
            refused_batch = (i, {m.group[e[0]] for e in op[1] if 0 <= e[0] < m.n_objects}) if name in ("pose_objects", "animate_objects") else None
            continue
        accepted[name] = accepted.get(name, 0) + 1
        weak += m.state_bytes() == before

        def last(g, n=1):
            return [e[:2] for e in geo.get(g, [])[-n:]]

        def posed(obj, event, entry=None):
            g = m.group[obj]
            mine = [mark for mark, o in marks.get(g, []) if o == obj]
            was = last(g)[0] if last(g) else (None, None)
            if event == "skin_mesh":
                pairs.update(p for p, hit in (("rebuild>skin_mesh", was[0] == "rebuild"), ("refit>skin_mesh", was[0] == "refit"), ("animate>skin_mesh", was[0] == "animate"),
                                              ("set_morph_targets>skin_mesh", "set_morph_targets" in mine), ("clear_morph_targets>skin_mesh", "clear_morph_targets" in mine)) if hit)
            if event == "morph_mesh":
                if was[0] == "rebuild" and obj in morph_at and morph_at[obj] < geo[g][-1][2]:
                    pairs.add(f"rebuild>morph_mesh/leaf{morph_leaf[obj]}")
                pairs.update(p for p, hit in (("set_skin_of_another_joint_count>morph_mesh", "set_skin_other" in mine), ("clear_skin>morph_mesh", "clear_skin" in mine)) if hit)
            if event == "entry" and entry[1] is None and entry[2] is not None and was[0] == "animate":
                pairs.add("animate>entry_with_weights_only")
            if event == "animate" and obj in skin_at and clip_at.get(entry[1], i) < upload_at < skin_at[obj] and (not geo.get(g) or geo[g][-1][2] < upload_at):
                pairs.add("upload>set_skin+set_skeleton+animate_with_an_older_clip")
            if m.top_level and "update_transforms" in [mark for mark, _ in marks.get(g, [])]:
                pairs.add("update_transforms>pose_under_top_level")
            geo.setdefault(g, []).append((event, None, i))
            marks[g] = []

        def mark(obj, what):
            marks.setdefault(m.group[obj], []).append((what, obj))

        if name == "refit_mesh":
            geo.setdefault(m.group[op[1]], []).append(("refit", None, i)); marks[m.group[op[1]]] = []
        elif name == "rebuild_mesh":
            g = m.group[op[1]]
            if last(g, 2) and [e[0] for e in last(g, 2)] == ["rebuild", "refit"] and last(g, 2)[0][1] != op[2]:
                pairs.add("rebuild>refit>rebuild_other_option")
            geo.setdefault(g, []).append(("rebuild", op[2], i)); marks[g] = []
        elif name in ("skin_mesh", "morph_mesh"):
            posed(op[1], name)
        elif name in ("pose_objects", "animate_objects"):
            for e in op[1]:
                posed(e[0], "entry" if name == "pose_objects" else "animate", e)
            if refused_batch and refused_batch[0] == i - 1 and refused_batch[1] == {m.group[e[0]] for e in op[1]}:
                pairs.add("refused_batch>accepted_batch_over_the_same_objects")
        elif name == "set_morph_targets":
            morph_at[op[1]], morph_leaf[op[1]] = i, m.tuning["morph_leaf_order"]
            mark(op[1], "set_morph_targets")
        elif name == "clear_morph_targets" and op[1] in had_morph:
            morph_at.pop(op[1], None)
            mark(op[1], "clear_morph_targets")
        elif name == "set_skin":
            skin_at[op[1]] = i
            mark(op[1], "set_skin_other" if had_skin.get(op[1], op[5]) != op[5] else "set_skin")
        elif name == "clear_skin" and op[1] in had_skin:
            mark(op[1], "clear_skin")
        elif name == "update_transforms":
            for k in range(m.n_objects):
                mark(k, "update_transforms")
        elif name == "upload":
            upload_at = i
            morph_at.clear(); skin_at.clear()
        elif name == "create_clip":
            clip_at[op[1]] = i
        refused_batch = None
    share = len(m.differing_meshes()) / len(m.mesh_objects())
    m.close()
    return dict(accepted=accepted, refusals=refusals, pairs=pairs, weak=weak, share=share)


@functools.lru_cache(maxsize=None)
def default_coverage():
    return tuple((spec, analyse(spec[0], ops, E.SLOW_KNOBS if spec[1] == "knobs" else None)) for spec, ops in default_sequences())


def test_every_operation_is_accepted_three_times_and_every_refusal_occurs():
    accepted, refusals = {}, set()
    for _, c in default_coverage():
        for name, n in c["accepted"].items():
            accepted[name] = accepted.get(name, 0) + n
        refusals |= c["refusals"]
    assert set(accepted) == set(E.OP_KINDS), set(E.OP_KINDS) - set(accepted)
    assert min(accepted.values()) >= 3, {k: v for k, v in accepted.items() if v < 3}
    assert refusals == set(E.REFUSAL_KINDS), set(E.REFUSAL_KINDS) - refusals


def test_every_sequence_mostly_edits_and_leaves_half_of_its_meshes_changed():
    for spec, c in default_coverage():
        assert 4 * c["weak"] <= spec[3], (spec, c["weak"])                     # at most a quarter refused or without effect
        assert c["share"] >= 0.5, (spec, c["share"])


def test_every_ordered_pair_occurs_on_one_object_with_no_other_geometry_edit_in_between():
    pairs = set()
    for _, c in default_coverage():
        pairs |= c["pairs"]
    assert pairs == set(PAIRS), set(PAIRS) - pairs


# ---- telling wrong rules apart ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_the_default_sequences_tell_a_wrong_model_from_the_right_one(mutant):
    """a mutant no sequence can tell apart names a rule the fuzz cannot check"""
    kinds = ("instanced",) if mutant == "one_placement_only" else E.SCENE_KINDS
    told = [spec for spec, ops in default_sequences() if spec[0] in kinds and final_bytes(spec[0], ops, mutant) != final_bytes(spec[0], ops)]
    assert told, mutant
