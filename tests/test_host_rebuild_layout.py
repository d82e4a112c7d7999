"""CPU tests of the host half of cgpt_scene_rebuild_mesh (csrc/device/rebuild_layout.hip, seen through cgpth_rebuild_plan)
against tests/rebuild_ref.py, which restates rebuild_layout.h's rules in numpy: where the span of a rebuilt mesh goes at a first and at a
later rebuild, the refit levels from the builder's level ranges, which records take the mesh's top slots, and the two refusals.  No GPU
is touched."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from rebuild_ref import LEAF_BIT, NO_SPAN, Book, Refused, chain_tree, complete_tree, rebuild, top_slots
from scenes import GROUND_I, GROUND_V
from test_host_scene_layout import Layout, Raw, new_scene

BIG, NAIVE, LEAFY, GROUND, TRI, SUN = range(6)


def scene(instances=False):
    """a tree above kTopRecords pairs, a second tree, a leaf-rooted mesh, the ground quad, a triangle object and a sphere light;
    instances: two more placements of BIG"""
    s = new_scene()
    assert s.add_mesh(P.Mesh.dragon_standin(2), 3, P.BUILD_SAH_INTERVALS) == BIG
    assert s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_NAIVE) == NAIVE
    assert s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_SAH_PRIMITIVES) == LEAFY
    assert s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), 1, P.BUILD_SAH_INTERVALS) == GROUND
    assert s.add_triangle([[-1.0, 0.5, 2.0], [1.25, 0.5, 2.0], [0.0, 2.0, 2.5]], [0.0, 0.0, 1.0], 0) == TRI
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    if instances:
        s.add_instance(BIG, 1)
        s.add_instance(BIG, 0)
    return s


def words(trees):
    out = []
    for level_first, ranks in trees:
        out += [len(level_first)] + list(level_first) + [len(ranks)] + list(ranks)
    return np.asarray(out, np.uint32)


def plan(s, obj, trees, instanced=False, assume=0):
    """(status, message, view as a dict of numpy arrays and ints, Book before any rebuild)"""
    raw = Raw(s.flatten())
    desc, keep = raw.desc()
    lay_view = N.SceneLayoutView()
    call = N.lib().cgpth_scene_layout_instanced if instanced else N.lib().cgpth_scene_layout
    assert call(C.byref(desc), C.byref(lay_view)) == N.CGPT_OK
    lay = Layout(lay_view)
    group = None
    if instanced:
        first = {}
        group = [first.setdefault((o.node_offset, o.node_count, o.tri_offset, o.tri_count), i) if o.kind == N.OBJECT_MESH else i for i, o in enumerate(raw.objects)]
    book = Book(lay, raw, group)
    w = words(trees)
    v = N.RebuildPlanView()
    rc = N.lib().cgpth_rebuild_plan(C.byref(desc), int(instanced), obj, w.ctypes.data_as(C.POINTER(C.c_uint32)), len(trees), assume, C.byref(v))
    del keep
    msg = N.lib().cgpth_last_error().decode()
    if rc != N.CGPT_OK:
        return rc, msg, None, book
    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
    got = dict(members=arr(v.members, v.n_members), top_slots=arr(v.top_slots, v.n_top_slots), level_offsets=arr(v.level_offsets, v.n_level_offsets),
               names=arr(v.names, v.n_names), record_perm=arr(v.record_perm, v.n_record_perm), root_codes=arr(v.root_codes, v.n_objects),
               span_bases=arr(v.span_bases, v.n_objects), node_counts=arr(v.node_counts, v.n_objects))
    for k in ("span_base", "level_begin", "pair_base", "leaf_base", "n_nodes", "n_pairs", "max_depth", "grow", "n_pair_records", "n_refit_levels", "stack_depth", "n_top_records"):
        got[k] = getattr(v, k)
    return rc, msg, got, book


def spread_ranks(n_used, n_pairs, seed):
    """distinct ranks as a level-ordered array would give them: rank 0 (the root) first"""
    rng = np.random.default_rng(seed)
    rest = rng.permutation(np.arange(1, n_pairs))[:max(0, n_used - 1)]
    return ([0] + rest.tolist())[:n_used]


def check(s, obj, level_firsts, instanced=False, seed=3):
    """runs the rebuilds through the reference one by one to learn each K, then all of them through the library; compares everything"""
    _, _, _, book = plan(s, obj, [([0, 1], [])], instanced)               # only for the Book
    trees, want = [], None
    for t, lf in enumerate(level_firsts):
        k = min(len(top_slots(book, obj)), lf[-1] // 2)
        ranks = spread_ranks(k, lf[-1] // 2, seed + t)
        trees.append((lf, ranks))
        want = rebuild(book, obj, lf, ranks)
    rc, msg, got, _ = plan(s, obj, trees, instanced)
    assert rc == N.CGPT_OK, msg
    for key in ("members", "top_slots", "level_offsets", "names"):
        assert got[key].tolist() == list(want[key]), key
    for key in ("span_base", "level_begin", "pair_base", "n_nodes", "n_pairs", "max_depth", "grow", "n_pair_records", "n_refit_levels", "stack_depth"):
        assert got[key] == want[key], (key, got[key], want[key])
    assert got["record_perm"].tolist() == book.record_perm
    assert got["root_codes"].tolist() == book.root_code and got["span_bases"].tolist() == book.span_base
    meshes = [j for j, kind in enumerate(book.kind) if kind == N.OBJECT_MESH]
    assert [got["node_counts"][j] for j in meshes] == [book.node_count[j] for j in meshes]
    return got, want, book


def test_first_rebuild_moves_the_span_to_the_end_and_keeps_the_top_slots():
    s = scene()
    got, want, book = check(s, BIG, [complete_tree(9)])                       # 255 pairs: more than the slots BIG owns
    k = len(got["top_slots"])
    assert 0 < k < 255 and got["grow"] == 1 and got["n_top_records"] == 256
    raw = Raw(s.flatten())
    old_pairs = sum(o.node_count // 2 for o in raw.objects if o.kind == N.OBJECT_MESH)
    assert got["span_base"] == old_pairs and got["n_pair_records"] == old_pairs + 320 - 1
    assert got["level_offsets"].tolist() == [0, 1, 3, 7, 15, 31, 63, 127, 255]
    names = got["names"]
    assert sorted(names[names < 256].tolist()) == got["top_slots"].tolist()  # every slot taken, the others in the span by rank
    rest = np.flatnonzero(names >= 256)
    assert np.array_equal(names[rest], got["span_base"] + rest)
    assert got["root_codes"][BIG] == names[0] < 256
    s.close()


def test_fewer_splitting_nodes_than_slots_leaves_slots_unused():
    s = scene()
    got, want, book = check(s, BIG, [complete_tree(4)])                       # 7 pairs
    assert len(got["top_slots"]) > 7 and got["n_pairs"] == 7
    assert sorted(got["names"].tolist()) == got["top_slots"][:7].tolist()  # the lowest seven, whichever rank took which
    s.close()


def test_a_mesh_without_top_slots_and_a_leaf_rooted_result():
    s = scene()
    got, _, _ = check(s, LEAFY, [chain_tree(12)])                             # a leaf root grows records: K = 0
    assert len(got["top_slots"]) == 0 and np.array_equal(got["names"], got["span_base"] + np.arange(11))
    assert got["level_offsets"].tolist() == list(range(12)) and got["stack_depth"] >= 12
    got, _, book = check(s, NAIVE, [[0, 1]])                                   # a tree becomes a leaf root
    assert got["n_pairs"] == 0 and got["level_offsets"].size == 0 and got["root_codes"][NAIVE] == LEAF_BIT | got["leaf_base"]
    assert got["grow"] == 1 and got["span_bases"][NAIVE] != NO_SPAN
    got, _, _ = check(s, GROUND, [[0, 1, 3]])                                  # the ground quad: room for one record
    assert got["n_pairs"] == 1 and got["n_pair_records"] == got["span_base"] + 1
    s.close()


def test_a_second_rebuild_reuses_the_span():
    s = scene()
    got, want, book = check(s, BIG, [complete_tree(9), chain_tree(40), complete_tree(8)])
    assert got["grow"] == 0
    first, _, _ = check(s, BIG, [complete_tree(9)])
    for key in ("span_base", "level_begin", "pair_base", "n_pair_records", "n_refit_levels"):
        assert got[key] == first[key], key
    assert len(got["record_perm"]) == len(first["record_perm"])
    # the chain in between had 39 pairs: the slots it could not use are given up
    assert len(got["top_slots"]) == min(len(first["top_slots"]), 39)
    s.close()


def test_every_member_of_an_instanced_group_follows():
    s = scene(instances=True)
    got, want, book = check(s, 7, [complete_tree(7)], instanced=True)         # through the last placement
    assert got["members"].tolist() == [BIG, 6, 7]
    assert len({int(got["root_codes"][j]) for j in (BIG, 6, 7)}) == 1 and len({int(got["span_bases"][j]) for j in (BIG, 6, 7)}) == 1
    assert all(got["node_counts"][j] == 127 for j in (BIG, 6, 7))
    s.close()


def test_refusals():
    s = scene()
    rc, msg, _, book = plan(s, BIG, [(chain_tree(65), [0])])                  # depth 64: one more than the stack holds
    assert rc == N.CGPT_ERR_UNSUPPORTED and "BVH depth 64 exceeds the traversal stack of 64" in msg
    with pytest.raises(Refused) as e:
        rebuild(book, BIG, chain_tree(65), [0])
    assert e.value.status == rc
    k = min(len(top_slots(book, BIG)), 63)
    rc, msg, _, _ = plan(s, BIG, [(chain_tree(64), spread_ranks(k, 63, 1))])
    assert rc == N.CGPT_OK, msg
    limit = (1 << 26) - 319
    rc, msg, _, book = plan(s, BIG, [(complete_tree(3), [0, 1, 2])], assume=limit)
    assert rc == N.CGPT_ERR_INVALID and "2^26" in msg
    with pytest.raises(Refused) as e:
        rebuild(book, BIG, complete_tree(3), [0, 1, 2], assume_pair_records=limit)
    assert e.value.status == rc
    rc, msg, _, _ = plan(s, BIG, [(complete_tree(3), [0, 1, 2])], assume=limit - 1)
    assert rc == N.CGPT_OK, msg
    for obj in (TRI, SUN, 99):                                                 # no mesh
        assert plan(s, obj, [([0, 1], [])])[0] == N.CGPT_ERR_INVALID
    s.close()
