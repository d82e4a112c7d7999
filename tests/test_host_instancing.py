"""CPU tests of mesh instancing in the host half of an upload (csrc/device/scene_layout.hip through cgpth_scene_layout_instanced, and the
host mirror's cgpth_scene_add_instance): one laid-out copy per distinct tuple of slice words, the sharers' equal bases, the record
permutation, a walk of every object's tree against the plain layout of the same cgpt_scene_desc -- the yardstick throughout -- and the
refusals.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.scene import triangles_from_arrays
import instancing_scenes as IS
import test_host_scene_layout as HL
import transform_scenes as TS

LEAF_BIT = HL.LEAF_BIT
MESH = N.OBJECT_MESH


def lay_out(flat, instanced):
    """(status, message, HL.Layout or None) of cgpth_scene_layout / cgpth_scene_layout_instanced on a Flat scene"""
    desc, keep = flat.desc()
    view = N.SceneLayoutView()
    fn = N.lib().cgpth_scene_layout_instanced if instanced else N.lib().cgpth_scene_layout
    rc = fn(C.byref(desc), C.byref(view))
    del keep
    return rc, N.lib().cgpth_last_error().decode(), (HL.Layout(view) if rc == N.CGPT_OK else None)


def ok(flat, instanced):
    rc, msg, lay = lay_out(flat, instanced)
    assert rc == N.CGPT_OK, msg
    return lay


@pytest.fixture(scope="module")
def grove():
    g = IS.Grove()
    yield g, ok(g.flat, False), ok(g.flat, True)
    g.close()


def tree_walk(lay, oi):
    """What a traversal from objects[oi].root_code meets, in order: ("pair", the record's 12 box words) and ("leaf", the triangles'
    ten geometry words, tri_idx and last_in_leaf) -- no record index, no leaf base: those are names, and differ between the layouts."""
    out, todo = [], [lay.objects[oi].root_code]
    while todo:
        code = todo.pop()
        if code & LEAF_BIT:
            slot = code & ~LEAF_BIT
            while True:
                rec = lay.tri_leaf[slot].view(np.uint32)
                out.append(("leaf", rec.tobytes()))
                if rec[11]:
                    break
                slot += 1
            continue
        rec = lay.node_pairs[code].view(np.uint32)
        out.append(("pair", rec[:12].tobytes()))
        todo += [int(rec[15]), int(rec[14])]
    return out


def test_one_copy_per_distinct_slice_tuple(grove):
    g, plain, inst = grove
    uniq, keep = g.unique()
    want = ok(uniq, False)                                    # the plain layout of the scene with one object per group
    for name in ("tri_leaf", "tri_orig", "tri_normal", "node_pairs", "refit_levels"):
        assert getattr(inst, name).shape == getattr(want, name).shape, name
    assert inst.n_pair_records == want.n_pair_records and inst.n_top_records == want.n_top_records
    assert inst.tri_leaf.shape[0] == IS.ICO_TRIS + 2 + 12 + 12 + 1
    assert plain.tri_leaf.shape[0] == IS.N_ICOS * IS.ICO_TRIS + IS.N_QUADS * 2 + 12 + 2 * 12 + 1
    # the arrays are those of the one-object-per-group scene to the bit: the same meshes in the same order
    for name in ("tri_leaf", "tri_orig", "tri_normal", "node_pairs"):
        assert np.array_equal(getattr(inst, name).view(np.uint32), getattr(want, name).view(np.uint32)), name
    assert np.array_equal(inst.refit_levels, want.refit_levels) and np.array_equal(inst.record_perm, want.record_perm)
    # the shared quad takes 2 of the 16 LDS records however many objects name it, and the triangle object one; under the plain layout
    # eight quads fill the 16 and the other two, and the triangle object, are left out
    assert inst.n_small_tris == 2 + 1
    assert plain.n_small_tris == 16
    assert inst.stack_depth == plain.stack_depth == want.stack_depth


def test_normal_pairs_follow_the_copies(grove):
    g, plain, inst = grove
    desc, keep = g.flat.desc()
    vp, vi = N.SceneLayoutView(), N.SceneLayoutView()
    assert N.lib().cgpth_scene_layout(C.byref(desc), C.byref(vp)) == 0
    n_plain = vp.n_tri_normal12
    assert N.lib().cgpth_scene_layout_instanced(C.byref(desc), C.byref(vi)) == 0
    assert vi.n_tri_normal12 == 2 * inst.tri_orig.shape[0] and n_plain == 2 * plain.tri_orig.shape[0]
    del keep


def test_sharers_have_equal_codes_and_bases(grove):
    g, plain, inst = grove
    for group in (g.icos, g.quads, [g.emitter, g.twin]):
        first = group[0]
        for oi in group:
            a, b = inst.objects[first], inst.objects[oi]
            assert (b.root_code, b.tri_base, b.n_tris) == (a.root_code, a.tri_base, a.n_tris)
            assert inst.leaf_base[oi] == inst.leaf_base[first] and inst.pair_base[oi] == inst.pair_base[first]
            assert inst.level_begin[oi] == inst.level_begin[first] and np.array_equal(inst.level_offsets[oi], inst.level_offsets[first])
            q = inst.obj_trace.view(np.uint32)
            assert q[oi, 0] == MESH and q[oi, 1] == a.root_code
        # under the plain layout every object has its own
        assert len({int(plain.leaf_base[oi]) for oi in group}) == len(group)
        assert len({plain.objects[oi].tri_base for oi in group}) == len(group)
    # what stays an object's own: kind, material, the area as given
    for oi, o in enumerate(g.flat.objects):
        d = inst.objects[oi]
        assert (d.kind, d.mat_index) == (o.kind, o.mat_index)
        if o.kind == MESH:
            assert HL.bits([d.total_area])[0] == HL.bits([o.total_area])[0]
    assert inst.objects[g.twin].total_area == 0.5 != inst.objects[g.emitter].total_area
    assert list(inst.lights) == [g.lamp, g.emitter]
    # groups do not share with each other, nor with the unshared box and the triangle object
    bases = {int(inst.leaf_base[k]) for k in (g.icos[0], g.quads[0], g.emitter, g.box, g.tri)}
    assert len(bases) == 5


def test_record_perm_is_a_permutation(grove):
    g, plain, inst = grove
    for lay in (plain, inst):
        assert sorted(lay.record_perm) == list(range(lay.n_pair_records)) and lay.n_pair_records == lay.node_pairs.shape[0]
    assert inst.n_pair_records == 79 + 0 + 2 * (g.flat.objects[g.box].node_count // 2)      # the icosphere, the leaf-rooted quad, the two boxes
    # the refit levels list every record of every group once
    assert sorted(inst.refit_levels) == list(range(inst.n_pair_records))
    assert sorted(plain.refit_levels) == list(range(plain.n_pair_records))


def test_every_object_walks_the_same_tree_in_both_layouts(grove):
    g, plain, inst = grove
    raw = HL.Raw(g.flat.desc()[0])
    for oi, o in enumerate(g.flat.objects):
        if o.kind not in (MESH, N.OBJECT_TRIANGLE):
            continue
        a, b = tree_walk(plain, oi), tree_walk(inst, oi)
        assert a == b, oi
        assert sum(kind == "leaf" for kind, _ in a) == o.tri_count
        if o.kind == MESH:
            HL.walk(raw, plain, oi)                           # and both are the input tree, record by record (device_scene.h)
            HL.walk(raw, inst, oi)
        # tri_orig at tri_base: the object's triangles in original order, in either layout
        for lay in (plain, inst):
            d = lay.objects[oi]
            assert np.array_equal(lay.tri_orig[d.tri_base:d.tri_base + d.n_tris].view(np.uint32),
                                  plain.tri_orig[plain.objects[oi].tri_base:plain.objects[oi].tri_base + d.n_tris].view(np.uint32))


def test_partial_overlap_stays_separate():
    s = P.Scene()
    mat = s.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
    s.add_mesh(P.Mesh.from_arrays(*IS.quad_mesh()), mat)
    f = TS.Flat(s.flatten())
    s.close()
    assert f.nodes.shape[0] == 1 and f.tris.shape[0] == 2 and list(f.tidx) == [0, 1]
    # triangles {t0, t1, t0'} with tri_indices {0, 1, 0}; nodes {the quad's leaf, a one-triangle leaf, a second two-triangle leaf}
    leaf = lambda count: np.array([[0, 0, 0, 0, 0, 0, 0, count]], np.uint32)
    f.nodes = np.vstack([f.nodes, leaf(1), leaf(2)])
    f.tris = np.vstack([f.tris, f.tris[0:1]])
    f.tidx = np.array([0, 1, 0], np.uint32)
    mesh = lambda node, tri, count: N.Object(kind=MESH, mat_index=mat, node_offset=node, node_count=1, tri_offset=tri, tri_count=count, max_depth=0, total_area=0.1)
    quad = f.objects[0]
    # 1: triangles [0, 1), inside the quad's [0, 2).  2: triangles [1, 3), which shares t1 with the quad.  3: the quad's four words
    f.objects = [quad, mesh(1, 0, 1), mesh(2, 1, 2), N.Object.from_buffer_copy(quad)]
    inst, plain = ok(f, True), ok(f, False)
    assert inst.leaf_base[3] == inst.leaf_base[0] and inst.objects[3].tri_base == inst.objects[0].tri_base
    assert len({int(inst.leaf_base[k]) for k in (0, 1, 2)}) == 3 and len({inst.objects[k].tri_base for k in (0, 1, 2)}) == 3
    assert inst.tri_leaf.shape[0] == 2 + 1 + 2 and plain.tri_leaf.shape[0] == 2 + 1 + 2 + 2
    for oi in range(4):
        assert tree_walk(inst, oi) == tree_walk(plain, oi)
    # the same triangle slice under another node slice is another mesh
    f.objects[3].node_offset = 2
    apart = ok(f, True)
    assert apart.leaf_base[3] != apart.leaf_base[0] and apart.tri_leaf.shape[0] == plain.tri_leaf.shape[0]
    # and so is the same node slice with another triangle count
    f.objects[3].node_offset = 1; f.objects[3].tri_count = 1
    assert ok(f, True).leaf_base[3] == ok(f, True).leaf_base[1]              # all four words of object 1: shared
    f.objects[3].tri_offset = 2
    assert ok(f, True).leaf_base[3] != ok(f, True).leaf_base[1]


@pytest.mark.parametrize("breaker, status, text", HL.REFUSALS, ids=[b.__name__[6:] for b, _, _ in HL.REFUSALS])
def test_every_refusal_of_the_plain_layout_is_a_refusal_here(breaker, status, text):
    s = HL.new_scene()
    s.add_mesh(P.Mesh.dragon_standin(1), 3, P.BUILD_SAH_INTERVALS)
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -4.0, 0.0), 1)
    raw = HL.Raw(s.flatten())
    s.close()
    raw.objects.append(N.Object.from_buffer_copy(raw.objects[0]))             # a sharer of the mesh, behind everything else
    breaker(raw)
    if breaker in (HL.break_node_slice, HL.break_tri_slice, HL.break_even_node_count):
        raw.objects[3] = N.Object.from_buffer_copy(raw.objects[0])            # the breakers edit object 0's words: the sharer follows
    if breaker is HL.break_light_index:
        text = text.replace("= 3 out", "= 4 out")                             # one object more than in the scene the list was written for
    desc, keep = raw.desc()
    got = []
    for fn in (N.lib().cgpth_scene_layout, N.lib().cgpth_scene_layout_instanced):
        view = N.SceneLayoutView()
        rc = fn(C.byref(desc), C.byref(view))
        got.append((rc, N.lib().cgpth_last_error().decode()))
    del keep
    assert got[0][0] == got[1][0] == status and text in got[0][1], got
    assert got[0][1] == got[1][1]                              # the same message, object index included


def test_null_arguments_are_refused():
    assert N.lib().cgpth_scene_layout_instanced(None, None) == N.CGPT_ERR_INVALID


def test_the_plain_layout_of_a_scene_without_sharers_equals_the_instanced_one():
    """cgpth_scene_layout is what it was: on the scene the existing layout test walks (test_host_scene_layout.mixed) it still passes
    that test's checks, and without sharers the instanced layout is the same layout to the bit."""
    s = HL.new_scene()
    s.add_mesh(P.Mesh.dragon_standin(2), 3, P.BUILD_SAH_INTERVALS)
    s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_NAIVE)
    s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_SAH_PRIMITIVES)            # equal geometry in another tree and other slices: no sharer
    s.add_mesh(P.Mesh.from_arrays(HL.GROUND_V, HL.GROUND_I), 1, P.BUILD_SAH_INTERVALS)
    s.add_triangle(*HL.TRIANGLE_OBJECT, 0)
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    s.add_plane((0.0, 1.0, 0.0), (0.5, -4.0, 0.25), 1)
    raw, plain = HL.laid_out(s)
    inst = ok(TS.Flat(s.flatten()), True)
    s.close()
    perm, _ = HL.expected_perm(raw)
    assert np.array_equal(plain.record_perm, perm)
    for name in ("node_pairs", "tri_leaf", "tri_orig", "tri_normal", "materials", "obj_trace"):
        assert np.array_equal(getattr(plain, name).view(np.uint32), getattr(inst, name).view(np.uint32)), name
    for name in ("lights", "refit_levels", "record_perm", "leaf_base", "pair_base", "level_begin"):
        assert np.array_equal(getattr(plain, name), getattr(inst, name)), name
    assert [bytes(o) for o in plain.objects] == [bytes(o) for o in inst.objects]
    assert (plain.stack_depth, plain.n_top_records, plain.n_pair_records, plain.n_small_tris) == (inst.stack_depth, inst.n_top_records, inst.n_pair_records, inst.n_small_tris)


# ---- the host mirror: Scene.add_instance --------------------------------------------------------------------------------------------------
def instanced_scene():
    s = P.Scene()
    mat = s.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
    other = s.add_material(P.Material(albedo=(0.9, 0.9, 0.9), specular=1.0))
    ball = s.add_mesh(P.Mesh.from_arrays(*IS.S.icosphere(1, (0.0, 0.0, 0.0), 0.5)), mat)
    sphere = s.add_sphere((0.0, 3.0, 0.0), 0.5, mat)
    plane = s.add_plane((0.0, 1.0, 0.0), (0.0, -1.0, 0.0), mat)
    tri = s.add_triangle(*HL.TRIANGLE_OBJECT, mat)
    return s, mat, other, ball, sphere, plane, tri


def test_add_instance_flattens_to_shared_slices():
    s, mat, other, ball, sphere, plane, tri = instanced_scene()
    shift = np.array([[1, 0, 0, 2.0], [0, 1, 0, 0.0], [0, 0, 1, 0.0]], np.float32)
    a = s.add_instance(ball, other, transform=shift, smooth=True)
    b = s.add_instance(a, mat)                                # a chain: an instance of the instance shares the owner's mesh
    assert (a, b) == (4, 5)
    d = s.flatten()
    words = lambda k: (d.objects[k].kind, d.objects[k].node_offset, d.objects[k].node_count, d.objects[k].tri_offset, d.objects[k].tri_count)
    assert words(a) == words(b) == words(ball) and d.objects[ball].kind == MESH
    assert (d.objects[a].mat_index, d.objects[b].mat_index, d.objects[ball].mat_index) == (other, mat, mat)
    assert d.n_triangles == 80 + 1 and d.n_nodes == d.objects[ball].node_count                # the mesh once, and the triangle object
    assert s.has_instances() and list(s.smooth_normals()) == [0, 0, 0, 0, 1, 0]
    assert np.array_equal(s.transforms()[a], shift) and np.array_equal(s.transforms()[b], s.transforms()[ball])
    inst = ok(TS.Flat(d), True)
    assert inst.leaf_base[a] == inst.leaf_base[b] == inst.leaf_base[ball] and inst.tri_orig.shape[0] == 81
    assert ok(TS.Flat(d), False).tri_orig.shape[0] == 3 * 80 + 1
    s.close()


def test_add_instance_refuses_what_has_no_mesh():
    s, mat, other, ball, sphere, plane, tri = instanced_scene()
    for k, kind in ((sphere, "sphere"), (plane, "plane"), (tri, "triangle object")):
        with pytest.raises(P.scene.HostError, match=kind):
            s.add_instance(k, mat)
    with pytest.raises(P.scene.HostError, match="out of range"):
        s.add_instance(99, mat)
    assert s.flatten().n_objects == 4 and not s.has_instances()
    s.close()


def test_a_host_refit_or_rebuild_through_the_instance_shows_through_the_owner():
    s, mat, other, ball, sphere, plane, tri = instanced_scene()
    a = s.add_instance(ball, other)
    v, i = IS.S.icosphere(1, (0.0, 0.0, 0.0), 0.5)
    v = v.copy(); v[:, 1] *= np.float32(0.5)
    before = s.bvh_export(ball)[0].copy()
    s.refit_mesh(a, triangles_from_arrays(v, i))
    after_owner, after_inst = s.bvh_export(ball), s.bvh_export(a)
    assert not np.array_equal(before, after_owner[0])
    assert np.array_equal(after_owner[0], after_inst[0]) and np.array_equal(after_owner[1], after_inst[1])
    assert s.bvh_info(ball).total_area == s.bvh_info(a).total_area
    d = s.flatten()
    assert d.n_triangles == 81
    got = np.ctypeslib.as_array(C.cast(d.triangles, C.POINTER(C.c_float)), shape=(81, 18))[:80]
    assert np.array_equal(got, triangles_from_arrays(v, i))
    s.rebuild_bvh(ball, P.BUILD_NAIVE)                        # through the owner: the instance sees the new tree
    assert np.array_equal(s.bvh_export(ball)[0], s.bvh_export(a)[0]) and not np.array_equal(s.bvh_export(a)[0], after_inst[0])
    # the objects travel with their mesh through a reordering
    s.sort_objects_spatially()
    d = s.flatten()
    meshes = [k for k in range(d.n_objects) if d.objects[k].kind == MESH]
    assert len(meshes) == 2 and d.objects[meshes[0]].tri_offset == d.objects[meshes[1]].tri_offset and d.n_triangles == 81
    s.close()
