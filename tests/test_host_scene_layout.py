"""CPU tests of the host half of a scene upload (csrc/device/scene_layout.hip, seen through cgpth_scene_layout): the device
layout that csrc/device/device_scene.h documents, restated here from that documentation and the input scene alone, and every
refusal that stands between a host's malformed tree and a kernel.  No GPU is touched.

Not covered: the 2^26 limit on triangles / child pairs ("scene too large"), which needs gigabytes of input.

Which check fires first for some malformed trees (recorded from the code, the messages are asserted below):
  * an inner node's left_first is checked when its PARENT is visited ("malformed children of node <parent>"), the root's by
    "malformed BVH root"; "malformed inner node" therefore never fires;
  * a node reachable twice is reported as "triangle slot ... is in two leaves": children lie beyond their parent, so there is
    no cycle, and the second descent reaches an already covered leaf before the visit count can exceed node_count
    ("BVH is not a tree").
"""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V

LEAF_BIT = 0x80000000
TOP_RECORDS, SMALL_MESH_TRIS, LDS_TRIS_MAX = 256, 8, 16      # device_scene.h: kTopRecords, kSmallMeshTris, kLdsTrisMax


class DevObject(C.Structure):                                 # device_scene.h: struct DevObject
    _fields_ = [("kind", C.c_uint32), ("mat_index", C.c_uint32), ("root_code", C.c_uint32), ("tri_base", C.c_uint32),
                ("n_tris", C.c_uint32), ("total_area", C.c_float), ("sphere_radius", C.c_float), ("sphere_radius_sq", C.c_float),
                ("sphere_center", C.c_float * 3), ("plane_normal", C.c_float * 3), ("plane_point", C.c_float * 3), ("pad_", C.c_uint32)]


def _array(ptr, n, width, dtype):
    if n == 0:
        return np.zeros((0, width), dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(n, width)).copy().view(dtype)


class Raw:
    """An owned, editable copy of a flattened scene (cgpt_scene_desc): nodes as 8 uint32 words {min.xyz, left_first, max.xyz,
    prim_count}, triangles as 18 float32 {v0 pos, v0 normal, v1 ..., v2 ...}."""

    def __init__(self, desc=None):
        if desc is None:
            return
        self.objects = [N.Object.from_buffer_copy(desc.objects[i]) for i in range(desc.n_objects)]
        self.nodes = _array(desc.nodes, desc.n_nodes, 8, np.uint32)
        self.tris = _array(desc.triangles, desc.n_triangles, 18, np.float32)
        self.tidx = _array(desc.tri_indices, desc.n_triangles, 1, np.uint32).ravel()
        self.materials = [N.Material.from_buffer_copy(desc.materials[i]) for i in range(desc.n_materials)]
        self.lights = [desc.light_indices[i] for i in range(desc.n_lights)]
        self.null = set()                                     # pointers to hand over as NULL
        self.counts = {}                                      # counts to hand over instead of the real ones

    def desc(self):
        objs = (N.Object * max(1, len(self.objects)))(*self.objects)
        mats = (N.Material * max(1, len(self.materials)))(*self.materials)
        lights = np.asarray(self.lights, np.uint32)
        nodes, tris, tidx = (np.ascontiguousarray(a) for a in (self.nodes, self.tris, self.tidx))
        d = N.SceneDesc()
        ptr = lambda name, p: None if name in self.null else p
        d.objects = ptr("objects", objs); d.n_objects = self.counts.get("objects", len(self.objects))
        d.nodes = ptr("nodes", nodes.ctypes.data_as(C.POINTER(N.BvhNode))); d.n_nodes = nodes.shape[0]
        d.triangles = ptr("triangles", tris.ctypes.data_as(C.POINTER(N.Triangle))); d.n_triangles = tris.shape[0]
        d.tri_indices = ptr("tri_indices", tidx.ctypes.data_as(C.POINTER(C.c_uint32)))
        d.materials = ptr("materials", mats); d.n_materials = self.counts.get("materials", len(self.materials))
        d.light_indices = ptr("light_indices", lights.ctypes.data_as(C.POINTER(C.c_uint32))); d.n_lights = len(self.lights)
        return d, (objs, mats, lights, nodes, tris, tidx)

    def mesh(self, oi):
        """(nodes, triangles, tri_indices) of mesh object oi: views into this scene's arrays"""
        o = self.objects[oi]
        return (self.nodes[o.node_offset:o.node_offset + o.node_count], self.tris[o.tri_offset:o.tri_offset + o.tri_count],
                self.tidx[o.tri_offset:o.tri_offset + o.tri_count])


class Layout:
    def __init__(self, v):
        self.node_pairs = _array(v.node_pairs, v.n_node_pairs // 4, 16, np.float32)
        self.tri_leaf = _array(v.tri_leaf, v.n_tri_leaf // 3, 12, np.float32)
        self.tri_orig = _array(v.tri_orig, v.n_tri_orig // 3, 12, np.float32)
        self.tri_normal = _array(v.tri_normal, v.n_tri_normal, 4, np.float32)
        self.materials = _array(v.materials, v.n_materials // 4, 16, np.float32)
        self.obj_trace = _array(v.obj_trace, v.n_obj_trace // 2, 8, np.float32)
        assert v.object_size == C.sizeof(DevObject) == 72
        self.objects = [DevObject.from_buffer_copy(C.string_at(v.objects + i * v.object_size, v.object_size)) for i in range(v.n_objects)]
        u32 = lambda p, n: _array(p, n, 1, np.uint32).ravel()
        self.lights, self.refit_levels, self.record_perm = u32(v.lights, v.n_lights), u32(v.refit_levels, v.n_refit_levels), u32(v.record_perm, v.n_record_perm)
        self.stack_depth, self.n_top_records, self.n_pair_records, self.n_small_tris = v.stack_depth, v.n_top_records, v.n_pair_records, v.n_small_tris
        n = v.n_objects
        self.leaf_base, self.pair_base, self.level_begin = u32(v.leaf_base, n), u32(v.pair_base, n), u32(v.level_begin, n)
        start = u32(v.level_offsets_start, n + 1)
        flat = u32(v.level_offsets, int(start[-1]))
        self.level_offsets = [flat[start[i]:start[i + 1]] for i in range(n)]
        assert (v.n_node_pairs, v.n_tri_leaf, v.n_tri_orig, v.n_materials, v.n_obj_trace) == \
               (4 * self.node_pairs.shape[0], 3 * self.tri_leaf.shape[0], 3 * self.tri_orig.shape[0], 4 * self.materials.shape[0], 2 * n)


def layout(raw):
    """(status, message, Layout or None) of cgpth_scene_layout on a Raw scene"""
    desc, keep = raw.desc()
    view = N.SceneLayoutView()
    rc = N.lib().cgpth_scene_layout(C.byref(desc), C.byref(view))
    del keep
    return rc, N.lib().cgpth_last_error().decode(), (Layout(view) if rc == N.CGPT_OK else None)


def laid_out(scene):
    raw = Raw(scene.flatten())
    rc, msg, lay = layout(raw)
    assert rc == N.CGPT_OK, msg
    return raw, lay


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def octahedron(n_faces=8, offset=(0.0, 0.0, 0.0)):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)[:n_faces]
    return P.Mesh.from_arrays(np.hstack([v + np.asarray(offset, np.float32), v]), f)


def new_scene():
    s = P.Scene()
    for m in P.REFERENCE_MATERIALS:
        s.add_material(m)
    return s


TRIANGLE_OBJECT = ([[-1.0, 0.5, 2.0], [1.25, 0.5, 2.0], [0.0, 2.0, 2.5]], [[0.0, 0.6, 0.8], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
MESH, SPHERE, PLANE, TRIANGLE = N.OBJECT_MESH, N.OBJECT_SPHERE, N.OBJECT_PLANE, N.OBJECT_TRIANGLE


@pytest.fixture(scope="module")
def mixed():
    """every kind of object: a tree above kTopRecords pairs, a second tree, a leaf-rooted mesh, the small ground quad, a triangle
    object, a sphere light and a plane"""
    s = new_scene()
    s.add_mesh(P.Mesh.dragon_standin(2), 3, P.BUILD_SAH_INTERVALS)
    s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_NAIVE)
    s.add_mesh(P.Mesh.dragon_standin(1), 0, P.BUILD_SAH_PRIMITIVES)
    s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), 1, P.BUILD_SAH_INTERVALS)
    s.add_triangle(*TRIANGLE_OBJECT, 0)
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    s.add_plane((0.0, 1.0, 0.0), (0.5, -4.0, 0.25), 1)
    raw, lay = laid_out(s)
    assert [o.kind for o in raw.objects] == [MESH, MESH, MESH, MESH, TRIANGLE, SPHERE, PLANE]
    assert raw.objects[0].node_count == 2 * 319 + 1 and raw.objects[1].node_count > 1 and raw.objects[2].node_count == 1
    return raw, lay


@pytest.fixture(scope="module")
def single():
    s = new_scene()
    s.add_mesh(P.Mesh.dragon_standin(1), 3, P.BUILD_SAH_INTERVALS)
    raw, lay = laid_out(s)
    assert raw.objects[0].tri_count == 80 and raw.objects[0].node_count == 2 * 79 + 1
    return raw, lay


def walk(raw, lay, oi):
    """Walks the input tree of mesh oi from node 0 and node_pairs from objects[oi].root_code side by side, checking every record
    and leaf against device_scene.h.  Returns (records reached per depth as [(input pair index, record)], depth of the deepest leaf)."""
    nodes, tris, tidx = raw.mesh(oi)
    leaf_base = int(lay.leaf_base[oi])
    per_depth, deepest = {}, 0
    todo = [(0, lay.objects[oi].root_code, 0)]
    seen = 0
    while todo:
        ni, code, depth = todo.pop()
        seen += 1
        assert seen <= nodes.shape[0]
        first, count = int(nodes[ni, 3]), int(nodes[ni, 7])
        if count > 0:                                         # a leaf: its run of tri_leaf records
            deepest = max(deepest, depth)
            assert code == LEAF_BIT | (leaf_base + first), (oi, ni)
            run = lay.tri_leaf[leaf_base + first:leaf_base + first + count]
            assert run.shape[0] == count
            words = run.view(np.uint32)
            assert np.array_equal(words[:, 11], [0] * (count - 1) + [1])                       # last_in_leaf
            assert np.array_equal(words[:, 10], tidx[first:first + count])                     # tri_idx, in tri_indices order
            t = tris[tidx[first:first + count]]
            v0, e1, e2 = t[:, 0:3], t[:, 6:9] - t[:, 0:3], t[:, 12:15] - t[:, 0:3]             # float32 subtractions
            expect = np.hstack([v0, e1, e2[:, 0:2], np.zeros((count, 1), np.float32), e2[:, 2:3]])
            assert np.array_equal(words[:, 0:10], bits(expect)), (oi, ni)
            continue
        assert code & LEAF_BIT == 0 and code < lay.n_pair_records, (oi, ni)
        per_depth.setdefault(depth, []).append(((first - 1) // 2, code))
        rec = lay.node_pairs[code].view(np.uint32)
        l, r = nodes[first], nodes[first + 1]
        # {lmin.x, rmin.x, lmin.y, rmin.y | lmin.z, rmin.z, lmax.x, rmax.x | lmax.y, rmax.y, lmax.z, rmax.z | -, -, lcode, rcode}
        side = [0, 1, 2, 4, 5, 6]                             # min.xyz, max.xyz words of a 32-byte node
        assert np.array_equal(rec[0:12:2], l[side]) and np.array_equal(rec[1:12:2], r[side]), (oi, ni)
        todo.append((first + 1, int(rec[15]), depth + 1))
        todo.append((first, int(rec[14]), depth + 1))
    return per_depth, deepest


def mesh_objects(raw):
    return [i for i, o in enumerate(raw.objects) if o.kind == MESH]


def test_round_trip(mixed):
    raw, lay = mixed
    deepest = 0
    for oi in mesh_objects(raw):
        deepest = max(deepest, walk(raw, lay, oi)[1])
    assert deepest == 10 and lay.stack_depth == deepest + 1    # the level-2 tree is the deepest (depth 10)
    # tri_orig / tri_normal: the input triangles in original order at tri_base, objects one after the other
    tri_base = 0
    for oi, o in enumerate(raw.objects):
        if o.kind not in (MESH, TRIANGLE):
            continue
        d = lay.objects[oi]
        assert (d.kind, d.mat_index, d.tri_base, d.n_tris) == (o.kind, o.mat_index, tri_base, o.tri_count)
        t = raw.tris[o.tri_offset:o.tri_offset + o.tri_count]
        orig = lay.tri_orig[tri_base:tri_base + o.tri_count]
        # {p0.xyz, n0.x | p1.xyz, n0.y | p2.xyz, n0.z}
        expect = np.hstack([t[:, 0:3], t[:, 3:4], t[:, 6:9], t[:, 4:5], t[:, 12:15], t[:, 5:6]])
        assert np.array_equal(bits(orig), bits(expect))
        assert np.array_equal(bits(lay.tri_normal[tri_base:tri_base + o.tri_count]), bits(np.hstack([t[:, 3:6], np.zeros((o.tri_count, 1), np.float32)])))
        if o.kind == MESH:
            assert bits([d.total_area])[0] == bits([o.total_area])[0]
        tri_base += o.tri_count
    assert lay.tri_orig.shape[0] == lay.tri_normal.shape[0] == lay.tri_leaf.shape[0] == tri_base
    assert list(lay.lights) == raw.lights == [5]


def expected_perm(raw):
    """record_perm from the input alone: the first min(kTopRecords, n) records of one breadth-first walk that starts with the
    roots of all meshes in object order take positions 0, 1, ...; the others follow in ascending input order."""
    pair_base, n = {}, 0
    for oi in mesh_objects(raw):
        pair_base[oi] = n
        n += raw.objects[oi].node_count // 2
    queue = []                                                # (object, node index of an inner node)
    for oi in mesh_objects(raw):
        if raw.mesh(oi)[0][0, 7] == 0:
            queue.append((oi, 0))
    order, head = [], 0
    while head < len(queue):
        oi, ni = queue[head]; head += 1
        nodes = raw.mesh(oi)[0]
        first = int(nodes[ni, 3])
        order.append(pair_base[oi] + (first - 1) // 2)
        queue += [(oi, c) for c in (first, first + 1) if nodes[c, 7] == 0]
    assert len(order) == len(set(order)) == n                 # every pair of these trees is reachable
    top = order[:min(TOP_RECORDS, n)]
    rest = sorted(set(range(n)) - set(top))
    perm = np.zeros(n, np.uint32)
    perm[top + rest] = np.arange(n, dtype=np.uint32)
    return perm, pair_base


@pytest.mark.parametrize("which", ["mixed", "single"])
def test_record_order(which, request):
    raw, lay = request.getfixturevalue(which)
    perm, pair_base = expected_perm(raw)
    n = perm.size
    assert lay.n_pair_records == n == lay.node_pairs.shape[0] and lay.n_top_records == min(TOP_RECORDS, n)
    assert sorted(lay.record_perm) == list(range(n))
    assert np.array_equal(lay.record_perm, perm)
    for oi in mesh_objects(raw):
        assert lay.pair_base[oi] == pair_base[oi]
        per_depth, _ = walk(raw, lay, oi)                     # the codes in the records follow the renumbering
        for recs in per_depth.values():
            assert all(lay.record_perm[pair_base[oi] + k] == code for k, code in recs)
    if which == "single":                                     # fewer than kTopRecords: breadth-first throughout
        assert lay.n_top_records == 79
    else:
        assert n > TOP_RECORDS
        tail = np.flatnonzero(lay.record_perm >= TOP_RECORDS)
        assert np.array_equal(lay.record_perm[tail], np.arange(TOP_RECORDS, n))              # ascending input order


def small_rule(raw):
    """device_scene.h "record order": in object order, an object of at most kSmallMeshTris leaf records is small while the running
    total stays at most kLdsTrisMax; the small objects tile [0, n_small_tris), everything else follows in object order."""
    n_leaf = [o.tri_count if o.kind == MESH else 1 if o.kind == TRIANGLE else 0 for o in raw.objects]
    small, total = [], 0
    for n in n_leaf:
        small.append(0 < n <= SMALL_MESH_TRIS and total + n <= LDS_TRIS_MAX)
        total += n if small[-1] else 0
    base, nxt = [0] * len(n_leaf), 0
    for pick in (True, False):
        for i, n in enumerate(n_leaf):
            if small[i] == pick:
                base[i] = nxt; nxt += n
    return small, total, base, n_leaf


def test_small_triangles_come_first(mixed):
    raw, lay = mixed
    small, total, base, n_leaf = small_rule(raw)
    assert small == [False, False, False, True, True, False, False] and lay.n_small_tris == total == 3
    has = [i for i, n in enumerate(n_leaf) if n]
    assert [int(lay.leaf_base[i]) for i in has] == [base[i] for i in has]


@pytest.mark.parametrize("faces, expect_small, n_small", [
    # three 8-triangle meshes and a triangle object: two meshes fill the 16 records, so neither the third mesh nor the triangle
    # object (a 17th record) is small
    ((8, 8, 8), [True, True, False, False], 16),
    # the cap bites on the third mesh (14 + 8 > 16) and an object after it is still small (14 + 1)
    ((8, 6, 8), [True, True, False, True], 15),
])
def test_small_triangle_cap(faces, expect_small, n_small):
    s = new_scene()
    for k, f in enumerate(faces):
        s.add_mesh(octahedron(f, (3.0 * k, 0.0, 0.0)), 0, P.BUILD_SAH_INTERVALS)
    s.add_triangle(*TRIANGLE_OBJECT, 1)
    raw, lay = laid_out(s)
    small, total, base, _ = small_rule(raw)
    assert small == expect_small and total == n_small
    assert lay.n_small_tris == n_small and [int(b) for b in lay.leaf_base] == base
    small_ranges = sorted((base[i], base[i] + (raw.objects[i].tri_count if raw.objects[i].kind == MESH else 1)) for i in range(4) if small[i])
    assert small_ranges[0][0] == 0 and small_ranges[-1][1] == n_small
    assert all(a[1] == b[0] for a, b in zip(small_ranges, small_ranges[1:]))
    for oi in mesh_objects(raw):
        walk(raw, lay, oi)
    assert lay.objects[3].root_code == LEAF_BIT | base[3]


def test_refit_levels(mixed):
    raw, lay = mixed
    used = 0
    for oi, o in enumerate(raw.objects):
        offs = lay.level_offsets[oi]
        if o.kind != MESH or o.node_count == 1:               # no child-pair records: a triangle object, a leaf-rooted mesh, ...
            assert offs.size == 0
            continue
        per_depth, _ = walk(raw, lay, oi)
        assert offs[0] == 0 and np.all(np.diff(offs.astype(np.int64)) >= 0) and offs.size == max(per_depth) + 2
        begin = int(lay.level_begin[oi])
        for d in range(offs.size - 1):
            listed = lay.refit_levels[begin + offs[d]:begin + offs[d + 1]]
            assert sorted(listed) == sorted(code for _, code in per_depth[d]), (oi, d)
        assert begin == used
        used += int(offs[-1])
    assert used == lay.refit_levels.size == lay.n_pair_records


def test_obj_trace_and_materials(mixed):
    raw, lay = mixed
    q = lay.obj_trace.view(np.uint32)
    for oi, o in enumerate(raw.objects):
        d = lay.objects[oi]
        if o.kind in (MESH, TRIANGLE):                        # {kind 0, root code}
            assert q[oi, 0] == MESH and q[oi, 1] == d.root_code and not q[oi, 2:].any()
    tri = lay.objects[4]
    assert tri.kind == TRIANGLE and tri.root_code == LEAF_BIT | int(lay.leaf_base[4])
    rec = lay.tri_leaf[lay.leaf_base[4]].view(np.uint32)
    assert rec[10] == 0 and rec[11] == 1                      # tri_idx 0, last_in_leaf
    sph, pl = raw.objects[5], raw.objects[6]
    r2 = np.float32(sph.sphere_radius) * np.float32(sph.sphere_radius)
    assert np.array_equal(q[5], np.concatenate([[SPHERE], bits(list(sph.sphere_center)), bits([r2]), [0, 0, 0]]))
    assert np.array_equal(q[6], np.concatenate([[PLANE], bits(list(pl.plane_normal)), bits(list(pl.plane_point)), [0]]))
    assert bits([lay.objects[5].sphere_radius_sq])[0] == bits([r2])[0]
    # {albedo.xyz, specular | refractivity, absorption.xyz | ior, emissive.xyz | intensity, is_light, alpha, -}; an upload resets alpha
    assert lay.materials.shape[0] == len(raw.materials) == 4
    for i, m in enumerate(raw.materials):
        expect = bits(list(m.albedo) + [m.specular, m.refractivity] + list(m.absorption) + [m.ior] + list(m.emissive) + [m.intensity, 0, 0, 0])
        expect[13] = m.is_light
        assert np.array_equal(lay.materials[i].view(np.uint32), expect)
        assert lay.materials[i, 14] == 0.0


# ---- refusals: a valid raw scene with one thing broken per case --------------------------------------------------------------

@pytest.fixture(scope="module")
def valid_desc():
    s = new_scene()
    s.add_mesh(P.Mesh.dragon_standin(1), 3, P.BUILD_SAH_INTERVALS)
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -4.0, 0.0), 1)
    return s, s.flatten()


@pytest.fixture
def raw(valid_desc):
    return Raw(valid_desc[1])


def inner_child_of_root(nodes):
    return next(c for c in (int(nodes[0, 3]), int(nodes[0, 3]) + 1) if nodes[c, 7] == 0)


def leaves(nodes):
    """node indices of the reachable leaves, by ascending first slot"""
    out, todo = [], [0]
    while todo:
        ni = todo.pop()
        if nodes[ni, 7] > 0:
            out.append(ni)
        else:
            todo += [int(nodes[ni, 3]), int(nodes[ni, 3]) + 1]
    return sorted(out, key=lambda ni: nodes[ni, 3])


def break_no_objects(r): r.counts["objects"] = 0
def break_no_materials(r): r.counts["materials"] = 0
def break_null_lights(r): r.null.add("light_indices")
def break_mat_index(r): r.objects[2].mat_index = len(r.materials)
def break_null_nodes(r): r.null.add("nodes")
def break_node_slice(r): r.objects[0].node_offset = 1
def break_tri_slice(r): r.objects[0].tri_offset = 1
def break_even_node_count(r): r.objects[0].node_count -= 1
def break_tri_index(r): r.tidx[5] = r.objects[0].tri_count
def break_root_leaf_range(r): r.nodes[0, 3] = 1; r.nodes[0, 7] = r.objects[0].tri_count
def break_even_left_first(r): r.nodes[0, 3] += 1
def break_light_index(r): r.lights[0] = len(r.objects)
def break_plane_light(r): r.lights[0] = 2
def break_kind(r): r.objects[2].kind = 4


def break_child_not_beyond_parent(r):
    c = inner_child_of_root(r.nodes)
    r.nodes[c, 3] = c if c & 1 else c - 1                     # odd and in range, but not beyond the node itself


def break_child_pair_beyond_nodes(r):
    r.nodes[inner_child_of_root(r.nodes), 3] = r.objects[0].node_count       # odd; the pair's second node does not exist


def break_two_leaves_one_slot(r):
    a, b = leaves(r.nodes)[:2]
    r.nodes[b, 3] = r.nodes[a, 3]


def break_node_reachable_twice(r):
    first = int(r.nodes[0, 3])
    assert r.nodes[first, 7] == 0 and r.nodes[first + 1, 7] == 0              # both children of the root are inner nodes
    r.nodes[first + 1, 3] = r.nodes[first, 3]                                 # the right child now shares the left child's pair


REFUSALS = [
    (break_no_objects, N.CGPT_ERR_INVALID, "scene has no objects"),
    (break_no_materials, N.CGPT_ERR_INVALID, "scene has no materials"),
    (break_null_lights, N.CGPT_ERR_INVALID, "light_indices is null"),
    (break_mat_index, N.CGPT_ERR_INVALID, "object 2: mat_index 4 out of range"),
    (break_null_nodes, N.CGPT_ERR_INVALID, "mesh object 0 but nodes/triangles/tri_indices is null"),
    (break_node_slice, N.CGPT_ERR_INVALID, "object 0: node slice out of range"),
    (break_tri_slice, N.CGPT_ERR_INVALID, "object 0: triangle slice out of range"),
    (break_even_node_count, N.CGPT_ERR_INVALID, "odd node count, got 158"),
    (break_tri_index, N.CGPT_ERR_INVALID, "tri_indices[5] = 80 out of range"),
    (break_root_leaf_range, N.CGPT_ERR_INVALID, "malformed BVH root"),
    (break_even_left_first, N.CGPT_ERR_INVALID, "malformed BVH root"),
    (break_child_not_beyond_parent, N.CGPT_ERR_INVALID, "malformed children of node 0"),
    (break_child_pair_beyond_nodes, N.CGPT_ERR_INVALID, "malformed children of node 0"),
    (break_two_leaves_one_slot, N.CGPT_ERR_INVALID, "is in two leaves"),
    (break_node_reachable_twice, N.CGPT_ERR_INVALID, "is in two leaves"),      # not "BVH is not a tree": see the module docstring
    (break_light_index, N.CGPT_ERR_INVALID, "light_indices[0] = 3 out of range"),
    (break_plane_light, N.CGPT_ERR_UNSUPPORTED, "Main.cpp:383"),
    (break_kind, N.CGPT_ERR_UNSUPPORTED, "primitive kind 4 has no intersector"),
]


def test_the_unbroken_scene_is_accepted(raw):
    rc, msg, lay = layout(raw)
    assert rc == N.CGPT_OK, msg
    assert walk(raw, lay, 0)[1] == 8 and lay.stack_depth == 9


@pytest.mark.parametrize("breaker, status, text", REFUSALS, ids=[b.__name__[6:] for b, _, _ in REFUSALS])
def test_refusals(raw, breaker, status, text):
    breaker(raw)
    rc, msg, _ = layout(raw)
    assert rc == status and text in msg, (rc, msg)


def test_refusal_of_a_null_argument():
    assert N.lib().cgpth_scene_layout(None, None) == N.CGPT_ERR_INVALID


def chain_scene(depth):
    """A hand-built tree of the given depth: every inner node has a one-triangle leaf on the left and the chain on the right."""
    r = Raw()
    n_nodes, n_tris = 2 * depth + 1, depth + 1
    r.nodes = np.zeros((n_nodes, 8), np.uint32)
    r.nodes[:, 0:3] = bits([-1.0, -1.0, -1.0]); r.nodes[:, 4:7] = bits([float(n_tris), 1.0, 1.0])
    for k in range(depth):                                    # inner node 2k (the root is node 0) -> children 2k + 1 (leaf k), 2k + 2
        r.nodes[2 * k, 3] = 2 * k + 1
        r.nodes[2 * k + 1, 3] = k; r.nodes[2 * k + 1, 7] = 1
    r.nodes[2 * depth, 3] = depth; r.nodes[2 * depth, 7] = 1
    r.tris = np.zeros((n_tris, 18), np.float32)
    for t in range(n_tris):
        r.tris[t] = [t, 0, 0, 0, 0, 1, t + 0.5, 0, 0, 0, 0, 1, t, 0.5, 0, 0, 0, 1]
    r.tidx = np.arange(n_tris, dtype=np.uint32)
    o = N.Object(kind=MESH, mat_index=0, node_offset=0, node_count=n_nodes, tri_offset=0, tri_count=n_tris, max_depth=depth, total_area=0.125 * n_tris)
    r.objects, r.materials, r.lights, r.null, r.counts = [o], [P.REFERENCE_MATERIALS[0].to_abi()], [], set(), {}
    return r


def test_depth_limit_of_the_traversal_stack():
    deep = chain_scene(65)
    assert deep.nodes.shape[0] == 131
    rc, msg, _ = layout(deep)
    assert rc == N.CGPT_ERR_UNSUPPORTED and "BVH depth 65 exceeds the traversal stack of 64" in msg, (rc, msg)
    ok = chain_scene(63)
    rc, msg, lay = layout(ok)
    assert rc == N.CGPT_OK, msg
    per_depth, deepest = walk(ok, lay, 0)
    assert deepest == 63 and lay.stack_depth == 64 and sorted(per_depth) == list(range(63))
    assert [int(x) for x in lay.level_offsets[0]] == list(range(64))          # one record per depth
