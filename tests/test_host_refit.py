"""BVH refit and primitive edits in the host mirror (cgpth_scene_refit_mesh / cgpth_scene_update_primitive; MeshBVH::Refit), CPU only.

The contract (csrc/device/refit.hip): the tree keeps its nodes, left_first / prim_count and tri_indices; each node's bounds become
BVH::CalculateNodeBounds (ref: BVH.cpp:188-202) over the node's current leaf-order range of the new triangles -- 1e30 / -1e30 folded
with TriangleBounds (ref: Primitives.cpp:232-243) by std::min / std::max -- and total_area the sequential sum of GetTriangleArea in
original order (ref: BVH.cpp:22).  Checked against an independent numpy restatement and against the C oracle.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import GROUND_I, GROUND_V, standin_mesh

OPTIONS = [P.BUILD_NAIVE, P.BUILD_SAH_INTERVALS, P.BUILD_SAH_PRIMITIVES]


# ---- the independent statement of the contract -------------------------------------------------------------------------
def _std_min(a, b):
    return np.where(b < a, b, a)            # std::min(a, b): a NaN b never replaces a, a tie keeps a


def _std_max(a, b):
    return np.where(a < b, b, a)


def expected_bounds(nodes: np.ndarray, tri_indices: np.ndarray, tris: np.ndarray):
    """(lo[n,3], hi[n,3]) float32: each node's CalculateNodeBounds over its current range, folded sequentially.
    The sequential fold acc = std::min(acc, x) from 1e30 ends on the FIRST element equal to the smallest non-NaN value of the range with
    1e30 in front (a NaN never replaces acc, an equal value never does either; -0.0 == +0.0), and that is how it is evaluated here."""
    p = tris.reshape(-1, 3, 6)[:, :, :3]
    tb_lo = _std_min(_std_min(p[:, 0], p[:, 1]), p[:, 2])[tri_indices]    # TriangleBounds (v0, then v1, then v2), in leaf order
    tb_hi = _std_max(_std_max(p[:, 0], p[:, 1]), p[:, 2])[tri_indices]
    lf = nodes[:, 3].astype(np.int64); pc = nodes[:, 7].astype(np.int64)
    lo = np.empty((len(nodes), 3), np.float32); hi = np.empty((len(nodes), 3), np.float32)

    def fold(vals, sentinel, better):
        seq = np.concatenate([np.full((1, 3), sentinel, np.float32), vals])
        key = np.where(np.isnan(seq), better * np.inf, seq)             # NaN never wins
        best = key.min(axis=0) if better > 0 else key.max(axis=0)
        first = np.argmax(key == best, axis=0)                           # first element equal to the best value
        return seq[first, np.arange(3)]

    # a node's range: a leaf's own slots, an inner node's the union of its subtree's leaves (contiguous, found bottom-up)
    first = lf.copy(); count = pc.copy()
    for k in range(len(nodes) - 1, -1, -1):
        if pc[k] == 0:
            a, b = lf[k], lf[k] + 1
            first[k] = first[a]; count[k] = count[a] + count[b]
            assert first[b] == first[a] + count[a]
    for k in range(len(nodes)):
        lo[k] = fold(tb_lo[first[k]:first[k] + count[k]], np.float32(1e30), +1)
        hi[k] = fold(tb_hi[first[k]:first[k] + count[k]], np.float32(-1e30), -1)
    return lo, hi


def node_bounds(nodes: np.ndarray):
    f = nodes.view(np.float32)
    return f[:, 0:3], f[:, 4:7]


# ---- meshes and deformations ---------------------------------------------------------------------------------------------
def soup(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-4, 4, (n, 1, 3)).astype(np.float32)
    p = (c + rng.normal(0, 0.4, (n, 3, 3))).astype(np.float32)
    nrm = rng.normal(0, 1, (n, 3, 3)).astype(np.float32)
    v = np.concatenate([p, nrm], axis=2).reshape(-1, 6)
    return v, np.arange(3 * n, dtype=np.uint32)


def duck(reference_assets):
    m = P.Mesh.load_gltf(os.path.join(reference_assets, "Duck/Duck.gltf"))
    return m.vertices, m.indices


def deform(v, kind, seed=1):
    """moved vertices (positions only; normals turned too where it is cheap, so that the refit's normal path is exercised)"""
    rng = np.random.default_rng(seed)
    w = v.copy()
    if kind == "jitter":
        w[:, :3] += rng.normal(0, 0.05, (len(w), 3)).astype(np.float32)
        w[:, 3:] = w[:, [4, 5, 3]]
    elif kind == "translate":
        w[:, :3] += np.float32([1234.5, -77.25, 4096.0])
    elif kind == "collapse":
        w[:, 1] = np.float32(-2.5)                                       # every triangle in one plane: zero-height boxes
    elif kind == "special":
        specials = np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, 2e30, -2e30, 0.0, -0.0])
        pos = w[:, :3]
        mask = rng.random(pos.shape) < 0.2
        pos[mask] = specials[rng.integers(0, len(specials), mask.sum())]
        w[:, :3] = pos
    else:
        raise ValueError(kind)
    return w


def host_scene(v, i, option):
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    s.add_mesh(P.Mesh.from_arrays(v, i), 0, option)
    return s


def oracle_mesh(v, i, option):
    o = O.OracleScene()
    o.add_material((0.5, 0.5, 0.5))
    assert o.add_mesh(v, i, 0, option) == 0
    return o


def bits(x):
    return np.float32(x).view(np.uint32)


# ---- unchanged triangles give back the built tree --------------------------------------------------------------------------
MESHES = ["standin3", "standin4", "standin5", "duck", "soup"]


def mesh_named(name, reference_assets):
    if name.startswith("standin"):
        return standin_mesh(int(name[-1]))
    if name == "duck":
        return duck(reference_assets)
    return soup(3000, 7)


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("name", MESHES)
def test_refit_with_unchanged_triangles_gives_back_the_built_tree(name, option, reference_assets):
    v, i = mesh_named(name, reference_assets)
    s = host_scene(v, i, option)
    built, built_tri = s.bvh_export(0)
    area0 = s.bvh_info(0).total_area
    s.refit_mesh(0, P.triangles_from_arrays(v, i))
    nodes, tri = s.bvh_export(0)
    assert np.array_equal(tri, built_tri)
    assert np.array_equal(nodes[:, [3, 7]], built[:, [3, 7]])                   # left_first, prim_count word for word
    for a, b in zip(node_bounds(nodes), node_bounds(built)):
        assert np.array_equal(a, b)                                              # as values: only the sign of a zero may differ
    assert bits(s.bvh_info(0).total_area) == bits(area0)
    o = oracle_mesh(v, i, option)
    onodes, otri = o.bvh_export(0)
    assert np.array_equal(otri, tri) and np.array_equal(onodes[:, [3, 7]], nodes[:, [3, 7]])
    for a, b in zip(node_bounds(onodes), node_bounds(nodes)):
        assert np.array_equal(a, b)
    lo, hi = expected_bounds(nodes, tri, P.triangles_from_arrays(v, i))
    assert np.array_equal(node_bounds(nodes)[0].view(np.uint32), lo.view(np.uint32))
    assert np.array_equal(node_bounds(nodes)[1].view(np.uint32), hi.view(np.uint32))
    s.close(); o.close()


# ---- moved vertices ---------------------------------------------------------------------------------------------------
DEFORMS = ["jitter", "translate", "collapse", "special"]


@pytest.mark.parametrize("option", [P.BUILD_SAH_INTERVALS, P.BUILD_NAIVE, P.BUILD_SAH_PRIMITIVES])
@pytest.mark.parametrize("kind", DEFORMS)
@pytest.mark.parametrize("name", ["standin4", "soup"])
def test_refit_with_moved_vertices_follows_the_contract(name, kind, option, reference_assets):
    v, i = mesh_named(name, reference_assets)
    s = host_scene(v, i, option)
    built, built_tri = s.bvh_export(0)
    w = deform(v, kind)
    tris = P.triangles_from_arrays(w, i)
    s.refit_mesh(0, tris)
    nodes, tri = s.bvh_export(0)
    assert np.array_equal(tri, built_tri) and np.array_equal(nodes[:, [3, 7]], built[:, [3, 7]])
    lo, hi = expected_bounds(nodes, tri, tris)
    assert np.array_equal(node_bounds(nodes)[0].view(np.uint32), lo.view(np.uint32))   # word for word
    assert np.array_equal(node_bounds(nodes)[1].view(np.uint32), hi.view(np.uint32))
    # the flattened scene carries the new triangles in original order
    desc = s.flatten()
    got = np.ctypeslib.as_array(C.cast(desc.triangles, C.POINTER(C.c_float)), shape=(desc.n_triangles * 18,)).reshape(-1, 18)
    assert np.array_equal(got.view(np.uint32), tris.view(np.uint32))
    # total_area: the oracle's Build of the moved mesh reports the same sequential sum, whatever tree it builds
    o = oracle_mesh(w, i, P.BUILD_SAH_PRIMITIVES)                                  # never splits: cheap on any input
    want, got_area = o.bvh_info(0).total_area, s.bvh_info(0).total_area
    if kind == "special":
        assert np.isnan(want) and np.isnan(got_area)                            # a NaN / inf coordinate makes its area NaN
    else:
        assert bits(got_area) == bits(want)
    s.close(); o.close()


def test_refit_after_refit_equals_one_refit_and_rebuild_uses_new_centroids():
    v, i = standin_mesh(3)
    s = host_scene(v, i, P.BUILD_SAH_INTERVALS)
    for k in range(5):
        s.refit_mesh(0, P.triangles_from_arrays(deform(v, "jitter", seed=k), i))
    w = deform(v, "jitter", seed=99)
    w[:, :3] *= np.float32([1.0, 3.0, 0.5])                             # a deformation that moves split decisions
    tris = P.triangles_from_arrays(w, i)
    s.refit_mesh(0, tris)
    t = host_scene(v, i, P.BUILD_SAH_INTERVALS)
    t.refit_mesh(0, tris)
    assert np.array_equal(s.bvh_export(0)[0], t.bvh_export(0)[0])     # a refit depends on the tree and the new triangles only
    # Rebuild (ref: BVH.cpp:47-59) re-splits the refitted triangles from the current order pi -- what the oracle's Build does for the
    # triangle sequence w[pi] (same root range, same Subdivide); its tri_indices then index into that sequence
    pi = s.bvh_export(0)[1]
    s.rebuild_bvh(0, P.BUILD_SAH_INTERVALS)
    o = oracle_mesh(tris[pi].reshape(-1, 6), np.arange(3 * len(pi), dtype=np.uint32), P.BUILD_SAH_INTERVALS)
    onodes, otri = o.bvh_export(0)
    nodes, tri = s.bvh_export(0)
    assert np.array_equal(nodes, onodes) and np.array_equal(tri, pi[otri])
    assert not np.array_equal(nodes, t.bvh_export(0)[0])               # the re-split differs from the refitted tree
    s.close(); t.close(); o.close()


# ---- triangle objects, spheres and planes --------------------------------------------------------------------------------
TRI_P = np.array([[-1.0, 0.0, -2.0], [1.0, 0.5, -2.0], [0.0, 2.0, -2.5]], np.float32)
TRI_N = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 0.6, 0.8]], np.float32)


def mixed_scene():
    s = P.Scene()
    s.add_material(P.Material(albedo=(0.5, 0.5, 0.5)))
    s.add_material(P.Material(emissive=(1, 1, 1), intensity=4.0, is_light=True))
    s.add_mesh(P.Mesh.from_arrays(GROUND_V, GROUND_I), 0)                # 0
    s.add_triangle(TRI_P, TRI_N, 0)                                      # 1
    s.add_light(s.add_sphere((1.0, 6.0, -2.0), 1.5, 1))                  # 2
    s.add_plane((0.0, 0.0, 1.0), (0.0, 0.0, -20.0), 0)                   # 3
    v, i = standin_mesh(2)
    s.add_mesh(P.Mesh.from_arrays(v, i), 0)                              # 4
    return s


def flat_bytes(s):
    d = s.flatten()
    def raw(ptr, n, size):
        return C.string_at(C.cast(ptr, C.c_void_p), n * size) if n else b""
    return (raw(d.objects, d.n_objects, C.sizeof(N.Object)), raw(d.nodes, d.n_nodes, 32), raw(d.triangles, d.n_triangles, 72),
            raw(d.tri_indices, d.n_triangles, 4), raw(d.light_indices, d.n_lights, 4))


def test_triangle_object_is_refitted():
    s = mixed_scene()
    moved = np.concatenate([TRI_P + np.float32(0.5), TRI_N[[1, 2, 0]]], axis=1).reshape(1, 18)
    s.refit_mesh(1, moved)
    d = s.flatten()
    o = d.objects[1]
    assert o.kind == N.OBJECT_TRIANGLE
    got = np.ctypeslib.as_array(C.cast(C.pointer(d.triangles[o.tri_offset]), C.POINTER(C.c_float)), shape=(18,))
    assert np.array_equal(got, moved[0])
    s.close()


def test_sphere_and_plane_are_updated():
    s = mixed_scene()
    before = flat_bytes(s)
    s.update_primitive(2, center=(-3.0, 5.0, 1.0), radius=2.25)
    s.update_primitive(3, normal=(0.0, 0.6, 0.8), point=(0.0, -4.0, -18.0))
    d = s.flatten()
    sp, pl = d.objects[2], d.objects[3]
    assert list(sp.sphere_center) == [-3.0, 5.0, 1.0] and sp.sphere_radius == 2.25 and sp.mat_index == 1
    assert list(pl.plane_normal) == [np.float32(0.0), np.float32(0.6), np.float32(0.8)] and list(pl.plane_point) == [0.0, -4.0, -18.0]
    after = flat_bytes(s)
    assert after[1:] == before[1:]                                       # nodes, triangles, indices, lights untouched
    s.update_primitive(2, radius=0.5)                                    # the centre stays
    assert list(s.flatten().objects[2].sphere_center) == [-3.0, 5.0, 1.0] and s.flatten().objects[2].sphere_radius == 0.5
    s.close()


# ---- errors leave the scene unchanged -------------------------------------------------------------------------------------
def test_refit_errors_leave_the_scene_unchanged():
    s = mixed_scene()
    L = N.lib()
    before = flat_bytes(s)
    v, i = standin_mesh(2)
    tris = P.triangles_from_arrays(deform(v, "translate"), i)
    ptr = tris.ctypes.data_as(C.POINTER(N.Triangle))
    n = len(tris)
    cases = [
        ((4, ptr, n - 1), "has %d triangles, got %d" % (n, n - 1)),       # wrong count
        ((4, ptr, n + 1), "a refit keeps the topology"),
        ((1, ptr, 2), "has 1 triangles, got 2"),                        # a triangle object takes one
        ((2, ptr, n), "is a sphere"),                                   # wrong kind
        ((3, ptr, n), "is a plane"),
        ((5, ptr, n), "out of range"),                                  # index
        ((4, None, n), "triangles is null"),                            # NULL
    ]
    for args, msg in cases:
        assert L.cgpth_scene_refit_mesh(s._h, *args) == N.CGPT_ERR_INVALID
        assert msg in L.cgpth_last_error().decode(), (args, L.cgpth_last_error())
        assert flat_bytes(s) == before
    assert L.cgpth_scene_refit_mesh(None, 0, ptr, n) == N.CGPT_ERR_INVALID
    with pytest.raises(P.HostError, match="has 320 triangles, got 319"):
        s.refit_mesh(4, tris[:-1])
    assert flat_bytes(s) == before
    s.close()


def test_update_primitive_errors_leave_the_scene_unchanged():
    s = mixed_scene()
    L = N.lib()
    before = flat_bytes(s)
    sphere = P.scene.primitive_abi(N.OBJECT_SPHERE, 1, (0, 1, 2), 3.0)
    cases = [
        ((2, P.scene.primitive_abi(N.OBJECT_PLANE, 1, normal=(0, 1, 0), point=(0, 0, 0))), "is a sphere, got kind 2"),   # other kind
        ((2, P.scene.primitive_abi(N.OBJECT_SPHERE, 0, (0, 1, 2), 3.0)), "has material 1, got 0"),                     # other material
        ((0, sphere), "is a mesh"),
        ((1, sphere), "is a triangle object"),
        ((5, sphere), "out of range"),
    ]
    for (k, obj), msg in cases:
        assert L.cgpth_scene_update_primitive(s._h, k, C.byref(obj)) == N.CGPT_ERR_INVALID
        assert msg in L.cgpth_last_error().decode(), (k, L.cgpth_last_error())
        assert flat_bytes(s) == before
    assert L.cgpth_scene_update_primitive(s._h, 2, None) == N.CGPT_ERR_INVALID
    assert "obj is null" in L.cgpth_last_error().decode()
    assert flat_bytes(s) == before
    s.close()


def test_triangles_from_arrays_layout():
    v, i = standin_mesh(1)
    t = P.triangles_from_arrays(v, i)
    assert t.dtype == np.float32 and t.shape == (len(i) // 3, 18) and t.flags.c_contiguous
    k = 17
    assert np.array_equal(t[k].reshape(3, 6), v[i[3 * k:3 * k + 3]])
    with pytest.raises(ValueError):
        P.triangles_from_arrays(v[:, :3], i)
    with pytest.raises(ValueError):
        P.triangles_from_arrays(v, i[:-1])
