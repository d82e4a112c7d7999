"""cgpt_scene_tree_costs (csrc/device/tree_cost.hip): the surface-area cost of uploaded meshes' trees, summed on the device.

The yardstick is tests/tree_cost_ref.py over the same context's own export_bvh: cost and root_half_area agree to the derived bound
(tree_cost_ref.tolerance: (n_nodes + 16) 2^-52 relative, the two sides differ in the order of two sums of non-negative terms), the counts
exactly.  The shapes are the smallest that reach each way the kernels can go wrong: 255 records (one partial block), 599 (two blocks and
a ragged tail), 1 279 (several), a 3-node tree of the small-mesh class, leaf roots (no launch), and records a refit, a batch pose and a
first and second rebuild have written, among the top slots and in the span at the end of node_pairs."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.renderer import TREE_COST_DTYPE
from skin_cases import make_case
from test_gpu_rebuild_mesh import BALL, GROUND, H, SEED, SPP, STRIP, W, bend_case, fresh, make_scene, strip
from tree_cost_cases import TWO, cube
from tree_cost_ref import tolerance, tree_cost

pytestmark = pytest.mark.gpu

CONSTANTS = ((1.0, 1.0), (1.5, 0.25))
S256, TWO_OBJ, CUBE_OBJ = 4, 5, 6


def raw(x):
    return np.ascontiguousarray(x).view(np.uint8)


def assert_agrees(r, obj, constants=CONSTANTS):
    nodes = r.export_bvh(obj)
    for c_inner, c_tri in constants:
        got, want = r.tree_costs([obj], c_inner, c_tri)[0], tree_cost(nodes, c_inner, c_tri)
        assert (got["n_inner"], got["n_leaves"], got["max_leaf_tris"], got["reserved"]) == (want.n_inner, want.n_leaves, want.max_leaf_tris, 0), (obj, got, want)
        tol = tolerance(len(nodes))
        assert abs(got["cost"] - want.cost) <= tol * abs(want.cost), (obj, got["cost"], want.cost, tol)
        assert abs(got["root_half_area"] - want.root_half_area) <= tol * abs(want.root_half_area), (obj, got["root_half_area"], want.root_half_area)
    return got


def mixed_scene(n=600):
    """objects: 0 the n-strip, 1 the ground quad, 2 a sphere, 3 the light, 4 a 256-strip, 5 two far triangles (3 nodes), 6 a cube"""
    return make_scene(n, extra_meshes=((strip(256, origin=(-2.0, 1.6, 0.2)), 1, P.BUILD_SAH_INTERVALS), (TWO, 0, P.BUILD_SAH_INTERVALS),
                                       (cube((1.0, 2.5, -1.0)), 1, P.BUILD_SAH_BINNED)))


@pytest.fixture(scope="module")
def mixed():
    s, binds = mixed_scene()
    r = fresh(s)
    yield s, binds, r
    r.close(); s.close()


# ---- agreement with the statement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 600, 1280])
def test_a_strip_agrees_with_the_statement(n):
    s, _ = make_scene(n)
    r = fresh(s)
    assert r.export_bvh(STRIP).shape[0] == 2 * n - 1                          # n - 1 records: 255, 599, 1 279
    got = assert_agrees(r, STRIP)
    assert (got["n_inner"], got["n_leaves"]) == (n - 1, n)
    r.close(); s.close()


def test_small_meshes_and_leaf_roots(mixed):
    s, _, r = mixed
    assert r.export_bvh(TWO_OBJ).shape[0] == 3 and r.export_bvh(GROUND).shape[0] == 1
    for obj in (TWO_OBJ, CUBE_OBJ, S256):
        assert_agrees(r, obj)
    # the ground quad never splits: the host fills c_tri n_tris without a launch
    for c_inner, c_tri in CONSTANTS:
        got = r.tree_costs([GROUND], c_inner, c_tri)[0]
        assert tuple(got) == (c_tri * 2, 0.0, 0, 1, 2, 0)
    assert_agrees(r, GROUND)
    s2, _ = make_scene(1280, P.BUILD_SAH_PRIMITIVES)                          # a large leaf root
    r2 = fresh(s2)
    assert tuple(r2.tree_costs([STRIP, GROUND])[0]) == (1280.0, 0.0, 0, 1, 1280, 0)
    r2.close(); s2.close()


def test_after_a_refit_a_batch_pose_and_two_rebuilds():
    s, binds = mixed_scene(1280)
    r = fresh(s)
    bind_cost = r.tree_costs([STRIP])[0]["cost"]
    moved = binds[STRIP].copy()
    moved[:, 1::6] *= np.float32(1.7); moved[:, 2::6] += np.float32(0.25) * moved[:, 0::6]
    r.refit_mesh(STRIP, moved)                                                # bounds rewritten by the refit
    assert assert_agrees(r, STRIP)["cost"] != bind_cost
    j, w, n_joints, m = bend_case(binds[STRIP])
    r.set_skin(STRIP, binds[STRIP], j, w, n_joints)
    j2, w2, n2, m2 = make_case("bend", binds[S256], seed=2)
    r.set_skin(S256, binds[S256], j2, w2, n2)
    r.pose_objects([(STRIP, m, None), (S256, m2, None)])                      # ... by the batch
    posed = assert_agrees(r, STRIP)["cost"]
    assert_agrees(r, S256)
    r.rebuild_mesh(STRIP, P.BUILD_SAH_INTERVALS)                              # first rebuild: the top slots and the span at the end of node_pairs
    first = assert_agrees(r, STRIP)["cost"]
    assert first < posed
    r.rebuild_mesh(S256, P.BUILD_NAIVE)                                       # a second span behind the first
    assert_agrees(r, S256)
    r.rebuild_mesh(STRIP, P.BUILD_NAIVE)                                      # second rebuild: the span reused
    assert assert_agrees(r, STRIP)["cost"] != first
    for obj in (TWO_OBJ, CUBE_OBJ):                                           # the untouched neighbours still agree
        assert_agrees(r, obj, CONSTANTS[:1])
    r.close(); s.close()


def test_a_leaf_root_grown_by_a_rebuild():
    s, _ = make_scene(1280, P.BUILD_SAH_PRIMITIVES)                           # one node: no old records, the span alone
    r = fresh(s)
    assert r.tree_costs([STRIP])[0]["n_inner"] == 0
    n_nodes, _ = r.rebuild_mesh(STRIP, P.BUILD_SAH_BINNED)
    got = assert_agrees(r, STRIP)
    assert got["n_inner"] + got["n_leaves"] == n_nodes > 1
    r.close(); s.close()


# ---- determinism ----------------------------------------------------------------------------------------------------------------------
def test_a_batch_returns_each_entrys_own_bits_at_any_position(mixed):
    _, _, r = mixed
    batch = [STRIP, GROUND, S256, STRIP]
    got = r.tree_costs(batch, 1.5, 0.25)
    assert np.array_equal(raw(got), raw(r.tree_costs(batch, 1.5, 0.25)))      # a repeated call
    for k, obj in enumerate(batch):
        assert np.array_equal(raw(got[k:k + 1]), raw(r.tree_costs([obj], 1.5, 0.25))), k
    assert np.array_equal(raw(got[0:1]), raw(got[3:4]))
    back = r.tree_costs(batch[::-1] + [CUBE_OBJ, TWO_OBJ], 1.5, 0.25)
    assert np.array_equal(raw(back[:4][::-1]), raw(got))


def test_instanced_placements_report_equal_bits():
    s, _ = make_scene(600, instances=2)                                       # placements 0, 4, 5 of one copy
    one, r = fresh(s, instanced=False), fresh(s, instanced=True)
    assert r.scene_footprint().n_mesh_copies == 2
    got = r.tree_costs([STRIP, 4, 5])
    assert np.array_equal(raw(got[0:1]), raw(got[1:2])) and np.array_equal(raw(got[0:1]), raw(got[2:3]))
    assert np.array_equal(raw(got), raw(one.tree_costs([STRIP, 4, 5])))       # ... and the per-object copies' bits
    assert_agrees(r, 4)
    one.close(); r.close(); s.close()


def test_a_two_member_context_reports_the_one_device_bits(mixed):
    s, _, r = mixed
    g = fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY)
    batch = [STRIP, S256, GROUND, TWO_OBJ, CUBE_OBJ]
    assert np.array_equal(raw(g.tree_costs(batch)), raw(r.tree_costs(batch)))
    g.close()


def test_on_a_callers_stream(mixed):
    import torch
    _, _, r = mixed
    want = r.tree_costs([STRIP, S256])
    side = torch.cuda.Stream()
    r.set_stream(side)
    try:
        assert np.array_equal(raw(r.tree_costs([STRIP, S256])), raw(want))
    finally:
        r.set_stream(None)


# ---- the call only reads ---------------------------------------------------------------------------------------------------------------
def test_the_call_changes_nothing_and_keeps_the_temporal_history():
    s, _ = mixed_scene()
    r = fresh(s)

    def frame():
        r.reset_accumulator()
        r.render(W, H, SPP, seed=SEED, kernel=P.KERNEL_WAVEFRONT)
        return r.accumulator().view(np.uint32).copy()

    image = frame(); r.denoise_temporal(); frame(); r.denoise_temporal()
    history = r.temporal_history()
    assert history[..., 3].max() > SPP
    exports = [r.export_bvh(o) for o in (STRIP, S256, TWO_OBJ)]
    guides = r.guides()
    r.tree_costs([STRIP, GROUND, S256, TWO_OBJ, CUBE_OBJ])
    assert np.array_equal(raw(r.temporal_history()), raw(history))
    assert all(np.array_equal(a, r.export_bvh(o)) for a, o in zip(exports, (STRIP, S256, TWO_OBJ)))
    assert np.array_equal(raw(r.guides()), raw(guides))
    assert np.array_equal(frame(), image)
    r.denoise_temporal()
    assert r.temporal_history()[..., 3].max() > history[..., 3].max()          # the history went on growing: no generation moved
    r.close(); s.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_and_the_scene_untouched():
    L = N.lib()
    r = P.Renderer(0)
    with pytest.raises(P.DeviceError) as e:
        r.tree_costs([0])
    assert e.value.code == N.CGPT_ERR_NO_SCENE
    tri = (np.float32([[-1.0, 2.5, 2.0], [1.25, 2.5, 2.0], [0.0, 3.0, 2.5]]), np.float32([0, 0, 1]))
    s, binds = make_scene(257)
    assert s.add_triangle(*tri, 0) == 4
    assert s.add_plane((0.0, 0.0, 1.0), (0.0, 0.0, -30.0), 1) == 5
    r.upload(s)
    before = r.export_bvh(STRIP)
    out = np.zeros(2, TREE_COST_DTYPE)
    out["cost"] = -7.0
    sentinel = out.copy()
    objs = np.uint32([STRIP, STRIP])

    def call(objs_ptr, n, c_inner, c_tri, out_ptr):
        return L.cgpt_scene_tree_costs(r._ctx, objs_ptr, n, c_inner, c_tri, out_ptr)

    op, outp = objs.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(N.TreeCost))
    assert call(None, 2, 1.0, 1.0, outp) == N.CGPT_ERR_INVALID
    assert call(op, 2, 1.0, 1.0, None) == N.CGPT_ERR_INVALID
    assert call(None, 0, 1.0, 1.0, None) == N.CGPT_OK                         # n == 0: nothing to do
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(op, 2, bad, 1.0, outp) == N.CGPT_ERR_INVALID and call(op, 2, 1.0, bad, outp) == N.CGPT_ERR_INVALID
    for obj, text in ((6, "out of range"), (BALL, "no mesh"), (5, "no mesh"), (4, "no mesh")):
        objs[1] = obj
        assert call(op, 2, 1.0, 1.0, outp) == N.CGPT_ERR_INVALID
        message = L.cgpt_last_error(r._ctx).decode()
        assert text in message and "entry 1" in message, message
    assert np.array_equal(raw(out), raw(sentinel))
    # a bound that is not finite: the entry is named and `out` stays unwritten
    far = binds[STRIP].copy()
    far[100, 6] = np.float32(np.inf)
    r.refit_mesh(STRIP, far)
    objs[:] = (GROUND, STRIP)
    assert call(op, 2, 1.0, 1.0, outp) == N.CGPT_ERR_INVALID
    message = L.cgpt_last_error(r._ctx).decode()
    assert "entry 1" in message and "not finite" in message, message
    assert np.array_equal(raw(out), raw(sentinel))
    r.refit_mesh(STRIP, binds[STRIP])
    assert np.array_equal(r.export_bvh(STRIP), before)
    assert r.tree_costs([STRIP])[0]["cost"] > 0
    r.close(); s.close()
