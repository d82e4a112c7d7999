"""cgpt_scene_rebuild_degraded and Renderer.rebuild_degraded (csrc/device/tree_cost.hip): rebuild the meshes whose trees'
cost has grown past a ratio of a reference, and only those.

Three objects: the 1 280-triangle strip posed to the pinned pose (tree_cost_cases.PINNED_POSE; tests/test_host_tree_cost.py pins, on the
host mirror, that it separates: the refitted tree costs f_refit x the bind tree, the rebuilt one clearly less), a second strip left at
its bind pose, and the ground quad.  The thresholds are the midpoint of 1 and f_refit, which must rebuild the posed strip alone, and
2 f_refit, which must rebuild nothing.  What a rebuild leaves is compared, word for word, with a twin context that called rebuild_mesh."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.renderer import REBUILD_RESULT_DTYPE
from test_gpu_rebuild_mesh import BALL, GROUND, H, SEED, SPP, STRIP, W, fresh, make_scene, strip
from tree_cost_cases import N_STRIP, f_refit, midpoint_ratio, pinned_case

pytestmark = pytest.mark.gpu

SECOND = 4
OBJS = [STRIP, SECOND, GROUND]


def scene(instances=0):
    return make_scene(N_STRIP, extra_meshes=((strip(300, origin=(-2.0, 1.6, 0.2)), 1, P.BUILD_SAH_INTERVALS),), instances=instances)


def pose(r, binds, through=STRIP):
    j, w, n_joints, m = pinned_case(binds[STRIP])
    r.set_skin(through, binds[STRIP], j, w, n_joints)
    r.skin_mesh(through, m)


def exports(r, objs=(STRIP, SECOND)):
    return [r.export_bvh(o) for o in objs]


def image(r):
    r.reset_accumulator()
    r.render(W, H, SPP, seed=SEED, kernel=P.KERNEL_WAVEFRONT)
    return r.accumulator().view(np.uint32).copy()


def same(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(xs, ys))


def test_the_midpoint_rebuilds_the_posed_strip_alone():
    s, binds = scene()
    a, twin = fresh(s), fresh(s)
    first = a.rebuild_degraded(OBJS, midpoint_ratio())                        # at the bind pose: the baselines, and nothing to do
    assert not first["rebuilt"].any() and np.array_equal(first["cost_before"], first["cost_after"])
    bind = first["cost_before"]
    for r in (a, twin):
        pose(r, binds)
    untouched = exports(a, (SECOND,))
    got = a.rebuild_degraded(OBJS, midpoint_ratio())
    assert list(got["rebuilt"]) == [1, 0, 0], got
    assert got["cost_before"][0] > midpoint_ratio() * bind[0] and abs(got["cost_before"][0] / bind[0] / f_refit() - 1.0) < 1e-9   # the mirror's factor
    assert got["cost_after"][0] < got["cost_before"][0]
    assert np.array_equal(got["cost_before"][1:], bind[1:]) and np.array_equal(got["cost_after"][1:], bind[1:])
    twin.rebuild_mesh(STRIP, P.BUILD_SAH_BINNED)
    assert same(exports(a, (STRIP,)), exports(twin, (STRIP,)))                # word for word what rebuild_mesh leaves
    assert same(exports(a, (SECOND,)), untouched) and a.export_bvh(GROUND).shape[0] == 1
    assert np.array_equal(image(a), image(twin))
    assert a.tree_costs([STRIP])[0]["cost"] == got["cost_after"][0]
    # the baseline was replaced by the rebuilt tree's cost: the same call again finds nothing to do
    again = a.rebuild_degraded(OBJS, midpoint_ratio())
    assert not again["rebuilt"].any() and again["cost_before"][0] == got["cost_after"][0]
    for r in (a, twin):
        r.close()
    s.close()


def test_twice_f_refit_rebuilds_nothing_and_keeps_the_temporal_history():
    s, binds = scene()
    a = fresh(s)
    a.rebuild_degraded(OBJS, 2.0 * f_refit())
    pose(a, binds)
    before_image = image(a); a.denoise_temporal(); image(a); a.denoise_temporal()
    history = a.temporal_history()
    assert history[..., 3].max() > SPP
    before = exports(a)
    got = a.rebuild_degraded(OBJS, 2.0 * f_refit())
    assert not got["rebuilt"].any() and np.array_equal(got["cost_before"], got["cost_after"])
    assert same(exports(a), before) and np.array_equal(a.temporal_history().view(np.uint32), history.view(np.uint32))
    assert np.array_equal(image(a), before_image)
    a.denoise_temporal()
    assert a.temporal_history()[..., 3].max() > history[..., 3].max()          # the history was kept and went on growing
    a.close(); s.close()


def test_rebuild_mesh_replaces_the_baseline():
    s, binds = scene()
    a = fresh(s)
    a.rebuild_degraded([STRIP], midpoint_ratio())                             # the baseline: the bind tree
    pose(a, binds)
    a.rebuild_mesh(STRIP, P.BUILD_SAH_BINNED)                                 # costs more than midpoint x the bind tree, but is the new baseline
    got = a.rebuild_degraded([STRIP], midpoint_ratio())
    assert not got["rebuilt"].any()
    a.upload(s)                                                               # an upload drops it: measured again at first use, on the bind tree ...
    assert not a.rebuild_degraded([STRIP], midpoint_ratio())["rebuilt"].any()
    pose(a, binds)
    assert a.rebuild_degraded([STRIP], midpoint_ratio())["rebuilt"].all()     # ... which the pose exceeds; the rebuilt tree's baseline would not be
    a.close(); s.close()


def test_an_instanced_group_named_through_two_placements_is_rebuilt_once():
    s, binds = scene(instances=2)                                             # placements 0, 5, 6 of the strip's one copy
    a, twin = fresh(s, instanced=True), fresh(s, instanced=True)
    assert a.scene_footprint().n_mesh_copies == 3
    objs = [5, SECOND, STRIP]
    a.rebuild_degraded(objs, midpoint_ratio())
    for r in (a, twin):
        pose(r, binds, through=5)
    records = a.scene_footprint().n_pair_records
    got = a.rebuild_degraded(objs, midpoint_ratio())
    assert list(got["rebuilt"]) == [1, 0, 1]                                  # both placements reach the rebuilt copy
    assert got["cost_before"][0] == got["cost_before"][2] and got["cost_after"][0] == got["cost_after"][2] < got["cost_before"][0]
    assert a.scene_footprint().n_pair_records == records + N_STRIP - 1        # one span
    twin.rebuild_mesh(5, P.BUILD_SAH_BINNED)                                  # one rebuild
    assert same(exports(a, (STRIP, 5, 6, SECOND)), exports(twin, (STRIP, 5, 6, SECOND)))
    for r in (a, twin):
        r.close()
    s.close()


def test_a_two_member_context_stays_equal_across_its_members():
    s, binds = scene()
    one, g = fresh(s), fresh(s, [0, 0], P.CTX_GATHER_PEER_COPY)
    results = []
    for r in (one, g):
        r.rebuild_degraded(OBJS, midpoint_ratio())
        pose(r, binds)
        results.append(r.rebuild_degraded(OBJS, midpoint_ratio()))
    assert np.array_equal(results[0].view(np.uint8), results[1].view(np.uint8)) and list(results[1]["rebuilt"]) == [1, 0, 0]
    assert same(exports(one), exports(g))
    assert np.array_equal(image(one), image(g))                               # the group's image is made of both members' bands
    assert np.array_equal(one.tree_costs(OBJS).view(np.uint8), g.tree_costs(OBJS).view(np.uint8))   # every member sums the same bits, or the call fails
    one.close(); g.close(); s.close()


def test_refusals_come_before_any_rebuild():
    L = N.lib()
    s, binds = scene()
    a, twin = fresh(s), fresh(s)
    bind = a.tree_costs(OBJS)["cost"]
    for r in (a, twin):
        pose(r, binds)
    before, before_image = exports(a), image(a)
    out = np.zeros(3, REBUILD_RESULT_DTYPE)
    out["cost_before"] = -7.0
    sentinel = out.copy()

    def call(objs, refs, ratio, option=P.BUILD_SAH_BINNED, c_inner=1.0, c_tri=1.0, results=out, n=None):
        rows = (N.RebuildCandidate * max(1, len(objs)))(*[N.RebuildCandidate(int(o), 0, float(c)) for o, c in zip(objs, refs)])
        rc = L.cgpt_scene_rebuild_degraded(a._ctx, rows if objs else None, len(objs) if n is None else n, ratio, option, c_inner, c_tri,
                                           None if results is None else results.ctypes.data_as(C.POINTER(N.RebuildResult)))
        return rc, L.cgpt_last_error(a._ctx).decode()

    mid = midpoint_ratio()
    assert call([], [], mid, n=0)[0] == N.CGPT_OK
    assert call([], [], mid, n=3)[0] == N.CGPT_ERR_INVALID and call(OBJS, bind, mid, results=None)[0] == N.CGPT_ERR_INVALID
    for bad in (0.0, -1.0, float("inf"), float("nan")):                       # the posed strip comes first in every one of these: it must not be rebuilt
        assert call(OBJS, bind, bad)[0] == N.CGPT_ERR_INVALID
        assert call(OBJS, bind, mid, c_inner=bad)[0] == N.CGPT_ERR_INVALID and call(OBJS, bind, mid, c_tri=bad)[0] == N.CGPT_ERR_INVALID
        rc, message = call(OBJS, [bind[0], bad, bind[2]], mid)
        assert rc == N.CGPT_ERR_INVALID and "entry 1" in message and "reference_cost" in message, message
    rc, message = call(OBJS, bind, mid, option=4)
    assert rc == N.CGPT_ERR_INVALID and "unknown build option" in message
    rc, message = call(OBJS, bind, mid, option=P.BUILD_SAH_PRIMITIVES)
    assert rc == N.CGPT_ERR_UNSUPPORTED and "never splits" in message
    for obj, text in ((7, "out of range"), (BALL, "no mesh")):
        rc, message = call([STRIP, SECOND, obj], bind, mid)
        assert rc == N.CGPT_ERR_INVALID and text in message and "entry 2" in message, message
    assert np.array_equal(out.view(np.uint8), sentinel.view(np.uint8))
    assert same(exports(a), before) and np.array_equal(image(a), before_image)

    # the binned build's domain is checked on the device: entry 1 is refused mid-call, entry 0 stays rebuilt and valid
    far = binds[SECOND].copy()
    far[100, 6] = np.float32(1e31)
    a.refit_mesh(SECOND, far)
    rc, message = call(OBJS, [bind[0], 1e-3, bind[2]], mid)                   # a reference that any cost exceeds
    assert rc == N.CGPT_ERR_INVALID and message.startswith("entry 1:") and "finite positions of magnitude <= 1e30" in message, message
    assert np.array_equal(out.view(np.uint8), sentinel.view(np.uint8))
    twin.rebuild_mesh(STRIP, P.BUILD_SAH_BINNED)
    twin.refit_mesh(SECOND, far)
    costs = a.tree_costs([STRIP])[0]
    a._node_counts[STRIP] = int(costs["n_inner"] + costs["n_leaves"])          # the raw call went round the Renderer's bookkeeping
    assert same(exports(a), exports(twin)) and np.array_equal(image(a), image(twin))
    for r in (a, twin):
        r.close()
    s.close()


def test_the_example_rebuilds_only_where_the_call_says_so(tmp_path):
    """render_main --bend 15 --rebuild-ratio R: a cost line a frame and posed mesh; with a ratio nothing reaches no mesh is rebuilt and the
    temporal history is kept (the last frame's temporal image differs from its denoised one), with a ratio below 1 every frame rebuilds"""
    from cpugpupathtracing_amd import build as B
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(B.REPO_DIR, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(B.REPO_DIR, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt", "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    for ratio, rebuilt in (("1e9", False), ("0.5", True)):
        out = subprocess.run([exe, "--bend", "15", "--rebuild-ratio", ratio, "64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        lines = [l for l in out.stdout.splitlines() if "tree cost" in l]
        assert len(lines) == 8 and all(lines[k].startswith(f"frame {k}: object 0 ") for k in range(8)), out.stdout
        assert [("rebuilt" in l) for l in lines] == [rebuilt] * 8, out.stdout
        same_images = [(tmp_path / f"bend_{k:02d}_denoised.ppm").read_bytes() == (tmp_path / f"bend_{k:02d}_temporal.ppm").read_bytes() for k in range(8)]
        assert all(same_images) if rebuilt else (same_images[0] and not same_images[7]), same_images
