"""BUILD_SAH_BINNED on the GPU (csrc/device/bvh_build.hip: binned_*) against the host mirror (csrc/host/mesh_bvh.cpp: BuildTreeBinned),
which tests/test_host_binned_build.py holds to the numpy restatement: every 32-byte node word, every tri index, n_nodes, max_depth and the
total_area bytes equal, under the default level borders and under each forced level strategy.  The oracle has no binned build; it
checks what is traced through a binned tree (the closest hit does not depend on the tree)."""
import ctypes as C
import time

import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from test_host_binned_build import soup_mesh

pytestmark = pytest.mark.gpu

BINNED = P.BUILD_SAH_BINNED
MESHES = {f"standin{level}": (lambda level=level: P.Mesh.dragon_standin(level)) for level in (0, 2, 4, 5)}
MESHES.update({f"soup{n}": (lambda seed=seed, n=n: soup_mesh(seed, n)) for seed, n in ((2, 1), (3, 2), (4, 3), (5, 17), (6, 257), (7, 1000), (8, 5000), (9, 40000))})
# CGPT_BVH_PIECE_TRIS, CGPT_BVH_WAVE_TRIS, CGPT_BVH_QUARTER_TRIS (None: the defaults)
STRATEGIES = {"default": None, "pieces_of_one_triangle": (1, 2048, 32), "workgroups_only": (10 ** 9, 0, 0), "wavefronts_only": (10 ** 9, 10 ** 9, 0),
              "quarter_wavefronts_only": (10 ** 9, 10 ** 9, 10 ** 9)}


@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(0)
    yield r
    r.close()


_host_cache = {}


def host_build(name):
    """the host mirror's binned tree of MESHES[name], built once: (mesh, scene, triangle pointer, n_tris, (nodes, tri, depth, area))"""
    if name not in _host_cache:
        mesh = MESHES[name]()
        s = P.Scene()
        s.add_material(P.Material())
        s.add_mesh(mesh, 0, BINNED)
        nodes, tri = s.bvh_export(0)
        info = s.bvh_info(0)
        desc = s.flatten()
        obj = desc.objects[0]
        ptr = C.cast(C.addressof(desc.triangles.contents) + obj.tri_offset * C.sizeof(N.Triangle), C.POINTER(N.Triangle))
        _host_cache[name] = (mesh, s, desc, ptr, obj.tri_count, (np.asarray(nodes).view(np.uint32).reshape(-1, 8).copy(), np.asarray(tri).copy(), info.max_depth, info.total_area))
    return _host_cache[name]


def assert_same(host, gpu, who="host mirror"):
    hn, ht, hd, ha = host
    gn, gt, gd, ga = gpu
    assert gn.shape == hn.shape, (who, gn.shape, hn.shape)                                         # n_nodes
    assert np.array_equal(gt, ht), f"tri order differs from the {who}'s at {np.flatnonzero(gt != ht)[:8]}"
    bad = np.flatnonzero((gn != hn).any(axis=1))
    assert bad.size == 0, f"{bad.size} nodes differ from the {who}'s, first {bad[:8]}: gpu {gn[bad[0]]} {who} {hn[bad[0]]}"
    assert gd == hd, (who, gd, hd)
    assert np.float32(ga).tobytes() == np.float32(ha).tobytes(), (who, ga, ha)


@pytest.mark.parametrize("strategy", list(STRATEGIES))
@pytest.mark.parametrize("name", list(MESHES))
def test_gpu_tree_equals_the_host_mirror(renderer, monkeypatch, name, strategy):
    if STRATEGIES[strategy] is not None:
        for var, value in zip(("CGPT_BVH_PIECE_TRIS", "CGPT_BVH_WAVE_TRIS", "CGPT_BVH_QUARTER_TRIS"), STRATEGIES[strategy]):
            monkeypatch.setenv(var, str(value))
    _, _, _, ptr, n_tris, host = host_build(name)
    assert_same(host, renderer.build_bvh(ptr, n_tris, BINNED))


@pytest.mark.parametrize("name", ["standin4", "soup5000"])
def test_device_rebuild_from_a_permuted_order(renderer, name):
    """cgpt_bvh_build_ex with initial_tri_indices: the binned build over that order == the host Rebuild from it (the stable partition
    keeps the order inside each side, so the order inside a leaf of several triangles is the starting order's)"""
    mesh, _, _, ptr, n_tris, _ = host_build(name)
    s = P.Scene()
    s.add_material(P.Material())
    s.add_mesh(mesh, 0, P.BUILD_NAIVE)                                     # leaves a permuted order behind
    _, start = s.bvh_export(0)
    start = np.asarray(start).copy()
    assert not np.array_equal(start, np.arange(n_tris))
    s.rebuild_bvh(0, BINNED)
    nodes, tri = s.bvh_export(0)
    info = s.bvh_info(0)
    host = (np.asarray(nodes).view(np.uint32).reshape(-1, 8), np.asarray(tri), info.max_depth, info.total_area)
    assert_same(host, renderer.build_bvh(ptr, n_tris, BINNED, start))


@pytest.mark.parametrize("first", [P.BUILD_SAH_INTERVALS, BINNED])
def test_scene_rebuild_with_the_device_builder(renderer, first):
    """options 1 -> 3 and 3 -> 3 through Scene.rebuild_bvh(device_builder=...) == the same on the host"""
    for mesh in (P.Mesh.dragon_standin(4), soup_mesh(7, 3000)):
        scenes = []
        for builder in (None, renderer):
            s = P.Scene()
            s.add_material(P.Material())
            s.add_mesh(mesh, 0, first, device_builder=builder)
            s.rebuild_bvh(0, BINNED, device_builder=builder)
            scenes.append(s)
        (hn, ht), (gn, gt) = scenes[0].bvh_export(0), scenes[1].bvh_export(0)
        hi, gi = scenes[0].bvh_info(0), scenes[1].bvh_info(0)
        assert_same((np.asarray(hn).view(np.uint32).reshape(-1, 8), np.asarray(ht), hi.max_depth, hi.total_area),
                    (np.asarray(gn).view(np.uint32).reshape(-1, 8), np.asarray(gt), gi.max_depth, gi.total_area))
        assert gi.nodes_used == hi.nodes_used > 1


# ---- what is traced and rendered through a binned tree ---------------------------------------------------------------------------
RAY_SEED = 20261


def binned_scene(option=BINNED):
    mesh = P.Mesh.dragon_standin(3)
    s = P.Scene()
    for m in P.REFERENCE_MATERIALS:
        s.add_material(m)
    s.add_mesh(mesh, 3, option)
    s.add_light(s.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -3.0, 0.0), 1)
    s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    return mesh, s


def oracle_scene(mesh, option):
    o = O.OracleScene()
    for m in P.REFERENCE_MATERIALS:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light)
    o.add_mesh(mesh.vertices, mesh.indices, 3, option)
    o.add_light(o.add_sphere((10.0, 10.0, 10.0), 5.0, 2))
    o.add_plane((0.0, 1.0, 0.0), (0.0, -3.0, 0.0), 1)
    o.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    return o


def ray_set(mesh, o):
    """64 x 64 camera rays plus 20 000 random rays aimed at the mesh"""
    co, cd = o.camera_rays(64, 64)
    pos = np.asarray(mesh.vertices, np.float32).reshape(-1, 6)[:, :3]
    center, extent = (pos.min(axis=0) + pos.max(axis=0)) / 2, (pos.max(axis=0) - pos.min(axis=0)) / 2
    rng = np.random.default_rng(RAY_SEED)
    n = 20000
    ro = (center + rng.uniform(-1, 1, (n, 3)) * extent * 4).astype(np.float32)         # inside and around the mesh
    target = (center + rng.uniform(-1, 1, (n, 3)) * extent).astype(np.float32)
    rd = (target - ro).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([co.reshape(-1, 3), ro]).astype(np.float32), np.concatenate([cd.reshape(-1, 3), rd.astype(np.float32)]).astype(np.float32)


def test_closest_hits_through_a_binned_tree_equal_the_oracle(renderer):
    """t, obj and tri of cgpt_intersect_rays on the binned tree, bit for bit the oracle's on its own SAH_INTERVALS tree.  The oracle's
    NAIVE and SAH_INTERVALS trees agree on every ray of this set (checked here on the CPU): the closest hit does not depend on the tree."""
    mesh, s = binned_scene()
    o = oracle_scene(mesh, O.BUILD_SAH_INTERVALS)
    origins, dirs = ray_set(mesh, o)
    want_t, want_obj, want_tri, _ = o.intersect_rays(origins, dirs)
    naive = oracle_scene(mesh, O.BUILD_NAIVE)
    nt, nobj, ntri, _ = naive.intersect_rays(origins, dirs)
    assert np.array_equal(nt.view(np.uint32), want_t.view(np.uint32)) and np.array_equal(nobj, want_obj) and np.array_equal(ntri, want_tri)
    hit_mesh = np.count_nonzero(want_obj == 0)
    assert hit_mesh > 5000, hit_mesh                                           # the set does exercise the mesh
    renderer.upload(s)
    t, obj, tri, _ = renderer.intersect_rays(origins, dirs)
    assert np.array_equal(obj, want_obj), np.count_nonzero(obj != want_obj)
    assert np.array_equal(t.view(np.uint32), want_t.view(np.uint32)), np.count_nonzero(t.view(np.uint32) != want_t.view(np.uint32))
    assert np.array_equal(tri, want_tri), np.count_nonzero(tri != want_tri)


@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_BRUTE_FORCE])
def test_every_render_path_agrees_on_a_binned_tree(renderer, mode):
    _, s = binned_scene()
    renderer.upload(s)
    settings = P.Settings(render_mode=mode)
    frames = []
    for kernel in (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT, P.KERNEL_AUTO):
        renderer.reset_accumulator()
        renderer.render(32, 32, 4, seed=0x2468ACE, kernel=kernel, settings=settings)
        frames.append(renderer.accumulator().view(np.uint32).copy())
    assert np.count_nonzero(frames[0]) > 0
    for k, f in enumerate(frames[1:], 1):
        assert np.array_equal(frames[0], f), f"kernel {k}: {np.count_nonzero(frames[0] != f)} words differ from the megakernel's"


def test_device_refit_of_a_binned_tree_equals_the_host_refit(renderer):
    mesh, s = binned_scene()
    renderer.upload(s)
    assert np.array_equal(renderer.export_bvh(0), np.asarray(s.bvh_export(0)[0]).view(np.uint32).reshape(-1, 8))
    rng = np.random.default_rng(5)
    tris = P.triangles_from_arrays(mesh.vertices, mesh.indices).copy()
    tris.reshape(-1, 3, 6)[:, :, :3] += rng.normal(0, 0.05, (tris.shape[0], 3, 3)).astype(np.float32)
    area = renderer.refit_mesh(0, tris)
    s.refit_mesh(0, tris)
    host = np.asarray(s.bvh_export(0)[0]).view(np.uint32).reshape(-1, 8)
    dev = renderer.export_bvh(0)
    assert np.array_equal(dev, host), f"{np.count_nonzero(dev != host)} words differ"
    assert np.float32(area).tobytes() == np.float32(s.bvh_info(0).total_area).tobytes()


def test_refusals(renderer):
    mesh = P.Mesh.dragon_standin(1)
    s = P.Scene()
    s.add_material(P.Material())
    s.add_mesh(mesh, 0, P.BUILD_SAH_INTERVALS)
    desc = s.flatten()
    n_tris = desc.objects[0].tri_count
    with pytest.raises(P.DeviceError, match="unknown build option"):
        renderer.build_bvh(desc.triangles, n_tris, 7)
    with pytest.raises(P.DeviceError, match="unknown build option"):
        renderer.build_bvh(desc.triangles, n_tris, 4)
    for bad in (np.nan, 2e30):
        tris = P.triangles_from_arrays(mesh.vertices, mesh.indices).copy()
        tris[11, 7] = bad                                                    # v1.pos.y of triangle 11
        ptr = tris.ctypes.data_as(C.POINTER(N.Triangle))
        with pytest.raises(P.DeviceError, match="1e30") as e:
            renderer.build_bvh(ptr, n_tris, BINNED)
        assert e.value.code == N.CGPT_ERR_INVALID
    good = renderer.build_bvh(desc.triangles, n_tris, BINNED)                # the context is still usable
    assert good[0].shape[0] > 1
    with pytest.raises(P.HostError):
        s.add_mesh(mesh, 0, 4, device_builder=renderer)
    with pytest.raises(P.HostError):
        s.rebuild_bvh(0, 4, device_builder=renderer)


def test_build_time_host_vs_device_both_options(renderer):
    """prints, asserts nothing: stand-in level 7 (327,680 triangles), both options, host and device"""
    mesh = P.Mesh.dragon_standin(7)
    for name, option in (("SAH intervals", P.BUILD_SAH_INTERVALS), ("SAH binned", BINNED)):
        t = []
        for builder in (None, renderer, renderer):
            s = P.Scene()
            s.add_material(P.Material())
            t0 = time.perf_counter()
            s.add_mesh(mesh, 0, option, device_builder=builder)
            t.append(time.perf_counter() - t0)
        print(f"327,680 triangles, {name}: host build {t[0] * 1e3:.0f} ms, device build {t[2] * 1e3:.0f} ms (first call {t[1] * 1e3:.0f} ms)")
