"""wf_shade resolves the rays that the top of IntersectScene decides by itself (wf_shade: "Probe"; rt_device.hpp probe_scene): a shadow ray
or a diffuse bounce ray that misses both halves of every mesh's root box and every analytic object (or ends on a sphere, a plane or a
leaf triangle, for a shadow ray) never reaches the trace kernel.  The knob `probe` must never change a result: every case renders the
wavefront pipeline with probe 1 and 0 and compares accumulator and pixels bit for bit with each other, with the megakernel and with the
persistent kernel, and the traced rays with the oracle's (every decided ray is still one IntersectScene call).  stats.probe_resolved
shows that the probe ran where it should and nowhere else."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from scenes import GROUND_I, GROUND_V, MAT_SPEC_DIFFUSE, reference_layout_pair, standin_mesh
from test_gpu_glossy import _glossy_layout
from test_gpu_triangle_objects import Pair, many_objects, no_meshes, occluder, visible_surfaces

pytestmark = pytest.mark.gpu

W, H = 45, 37                  # not multiples of the 8x8 tile: the edge tiles are padded
SEED = 0x2468ACE1
GLASS, SPEC_DIFFUSE = 3, 4
BANDS_ON = {"bands": 4, "bands_min_paths": 0}   # image bands even for these small batches
ORACLE_MODE = {P.MODE_ADVANCED: O.MODE_ADVANCED, P.MODE_BRUTE_FORCE: O.MODE_BRUTE_FORCE, P.MODE_COMPARISON: O.MODE_COMPARISON}


def _counters(st):
    return (st.traced_rays, st.inner_steps, st.tri_tests, st.bvh_depth_sum, st.closest_hits)


def _layout(material=GLASS, level=3, depth=5):
    return reference_layout_pair(*standin_mesh(level), material, aspect=W / H, extra_materials=(MAT_SPEC_DIFFUSE,),
                                 settings=P.Settings(max_ray_depth=depth))


def _render(s, kernel, spp, knobs=None, counters=False, settings=None, first=0, rows=None, interleave=None, size=(W, H)):
    r = P.Renderer(0)
    try:
        r.upload(s)
        if knobs:
            r.set_tuning(**knobs)
        if first:                                                    # the same history for every kernel
            r.render(size[0], size[1], first, seed=SEED, kernel=P.KERNEL_MEGAKERNEL, settings=settings, rows=rows, interleave=interleave)
        r.reset_stats()
        r.render(size[0], size[1], spp, seed=SEED, kernel=kernel, counters=counters, settings=settings, rows=rows, interleave=interleave)
        return r.accumulator().copy(), r.pixels().copy(), r.stats(), r.n_rows
    finally:
        r.close()


def _check(s, spp, knobs=None, o=None, mode=P.MODE_ADVANCED, settings=None, resolves=True, **kw):
    """probe 1 and 0 against the megakernel and the persistent kernel; traced rays against the oracle `o` (rendered from sample 0).
    resolves: True -> some rays are decided, False -> none, None -> not asserted.  Returns the stats of the probe-1 render."""
    knobs = knobs or {}
    size = kw.get("size", (W, H))
    ref_acc, ref_px, ref_st, n_rows = _render(s, P.KERNEL_MEGAKERNEL, spp, settings=settings, **kw)
    acc, px, st, _ = _render(s, P.KERNEL_PERSISTENT, spp, settings=settings, **kw)
    assert np.array_equal(acc.view(np.uint32), ref_acc.view(np.uint32)) and np.array_equal(px, ref_px)
    assert st.traced_rays == ref_st.traced_rays and st.probe_resolved == 0 and ref_st.probe_resolved == 0
    if o is not None:
        o.reset_accumulator(); o.reset_stats()
        o.render(size[0], size[1], spp, ORACLE_MODE[mode], O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
        assert o.stats().traced_rays == ref_st.traced_rays
    on = None
    for probe in (1, 0):
        acc, px, st, _ = _render(s, P.KERNEL_WAVEFRONT, spp, {**knobs, "probe": probe}, settings=settings, **kw)
        assert st.last_kernel == P.KERNEL_WAVEFRONT
        assert np.array_equal(acc.view(np.uint32), ref_acc.view(np.uint32)), (probe, knobs)
        assert np.array_equal(px, ref_px), (probe, knobs)
        assert st.traced_rays == ref_st.traced_rays, (probe, knobs, st.traced_rays, ref_st.traced_rays)
        primaries = size[0] * n_rows * spp
        assert st.probe_resolved <= st.traced_rays - primaries, (probe, st.probe_resolved, st.traced_rays, primaries)
        if probe == 0:
            assert st.probe_resolved == 0
        else:
            on = st
            if resolves is not None:
                assert (st.probe_resolved > 0) == resolves, (knobs, st.probe_resolved)
    return on


# ---- the bench layout (glass stand-in, ground quad, two sphere lights) under the knobs that reorder or reroute its rays ----------------

@pytest.mark.parametrize("knobs", [
    {"batch": 8}, {"batch": 8, **BANDS_ON}, {"batch": 8, "spec_dedupe": 0}, {"batch": 8, "spec_dedupe": 1, **BANDS_ON},
    {"batch": 8, "retire_misses": 0}, {"batch": 8, "retire_misses": 1, "spec_dedupe": 0, **BANDS_ON},
    {"batch": 5, "path_order": 0}, {"batch": 5, "path_order": 1}, {"batch": 5, "path_order": 2}, {"batch": 1}, {},
], ids=str)
def test_bench_layout(knobs):
    o, s = _layout()
    st = _check(s, 24, knobs, o=o)
    # most later-round rays of this layout are ground-pixel shadow rays and bounce rays into the sky
    assert st.probe_resolved > (st.traced_rays - W * H * 24) // 4


def test_decided_share_does_not_depend_on_the_election_or_the_lists():
    _, s = _layout()
    got = {str(k): _render(s, P.KERNEL_WAVEFRONT, 16, {"batch": 8, **k})[2].probe_resolved
           for k in ({}, {"spec_dedupe": 0}, BANDS_ON, {"retire_misses": 0}, {"path_order": 0}, {"pools": 1})}
    assert len(set(got.values())) == 1 and min(got.values()) > 0, got


def test_c2_diffuse_and_specular_material():
    o, s = _layout(SPEC_DIFFUSE)
    _check(s, 32, {"batch": 16}, o=o)


@pytest.mark.parametrize("depth", [0, 1, 2, 8])
def test_max_depth(depth):
    o, s = _layout(depth=depth)
    _check(s, 16, {"batch": 8}, o=o)                                # depth 0: no bounce ray, but the first hit's shadow ray is probed


# ---- other object kinds ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", [visible_surfaces, occluder, no_meshes], ids=lambda f: f.__name__)
def test_plane_and_triangle_objects(scene):
    p = scene()
    assert len(p.kinds) <= 8
    _check(p.s, 16, {"batch": 8}, o=p.o)


def _leaf_root_scene(two_leaves=False):
    """every mesh has a leaf root (the ground quad: the probe tests its two triangles).  two_leaves: a mesh of two quads far apart as
    well, whose root is an inner node with two leaf children: the probe walks the children its slab test hits"""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=10.0, is_light=True))
    if two_leaves:
        quad = np.array([[-6, 1, -2, 0, 0, 1], [-6, -3, -2, 0, 0, 1], [-2, -3, -2, 0, 0, 1], [-2, 1, -2, 0, 0, 1]], np.float32)
        far = quad + np.array([14.0, 0, -3.0, 0, 0, 0], np.float32)
        p.mesh(np.vstack([quad, far]), np.concatenate([GROUND_I, GROUND_I + 4]), grey)
    p.mesh(GROUND_V, GROUND_I, grey)
    p.sphere((2.0, -1.5, 1.0), 1.5, grey)
    p.light(p.sphere((0.0, 10.0, 5.0), 3.0, light))
    p.camera(aspect=W / H)
    return p


@pytest.mark.parametrize("two_leaves", [False, True])
def test_mesh_with_a_leaf_root_or_leaf_children(two_leaves):
    p = _leaf_root_scene(two_leaves)
    assert p.s.bvh_info(1 if two_leaves else 0).nodes_used == 1
    if two_leaves:
        assert p.s.bvh_info(0).nodes_used == 3 and p.s.bvh_info(0).num_leaves == 2
    _check(p.s, 16, {"batch": 8}, o=p.o)


def test_mesh_light():
    """shadow rays aimed at the triangles of a mesh light; the stand-in is one 320-triangle leaf (never entered by the probe: its root
    is a leaf, so its triangles ARE the probe's work)"""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1, 1, 1), intensity=5.0, is_light=True))
    shiny = p.material(P.Material(albedo=(0.9, 0.9, 0.9), specular=0.8))
    lv = np.array([[-10, 20, 10, 0, -1, 0], [-10, 20, -10, 0, -1, 0], [10, 20, -10, 0, -1, 0], [10, 20, 10, 0, -1, 0]], np.float32)
    p.mesh(*standin_mesh(2), shiny)
    p.plane((0, 1, 0), (0, -3, 0), grey)
    p.light(p.mesh(lv, GROUND_I, light))
    p.camera(aspect=W / H)
    _check(p.s, 16, {"batch": 8}, o=p.o)


def test_closed_box_around_the_camera():
    """six planes around everything: no bounce ray leaves the scene, so only shadow rays can be decided"""
    p = Pair()
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=10.0, is_light=True))
    p.mesh(*standin_mesh(2), grey)
    for n, pt in (((0, 1, 0), (0, -3, 0)), ((0, -1, 0), (0, 14, 0)), ((1, 0, 0), (-11, 0, 0)), ((-1, 0, 0), (11, 0, 0)), ((0, 0, 1), (0, 0, -11)),
                  ((0, 0, -1), (0, 0, 12))):
        p.plane(n, pt, grey)
    p.light(p.sphere((3.0, 9.0, 3.0), 2.0, light))
    p.camera(aspect=W / H)
    _check(p.s, 16, {"batch": 8}, o=p.o)


def test_more_objects_than_probe_max_objects():
    p = many_objects()                                               # 48 objects: past the trace kernels' LDS object table too
    _check(p.s, 8, {"batch": 4, "probe_max_objects": 47}, o=p.o, resolves=False)
    _check(p.s, 8, {"batch": 4}, o=p.o, resolves=True)               # (the default is 128)
    p = visible_surfaces()                                           # 8 objects
    _check(p.s, 8, {"batch": 4, "probe_max_objects": 7}, resolves=False)
    _check(p.s, 8, {"batch": 4, "probe_max_objects": 8}, resolves=True)
    _check(p.s, 8, {"batch": 4, "probe_max_objects": 0}, resolves=False)


@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_COMPARISON])
def test_axis_parallel_centre_ray(mode):
    """the camera looks straight down at a half-mirror plane from an even-sized frame: the centre ray is (0, -1, 0), its mirror bounce
    (0, 1, 0), and rays around it are nearly so: zero direction components take the NaN-exact slab test and are left to the trace kernel"""
    p = Pair()
    half = p.material(P.Material(albedo=(0.8, 0.8, 0.8), specular=0.5))
    light = p.material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=10.0, is_light=True))
    grey = p.material(P.Material(albedo=(0.6, 0.6, 0.6)))
    p.plane((0, 1, 0), (0, -3, 0), half)
    p.mesh(*standin_mesh(2), grey)
    p.light(p.sphere((9.0, 12.0, 0.0), 3.0, light))
    p.camera(pos=(6.0, 9.0, 0.0), view_dir=(0, -1, 0), aspect=46 / 38)
    _check(p.s, 16, {"batch": 8}, o=p.o, mode=mode, settings=P.Settings(render_mode=mode), size=(46, 38))


# ---- glossy lobes, TracePath renders, debug views, counting kernels ------------------------------------------------------------------

def test_glossy_scene():
    s = _glossy_layout(aspect=W / H)
    _check(s, 16, {"batch": 8})
    _check(s, 16, {"batch": 8, **BANDS_ON}, settings=P.Settings(render_mode=P.MODE_COMPARISON))


def test_comparison_and_brute_force():
    o, s = _layout()
    _check(s, 16, {"batch": 8}, o=o, mode=P.MODE_COMPARISON, settings=P.Settings(render_mode=P.MODE_COMPARISON))   # right half: TracePathAdvanced
    _check(s, 16, {"batch": 8}, o=o, mode=P.MODE_BRUTE_FORCE, settings=P.Settings(render_mode=P.MODE_BRUTE_FORCE), resolves=False)


@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views_are_not_probed(debug):
    _, s = _layout()
    _check(s, 4, {"batch": 2}, settings=P.Settings(debug_render_mode=debug), resolves=False)


def test_counting_kernels_keep_the_oracle_counters():
    o, s = _layout()
    o.reset_accumulator(); o.reset_stats()
    o.render(W, H, 16, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    for probe in (1, 0):
        _, _, st, _ = _render(s, P.KERNEL_WAVEFRONT, 16, {"batch": 8, "probe": probe}, counters=True)
        assert _counters(st) == _counters(o.stats())
        assert st.probe_resolved == 0


# ---- resumed renders, bands of rows, several devices -------------------------------------------------------------------------------------

def test_resumed_render_in_several_batches_and_pools():
    _, s = _layout()
    _check(s, 26, {"batch": 4, "pools": 3}, first=7)
    _check(s, 26, {"batch": 4, "pools": 1, **BANDS_ON}, first=300)


def test_row_band_and_interleaved_band():
    _, s = _layout()
    _check(s, 16, {"batch": 8}, rows=(5, 30))
    for rank in range(3):
        _check(s, 16, {"batch": 8, **BANDS_ON}, interleave=(3, 3, rank))


def test_one_renderer_switching_the_knob_between_calls():
    """the knob is read at every render: the same context, accumulating, with probe 1, 0, 1"""
    _, s = _layout()
    r, ref = P.Renderer(0), P.Renderer(0)
    try:
        r.upload(s); ref.upload(s)
        r.set_tuning(batch=4)
        for probe in (1, 0, 1):
            r.set_tuning(probe=probe)
            r.reset_stats()
            r.render(W, H, 8, seed=SEED, kernel=P.KERNEL_WAVEFRONT)
            ref.render(W, H, 8, seed=SEED, kernel=P.KERNEL_MEGAKERNEL)
            assert np.array_equal(r.accumulator().view(np.uint32), ref.accumulator().view(np.uint32)), probe
            assert (r.stats().probe_resolved > 0) == (probe == 1)
    finally:
        r.close(); ref.close()


def test_shared_gpu_multi_device_context():
    _, s = _layout()
    ref_acc, ref_px, ref_st, _ = _render(s, P.KERNEL_MEGAKERNEL, 12)
    resolved = {}
    for probe in (1, 0):
        g = P.Renderer([0, 0, 0], flags=P.CTX_GATHER_PEER_COPY)
        try:
            g.upload(s)
            g.set_tuning(batch=4, probe=probe)
            g.reset_stats()
            g.render(W, H, 12, seed=SEED, kernel=P.KERNEL_WAVEFRONT)
            assert np.array_equal(g.accumulator().view(np.uint32), ref_acc.view(np.uint32)), probe
            assert np.array_equal(g.pixels(), ref_px), probe
            st = g.stats()
            assert st.traced_rays == ref_st.traced_rays and st.n_devices == 3
            resolved[probe] = st.probe_resolved
        finally:
            g.close()
    single = _render(s, P.KERNEL_WAVEFRONT, 12, {"batch": 4})[2].probe_resolved
    assert resolved[0] == 0 and resolved[1] == single > 0          # the ranks' shares add up to the one-device count
