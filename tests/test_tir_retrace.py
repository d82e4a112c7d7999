"""A ray traced again after total internal reflection is not walked.  The reference leaves the ray as it is when the
smooth dielectric finds k < 0 -- t, obj and tri included -- and calls IntersectScene on it again (SURVEY A-3); every intersector accepts
only t < ray.t, so the call returns the hit it starts from.  The production kernels take that hit without a walk, and shade_bounce runs
the iterations stuck on such a hit in place where the material samples no light.  Nothing may change: every case compares accumulator
and pixels of the three kernels bit for bit with each other and with their counting instantiations (counters=True: they still walk), the
traced rays with the oracle's, and the counting kernels' step counts with the oracle's and with each other (under the top-level tree,
where the oracle's list walk enters meshes the tree skips, the oracle's inner_steps and tri_tests are upper bounds and the three counting
kernels must still agree).  stats.retrace_unwalked shows that the short cut ran where it should and nowhere else."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from scenes import GROUND_I, GROUND_V
from test_gpu_triangle_objects import Pair

pytestmark = pytest.mark.gpu

W, H = 45, 37                  # not multiples of the 8x8 tile: the edge tiles are padded
SEED = 0x2468ACE1
KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT)
GLASS = P.Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, absorption=(0.2, 0.8, 0.8), ior=1.517)   # the bench's: roulette never ends the path
ORACLE_MODE = {P.MODE_ADVANCED: O.MODE_ADVANCED, P.MODE_BRUTE_FORCE: O.MODE_BRUTE_FORCE, P.MODE_COMPARISON: O.MODE_COMPARISON}
ORACLE_DEBUG = {P.DEBUG_NONE: O.DEBUG_NONE, P.DEBUG_RAY_DEPTH: O.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH: O.DEBUG_BVH_DEPTH}


def prism_mesh():
    """a closed box of 12 triangles with face normals, turned so that three faces see the camera: a ray that enters one face meets the
    neighbouring faces from inside beyond the critical angle"""
    a, b = np.radians(33.0), np.radians(24.0)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    rot = rx @ ry
    half = np.array([1.9, 1.4, 1.6])
    verts, idx = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            n = np.zeros(3); n[axis] = sign
            u, v = np.zeros(3), np.zeros(3)
            u[(axis + 1) % 3] = 1.0; v[(axis + 2) % 3] = 1.0
            base = len(verts)
            for cu, cv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = (n + cu * u + cv * v) * half
                verts.append(np.concatenate([rot @ p + np.array([0.0, -0.4, 0.0]), rot @ n]))
            idx += [base, base + 1, base + 2, base + 2, base + 3, base] if sign > 0 else [base, base + 2, base + 1, base + 2, base, base + 3]
    return np.ascontiguousarray(verts, np.float32), np.asarray(idx, np.uint32)


def ico_mesh(level=2):
    m = P.Mesh.bumpy_icosphere(level, (0.0, -0.3, 0.0), (2.4, 2.0, 2.2), 0.25)
    return m.vertices, m.indices


def scene(mesh, glass=GLASS, depth=5, nee=True, rr=True) -> Pair:
    """a closed glass mesh over a diffuse ground, one sphere light"""
    p = Pair()
    p.settings = dict(max_ray_depth=depth, next_event_estimation_enabled=nee, russian_roulette_enabled=rr)
    p.o.set_settings(depth, nee, True, rr)
    p.s.set_settings(P.Settings(**p.settings))
    grey = p.material(P.Material(albedo=(0.7, 0.7, 0.7)))
    light = p.material(P.Material(emissive=(1.0, 0.95, 0.8), intensity=10.0, is_light=True))
    g = p.material(glass)
    p.mesh(*mesh, g)
    p.mesh(GROUND_V, GROUND_I, grey)
    p.light(p.sphere((6.0, 9.0, 6.0), 3.0, light))
    p.camera(aspect=W / H)
    return p


def _render(s, kernel, spp, knobs=None, counters=False, settings=None, top_level=False):
    r = P.Renderer(0)
    try:
        if top_level:
            r.set_top_level(True)
        r.upload(s)
        if knobs:
            r.set_tuning(**knobs)
        r.render(W, H, spp, seed=SEED, kernel=kernel, counters=counters, settings=settings)
        return r.accumulator().copy(), r.pixels().copy(), r.stats()
    finally:
        r.close()


def _steps(st):
    return (st.inner_steps, st.tri_tests, st.bvh_depth_sum)


def check(p: Pair, spp, knobs=None, unwalked=True, oracle=True, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE, top_level=False, kernels=KERNELS):
    """unwalked: True -> every production render answered some rays without a walk, False -> none did.  oracle: the scene is one the
    oracle can state.  Returns the production stats per kernel."""
    settings = P.Settings(**p.settings, render_mode=mode, debug_render_mode=debug)
    want = None
    if oracle:
        p.o.reset_accumulator(); p.o.reset_stats()
        p.o.render(W, H, spp, ORACLE_MODE[mode], ORACLE_DEBUG[debug], O.RNG_PIXEL_PCG, SEED, nthreads=8)
        want = p.o.stats()
    first, out = None, {}
    for kernel in kernels:
        kn = knobs if kernel == P.KERNEL_WAVEFRONT else None
        acc, px, st = _render(p.s, kernel, spp, kn, settings=settings, top_level=top_level)
        cacc, cpx, cst = _render(p.s, kernel, spp, kn, counters=True, settings=settings, top_level=top_level)
        what = (kernel, knobs)
        assert st.last_kernel == kernel, what
        assert np.array_equal(acc.view(np.uint32), cacc.view(np.uint32)) and np.array_equal(px, cpx), what
        assert st.traced_rays == cst.traced_rays, (what, st.traced_rays, cst.traced_rays)
        assert cst.retrace_unwalked == 0, what                       # the counting kernels walk every ray
        assert (st.retrace_unwalked > 0) == unwalked, (what, st.retrace_unwalked)
        assert st.retrace_unwalked <= st.traced_rays - W * H * spp, what
        if want is not None:
            assert st.traced_rays == want.traced_rays, (what, st.traced_rays, want.traced_rays)
            if not top_level:
                assert _steps(cst) == _steps(want), what
            else:
                # the oracle walks the object list.  The tree does not enter a mesh whose box the ray misses: the root step of the glass mesh
                # and the two triangle tests of the ground quad (a leaf root) are then not executed; what a walk finds is the same
                assert cst.bvh_depth_sum == want.bvh_depth_sum and cst.inner_steps <= want.inner_steps and cst.tri_tests <= want.tri_tests, what
        if first is None:
            first = (acc, px, st.traced_rays, _steps(cst))
        else:
            assert np.array_equal(acc.view(np.uint32), first[0].view(np.uint32)) and np.array_equal(px, first[1]), what
            assert st.traced_rays == first[2], what
            assert _steps(cst) == first[3], what                      # the counting kernels agree on every step count, tree or list
        out[kernel] = st
    return out


# ---- the two meshes at the three sample counts (72: a wave of the wavefront pipeline is not one pixel) -------------------------------

@pytest.mark.parametrize("spp", [4, 16, 72])
@pytest.mark.parametrize("mesh", [prism_mesh, ico_mesh], ids=["prism", "icosphere"])
def test_glass_mesh(mesh, spp):
    check(scene(mesh()), spp, {"batch": 8} if spp != 72 else None)


def test_no_refractive_material_nothing_unwalked():
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.9, 0.9, 0.9), specular=0.6)), 16, {"batch": 8}, unwalked=False)


# ---- a material for every way out of the stuck iterations ----------------------------------------------------------------------------

def test_every_unwalked_ray_is_absorbed_when_the_glass_samples_no_light():
    """refractivity 1: the stuck iterations run inside shade_bounce to the depth limit; the trace kernel of the wavefront pipeline never
    sees a ray to trace again, so nothing changes with the election off"""
    p = scene(prism_mesh())
    a = check(p, 16, {"batch": 8, "spec_dedupe": 1}, kernels=(P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT))
    b = check(p, 16, {"batch": 8, "spec_dedupe": 0}, kernels=(P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT))
    counts = {st.retrace_unwalked for st in list(a.values()) + list(b.values())}
    assert len(counts) == 1, counts                                   # one count of stuck iterations, whoever runs them


def test_mirror_lobe_ends_the_stuck_iterations():
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.95, 0.95, 0.95), specular=0.5, refractivity=0.5, ior=1.517), depth=8), 16, {"batch": 8})


def test_glass_with_a_diffuse_share_samples_lights():
    """NEE applies on the refractive surface: the iterations are not absorbed, each re-traced ray is answered where it would be traced"""
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.9, 0.9, 0.9), refractivity=0.6, ior=1.517), depth=8), 16, {"batch": 8})


def test_glass_with_a_diffuse_share_without_lights_to_sample():
    """the same material with NEE off: absorbed, and the diffuse lobe is a way out"""
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.9, 0.9, 0.9), refractivity=0.6, ior=1.517), depth=8, nee=False), 16, {"batch": 8})


def test_roulette_ends_a_path_inside_the_stuck_iterations():
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.5, 0.5, 0.5), refractivity=1.0, ior=1.517), depth=8), 16, {"batch": 8})


def test_russian_roulette_off():
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.5, 0.5, 0.5), refractivity=1.0, ior=1.517), rr=False), 16, {"batch": 8})
    check(scene(ico_mesh(1), rr=False), 16, {"batch": 8})


@pytest.mark.parametrize("depth", [1, 2, 5, 8])
def test_max_ray_depth(depth):
    # depth 1: the ray enters at depth 0 and meets the inside at depth 1, where the loop ends whatever is drawn: no ray is traced again
    check(scene(prism_mesh(), depth=depth), 16, {"batch": 8}, unwalked=depth >= 2)
    check(scene(prism_mesh(), glass=P.Material(albedo=(0.9, 0.9, 0.9), refractivity=0.6, ior=1.517), depth=depth), 16, {"batch": 8}, unwalked=depth >= 2)


# ---- the other instantiations ----------------------------------------------------------------------------------------------------------

def test_rough_transmission_has_no_ray_to_trace_again():
    """GLOSSY >= 2: a facet with k < 0 reflects; the smooth glass next to it in the same instantiation still takes the short cut"""
    rough = P.Material(albedo=(1.0, 1.0, 1.0), refractivity=1.0, ior=1.517, transmission_roughness=0.3)
    check(scene(prism_mesh(), glass=rough), 16, {"batch": 8}, unwalked=False, oracle=False)
    p = scene(prism_mesh())
    p.s.add_mesh(P.Mesh.from_arrays(*ico_mesh(1)), p.s.add_material(rough))
    p.s.set_transform(3, [[0.4, 0, 0, 3.5], [0, 0.4, 0, 1.5], [0, 0, 0.4, 1.0]])
    check(p, 16, {"batch": 8}, oracle=False)


def test_smooth_normals():
    p = scene(ico_mesh())
    p.s.set_smooth_normals(0, True)
    check(p, 16, {"batch": 8}, oracle=False)


def test_transformed_mesh():
    p = scene(prism_mesh())
    c, s = np.cos(0.4), np.sin(0.4)
    p.s.set_transform(0, [[1.1 * c, 0, 1.1 * s, 0.3], [0, 0.9, 0, 0.2], [-1.1 * s, 0, 1.1 * c, -0.5]])
    check(p, 16, {"batch": 8}, oracle=False)


def test_top_level_tree():
    check(scene(ico_mesh()), 16, {"batch": 8}, top_level=True)


def test_comparison_mode():
    check(scene(prism_mesh()), 16, {"batch": 8}, mode=P.MODE_COMPARISON)          # left half: TracePath, whose glass returns black instead


def test_brute_force_has_no_ray_to_trace_again():
    check(scene(prism_mesh()), 8, {"batch": 8}, mode=P.MODE_BRUTE_FORCE, unwalked=False)


@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views(debug):
    # the ray-depth view shows the depth the stuck iterations counted up to; the BVH-depth view ends every path at its primary hit
    check(scene(prism_mesh()), 4, {"batch": 2}, debug=debug, unwalked=debug == P.DEBUG_RAY_DEPTH)


# ---- the wavefront pipeline's knobs ----------------------------------------------------------------------------------------------------

NEE_GLASS = P.Material(albedo=(0.9, 0.9, 0.9), refractivity=0.6, ior=1.517)    # its re-traced rays reach the trace kernel


@pytest.mark.parametrize("glass", [GLASS, NEE_GLASS], ids=["absorbed", "answered_in_trace"])
@pytest.mark.parametrize("knobs", [{"spec_dedupe": 0}, {"spec_dedupe": 1}, {"probe": 0}, {"probe": 1}, {"retire_misses": 0}, {"retire_misses": 1},
                                   {"spec_dedupe": 0, "probe": 0, "retire_misses": 0}, {"bands": 4, "bands_min_paths": 0}, {"pools": 1, "batch": 3}], ids=str)
def test_wavefront_knobs(glass, knobs):
    p = scene(prism_mesh(), glass=glass, depth=8)
    check(p, 16, {"batch": 8, **knobs}, kernels=(P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT))


def test_camera_inside_the_glass():
    """a primary hit can be total internal reflection: round 0 of the wavefront pipeline hands the hit record and its hit byte on"""
    p = scene(prism_mesh(), glass=NEE_GLASS, depth=6)
    p.camera(pos=(0.0, -0.4, 0.0), view_dir=(0.3, -0.2, -1.0), fov=100.0, aspect=W / H)
    check(p, 16, {"batch": 8})
    p = scene(prism_mesh(), depth=6)
    p.camera(pos=(0.0, -0.4, 0.0), view_dir=(0.3, -0.2, -1.0), fov=100.0, aspect=W / H)
    check(p, 16, {"batch": 8, "retire_misses": 0})


# ---- the ray query keeps walking: a finite tmax there is a bound, not a known hit ------------------------------------------------------

def test_ray_query_with_finite_tmax():
    p = scene(ico_mesh())
    rng = np.random.default_rng(5)
    n = 4096
    o = np.tile(np.array([0.0, 0.0, 8.0], np.float32), (n, 1))
    d = rng.normal(size=(n, 3)).astype(np.float32) * np.array([0.35, 0.35, 0.0], np.float32) + np.array([0.0, 0.0, -1.0], np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    r = P.Renderer(0)
    try:
        r.upload(p.s)
        t0, obj0, tri0, _ = r.intersect_rays(o, d)
        hit = obj0 != 0xFFFFFFFF
        assert hit.sum() > n // 2
        for scale in (1.5, 1.0, 0.5):                                 # beyond the hit, exactly the hit (strict: not found again), before it
            tmax = np.where(hit, t0 * np.float32(scale), np.float32(7.0)).astype(np.float32)
            got = r.intersect_rays(o, d, tmax)
            want = p.o.intersect_rays(o, d, tmax)
            for g, w in zip(got, want):
                assert np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)), scale
            if scale == 1.5:
                assert np.array_equal(got[1][hit], obj0[hit]) and np.array_equal(got[0][hit].view(np.uint32), t0[hit].view(np.uint32))
            if scale == 1.0:
                assert (got[1][hit] == 0xFFFFFFFF).all() and np.array_equal(got[0].view(np.uint32), tmax.view(np.uint32))
    finally:
        r.close()
