"""GPU parity: the HIP path through the C ABI against the CPU oracle on the same seeded inputs.

Tolerance: north_star asks RMSE < 1e-4 per pixel at matched seeds.  Everything except Beer's-law expf is expected to
be bit-identical (same float operation order, no FMA, IEEE div/sqrt), so non-glass scenes additionally assert exact equality.
"""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from scenes import MAT_SPEC_DIFFUSE, forty_object_pair, pair_from as _pair_from, quad_stack as _quad_stack, reference_layout_pair, rmse, standin_mesh

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4   # per-pixel RMSE on the float4 accumulator / n (north_star)


@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(0)
    yield r
    r.close()


def _render_pair(renderer, o, s, W, H, spp, kernel=P.KERNEL_MEGAKERNEL, seed=0x12345678):
    o.render(W, H, spp, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, seed, nthreads=8)
    renderer.upload(s)
    renderer.reset_accumulator(); renderer.reset_stats()
    renderer.render(W, H, spp, seed=seed, kernel=kernel, counters=True)
    return o.accumulator(), renderer.accumulator()


@pytest.mark.parametrize("level", [2, 4])
def test_intersect_rays_bit_exact(renderer, level):
    v, i = standin_mesh(level)
    o, s = reference_layout_pair(v, i, 1)
    renderer.upload(s)
    rng = np.random.default_rng(7)
    n = 20000
    origins = np.tile(np.array([0, 0, 8], np.float32), (n, 1)) + rng.normal(0, 0.5, (n, 3)).astype(np.float32)
    target = np.stack([rng.uniform(-8, 8, n), rng.uniform(-4, 4, n), rng.uniform(-10, 0, n)], 1).astype(np.float32)
    d = target - origins
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    # axis-aligned directions exercise the inf/NaN slab cases (SURVEY A-18)
    d[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    origins[:6] = np.array([0, 0, -4.97], np.float32)
    t0, obj0, tri0, dep0 = o.intersect_rays(origins, d)
    t1, obj1, tri1, dep1 = renderer.intersect_rays(origins, d)
    assert np.array_equal(obj0, obj1)
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32))
    hit = obj0 != 0xFFFFFFFF
    assert np.array_equal(tri0[hit], tri1[hit])
    assert np.array_equal(dep0, dep1)
    assert hit.sum() > n // 4


@pytest.mark.parametrize("mat,exact", [(1, True), (4, True), (3, False)])
def test_render_matches_oracle(renderer, mat, exact):
    v, i = standin_mesh(3)
    o, s = reference_layout_pair(v, i, mat, extra_materials=(MAT_SPEC_DIFFUSE,))
    W = H = 96
    spp = 4
    a0, a1 = _render_pair(renderer, o, s, W, H, spp)
    assert np.array_equal(a0[..., 3], a1[..., 3])
    e = rmse(a0[..., :3] / spp, a1[..., :3] / spp)
    assert e < RMSE_TOL, f"RMSE {e}"
    so, sg = o.stats(), renderer.stats()
    assert (so.traced_rays, so.inner_steps, so.tri_tests, so.bvh_depth_sum, so.closest_hits) == \
           (sg.traced_rays, sg.inner_steps, sg.tri_tests, sg.bvh_depth_sum, sg.closest_hits)
    if exact:
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
        assert np.array_equal(o.pixels(), renderer.pixels())
    assert abs(so.total_energy_received - sg.total_energy_received) < 1e-6 * max(1.0, so.total_energy_received)


# ---- behaviour of the Render() boundary ----------------------------------------------------------------------------------

def test_accumulation_continues_across_calls_and_reset(renderer):
    v, i = standin_mesh(2)
    o, s = reference_layout_pair(v, i, 4, extra_materials=(MAT_SPEC_DIFFUSE,))
    W, H = 64, 48
    o.render(W, H, 5, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 9, nthreads=4)
    renderer.upload(s)
    renderer.reset_accumulator()
    renderer.render(W, H, 2, seed=9)
    renderer.render(W, H, 3, seed=9)            # first_sample continues at 2 (data.num_accumulated, ref: Main.cpp:702)
    assert renderer.num_accumulated == 5 and renderer.stats().num_accumulated == 5
    assert np.array_equal(renderer.accumulator().view(np.uint32), o.accumulator().view(np.uint32))
    assert np.array_equal(renderer.pixels(), o.pixels())
    renderer.reset_accumulator()                # ref: Main.cpp:238-243
    assert not renderer.accumulator().any()
    renderer.render(W, H, 5, seed=9)
    assert np.array_equal(renderer.accumulator().view(np.uint32), o.accumulator().view(np.uint32))


@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_checkpoint_resume_is_bit_identical(kernel, tmp_path):
    """f-3: render 6 spp, dump accumulator + num_accumulated to a file, NEW context, load, render 4 more == 10 spp straight
    (data.accumulator / data.num_accumulated, ref: Main.cpp:204-205,238-243); whole image and an interleaved band."""
    from cpugpupathtracing_amd import distributed as D
    from cpugpupathtracing_amd.scene import read_accumulator as read_accumulator_file, write_accumulator as write_accumulator_file
    v, i = standin_mesh(3)
    o, s = reference_layout_pair(v, i, 3)
    W, H = 72, 52
    o.render(W, H, 10, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 11, nthreads=4)
    for il in (None, (4, 3, 1)):
        a = P.Renderer(0)
        a.upload(s)
        a.render(W, H, 6, seed=11, kernel=kernel, interleave=il)
        path = str(tmp_path / "ckpt.acc")
        write_accumulator_file(path, a.accumulator(), a.num_accumulated)
        a.render(W, H, 4, seed=11, kernel=kernel, interleave=il)
        straight, straight_px = a.accumulator().copy(), a.pixels().copy()
        a.close()

        b = P.Renderer(0)                        # a fresh context: nothing rendered, no framebuffer yet
        b.upload(s)
        acc, n = read_accumulator_file(path, W, straight.shape[0])
        assert n == 6
        b.load_accumulator(acc, n, W, H, interleave=il)
        assert b.stats().num_accumulated == 6
        assert np.array_equal(b.accumulator().view(np.uint32), acc.view(np.uint32))
        assert np.array_equal(b.pixels(), D.pack_pixels(acc, 6))            # data.pixels re-packed from the loaded sums
        b.render(W, H, 4, seed=11, kernel=kernel, interleave=il)
        assert b.num_accumulated == 10
        assert np.array_equal(b.accumulator().view(np.uint32), straight.view(np.uint32))
        assert np.array_equal(b.pixels(), straight_px)
        if il is None:
            assert rmse(b.accumulator()[..., :3] / 10, o.accumulator().reshape(H, W, 4)[..., :3] / 10) < 1e-4
        # wrong size is refused
        with pytest.raises(P.DeviceError):
            b.load_accumulator(acc[:-1], n, W, H, interleave=il)
        b.close()


@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (50, 33), (130, 70)])
def test_sizes_not_multiple_of_16_render_every_pixel(renderer, W, H):
    # the reference writes out of bounds here (SURVEY A-1); every pixel must be rendered, none outside touched
    v, i = standin_mesh(2)
    o, s = reference_layout_pair(v, i, 1, aspect=W / H)
    a0, a1 = _render_pair(renderer, o, s, W, H, 2)
    assert a1.shape == (H, W, 4) and np.all(a1[..., 3] == 2.0)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))


def test_row_bands_equal_full_image(renderer):
    v, i = standin_mesh(3)
    _, s = reference_layout_pair(v, i, 3, aspect=96 / 64)
    renderer.upload(s)
    renderer.reset_accumulator()
    renderer.render(96, 64, 3, seed=5)
    full = renderer.accumulator()
    for rows in ((0, 20), (20, 41), (41, 64)):
        renderer.render(96, 64, 3, seed=5, rows=rows)      # a band change re-allocates a zeroed band
        band = renderer.accumulator()
        assert band.shape == (rows[1] - rows[0], 96, 4)
        assert np.array_equal(band.view(np.uint32), full[rows[0]:rows[1]].view(np.uint32))


@pytest.mark.parametrize("settings", [
    P.Settings(next_event_estimation_enabled=False),
    P.Settings(cosine_weighted_diffuse_reflection_enabled=False),
    P.Settings(russian_roulette_enabled=False, max_ray_depth=3),
    P.Settings(max_ray_depth=0),
])
def test_settings_variants_match_oracle(renderer, settings):
    v, i = standin_mesh(2)
    o, s = reference_layout_pair(v, i, 4, extra_materials=(MAT_SPEC_DIFFUSE,), settings=settings)
    a0, a1 = _render_pair(renderer, o, s, 64, 64, 3)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert o.stats().traced_rays == renderer.stats().traced_rays


@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views_match_oracle(renderer, debug):
    v, i = standin_mesh(3)
    st = P.Settings(debug_render_mode=debug)
    o, s = reference_layout_pair(v, i, 3, settings=st)
    o.render(64, 64, 1, O.MODE_ADVANCED, debug, O.RNG_PIXEL_PCG, 3, nthreads=2)
    renderer.upload(s)
    renderer.reset_accumulator()
    renderer.render(64, 64, 1, seed=3)
    assert np.array_equal(renderer.pixels(), o.pixels())
    assert not renderer.accumulator().any()       # debug views bypass the accumulator (ref: Main.cpp:743-746)


def test_mesh_light_and_plane_objects(renderer):
    # quad mesh light (the commented-out light of ref: Main.cpp:802-814) over a plane floor and a mirror-ish blob
    v, i = standin_mesh(2)
    o = O.OracleScene(); s = P.Scene()
    mats = [P.Material(albedo=(0.7, 0.7, 0.7)), P.Material(emissive=(1, 1, 1), intensity=5.0, is_light=True),
            P.Material(albedo=(0.9, 0.9, 0.9), specular=0.8)]
    for m in mats:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light); s.add_material(m)
    lv = np.array([[-10, 20, 10, 0, -1, 0], [-10, 20, -10, 0, -1, 0], [10, 20, -10, 0, -1, 0], [10, 20, 10, 0, -1, 0]], np.float32)
    li = np.array([0, 1, 2, 2, 3, 0], np.uint32)
    o.add_mesh(v, i, 2, O.BUILD_NAIVE); s.add_mesh(P.Mesh.from_arrays(v, i), 2, P.BUILD_NAIVE)
    o.add_plane((0, 1, 0), (0, -3, 0), 0); s.add_plane((0, 1, 0), (0, -3, 0), 0)
    lo = o.add_mesh(lv, li, 1, O.BUILD_SAH_INTERVALS); ls = s.add_mesh(P.Mesh.from_arrays(lv, li), 1, P.BUILD_SAH_INTERVALS)
    o.add_light(lo); s.add_light(ls)
    o.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0); s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    s.set_settings(P.Settings())
    a0, a1 = _render_pair(renderer, o, s, 64, 64, 4)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert a1[..., :3].sum() > 0


def test_material_update_without_reupload(renderer):
    v, i = standin_mesh(2)
    o, s = reference_layout_pair(v, i, 0)
    renderer.upload(s)
    new = P.Material(albedo=(0.9, 0.1, 0.1), specular=0.3)
    s.set_material(0, new); o.set_material(0, new.albedo, new.specular)
    renderer.update_materials(s)               # ref: Main.cpp:263-265 (edit + ResetAccumulator)
    renderer.reset_accumulator()
    renderer.render(48, 48, 2, seed=11)
    o.render(48, 48, 2, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 11, nthreads=2)
    assert np.array_equal(renderer.accumulator().view(np.uint32), o.accumulator().view(np.uint32))


def test_error_behaviour(renderer):
    fresh = P.Renderer(0)
    with pytest.raises(P.DeviceError) as e:
        fresh.scene = P.Scene()                 # bypass the Python-side assert: the library itself must refuse
        fresh.render(16, 16, 1)
    assert e.value.code == 3                    # CGPT_ERR_NO_SCENE
    bad = P.Scene(); bad.add_material(P.Material()); bad.add_sphere((0, 0, 0), 1.0, 5)
    with pytest.raises(P.DeviceError, match="mat_index"):
        fresh.upload(bad)
    v, i = standin_mesh(2)
    _, s = reference_layout_pair(v, i, 1)
    fresh.upload(s)
    with pytest.raises(P.DeviceError, match="rows"):
        fresh.render(16, 16, 1, rows=(8, 4))
    with pytest.raises(P.DeviceError, match="max_ray_depth"):
        fresh.render(16, 16, 1, settings=P.Settings(max_ray_depth=300))
    fresh.render(16, 16, 0)                     # zero samples: a no-op that still allocates the band
    assert not fresh.accumulator().any()
    fresh.close()


# ---- BASELINE.json's full size: size-independent properties ---------------------------------------------------------------

def test_full_size_properties(renderer):
    """1920x1080 on the 81 920-triangle stand-in: too large for the oracle in a test, so check invariants --
    w channel counts samples, determinism across runs, band tiling == full frame, counters add up, and a
    sample of 2 000 pixels' first-sample radiance equals the oracle's (per-pixel RNG streams are independent)."""
    W, H, spp = 1920, 1080, 2
    v, i = standin_mesh(6)
    o, s = reference_layout_pair(v, i, 3, aspect=W / H)
    renderer.upload(s)
    renderer.reset_accumulator(); renderer.reset_stats()
    renderer.render(W, H, spp, seed=0x12345678, counters=True)
    full = renderer.accumulator()
    st = renderer.stats()
    assert np.all(full[..., 3] == spp) and np.isfinite(full).all() and (full[..., :3] >= 0).all()
    assert st.traced_rays >= W * H * spp and st.bvh_depth_sum <= st.inner_steps and st.closest_hits <= st.traced_rays
    renderer.reset_accumulator()
    renderer.render(W, H, spp, seed=0x12345678)
    assert np.array_equal(renderer.accumulator().view(np.uint32), full.view(np.uint32))      # deterministic
    renderer.render(W, H, spp, seed=0x12345678, rows=(405, 540))                              # rank 3 of 8
    assert np.array_equal(renderer.accumulator().view(np.uint32), full[405:540].view(np.uint32))
    # oracle on three 16-row bands through the dragon stand-in
    for rows in ((300, 316), (536, 552), (900, 916)):
        o.reset_accumulator()
        o.render(W, H, spp, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 0x12345678, nthreads=8, rows=rows)
        want = o.accumulator()[rows[0]:rows[1]]
        assert rmse(want[..., :3] / spp, full[rows[0]:rows[1], :, :3] / spp) < RMSE_TOL


# ---- wavefront pipeline (extend / shade / connect queues) ---------------------------------------------------------------

@pytest.mark.parametrize("mat,exact", [(1, True), (4, True), (3, False)])
def test_wavefront_matches_oracle_and_megakernel(renderer, mat, exact):
    v, i = standin_mesh(3)
    o, s = reference_layout_pair(v, i, mat, extra_materials=(MAT_SPEC_DIFFUSE,))
    W, H, spp = 100, 72, 19          # > one batch of 16 samples, sizes not multiples of 8
    a0, a1 = _render_pair(renderer, o, s, W, H, spp, kernel=P.KERNEL_WAVEFRONT)
    sw = renderer.stats()
    so = o.stats()
    assert np.array_equal(a0[..., 3], a1[..., 3])
    assert rmse(a0[..., :3] / spp, a1[..., :3] / spp) < RMSE_TOL
    assert (so.traced_rays, so.inner_steps, so.tri_tests, so.bvh_depth_sum, so.closest_hits) == \
           (sw.traced_rays, sw.inner_steps, sw.tri_tests, sw.bvh_depth_sum, sw.closest_hits)
    if exact:
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
        assert np.array_equal(o.pixels(), renderer.pixels())
    px_w = renderer.pixels()
    renderer.reset_accumulator()
    renderer.render(W, H, spp, seed=0x12345678, kernel=P.KERNEL_MEGAKERNEL)
    assert np.array_equal(renderer.accumulator().view(np.uint32), a1.view(np.uint32))      # same bits on both GPU paths, glass included
    assert np.array_equal(renderer.pixels(), px_w)
    assert abs(so.total_energy_received - sw.total_energy_received) < 1e-6 * max(1.0, so.total_energy_received)


def test_wavefront_settings_debug_and_bands(renderer):
    v, i = standin_mesh(2)
    for settings in (P.Settings(next_event_estimation_enabled=False), P.Settings(max_ray_depth=0),
                     P.Settings(russian_roulette_enabled=False, cosine_weighted_diffuse_reflection_enabled=False, max_ray_depth=2)):
        o, s = reference_layout_pair(v, i, 4, extra_materials=(MAT_SPEC_DIFFUSE,), settings=settings)
        a0, a1 = _render_pair(renderer, o, s, 64, 40, 3, kernel=P.KERNEL_WAVEFRONT)
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
        assert o.stats().traced_rays == renderer.stats().traced_rays
    for debug in (P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH):
        st = P.Settings(debug_render_mode=debug)
        o, s = reference_layout_pair(v, i, 3, settings=st)
        o.render(64, 64, 1, O.MODE_ADVANCED, debug, O.RNG_PIXEL_PCG, 3, nthreads=2)
        renderer.upload(s); renderer.reset_accumulator()
        renderer.render(64, 64, 1, seed=3, kernel=P.KERNEL_WAVEFRONT)
        assert np.array_equal(renderer.pixels(), o.pixels())
    o, s = reference_layout_pair(v, i, 3, aspect=96 / 64)
    renderer.upload(s); renderer.reset_accumulator()
    renderer.render(96, 64, 3, seed=5, kernel=P.KERNEL_WAVEFRONT)
    full = renderer.accumulator()
    renderer.render(96, 64, 3, seed=5, rows=(20, 41), kernel=P.KERNEL_WAVEFRONT)
    assert np.array_equal(renderer.accumulator().view(np.uint32), full[20:41].view(np.uint32))


def test_wavefront_mesh_light_scene(renderer):
    v, i = standin_mesh(2)
    o = O.OracleScene(); s = P.Scene()
    mats = [P.Material(albedo=(0.7, 0.7, 0.7)), P.Material(emissive=(1, 1, 1), intensity=5.0, is_light=True),
            P.Material(albedo=(0.9, 0.9, 0.9), specular=0.8)]
    for m in mats:
        o.add_material(m.albedo, m.specular, m.refractivity, m.absorption, m.ior, m.emissive, m.intensity, m.is_light); s.add_material(m)
    lv = np.array([[-10, 20, 10, 0, -1, 0], [-10, 20, -10, 0, -1, 0], [10, 20, -10, 0, -1, 0], [10, 20, 10, 0, -1, 0]], np.float32)
    li = np.array([0, 1, 2, 2, 3, 0], np.uint32)
    o.add_mesh(v, i, 2, O.BUILD_SAH_PRIMITIVES); s.add_mesh(P.Mesh.from_arrays(v, i), 2, P.BUILD_SAH_PRIMITIVES)   # one 320-triangle leaf
    o.add_plane((0, 1, 0), (0, -3, 0), 0); s.add_plane((0, 1, 0), (0, -3, 0), 0)
    lo = o.add_mesh(lv, li, 1, O.BUILD_SAH_INTERVALS); ls = s.add_mesh(P.Mesh.from_arrays(lv, li), 1, P.BUILD_SAH_INTERVALS)
    o.add_light(lo); s.add_light(ls)
    o.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0); s.set_camera((0, 0, 8), (0, 0, -1), 60.0, 1.0)
    s.set_settings(P.Settings())
    a0, a1 = _render_pair(renderer, o, s, 48, 48, 4, kernel=P.KERNEL_WAVEFRONT)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    so, sw = o.stats(), renderer.stats()
    assert (so.traced_rays, so.inner_steps, so.tri_tests) == (sw.traced_rays, sw.inner_steps, sw.tri_tests)


# ---- multi-GPU tiling on one GPU: interleaved bands and the zero-copy device view used by the RCCL gather ------------------

@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_interleaved_bands_equal_full_image(renderer, kernel):
    from cpugpupathtracing_amd import distributed as D
    v, i = standin_mesh(3)
    _, s = reference_layout_pair(v, i, 3, aspect=100 / 77)
    W, H, spp = 100, 77, 3
    renderer.upload(s)
    renderer.reset_accumulator()
    renderer.render(W, H, spp, seed=5, kernel=kernel)
    full = renderer.accumulator()
    seen = np.zeros(H, bool)
    for world, h in ((3, 8), (8, 8), (2, 16)):
        for rank in range(world):
            rows = D.interleaved_rows(H, rank, world, h)
            if len(rows) == 0:
                continue
            renderer.render(W, H, spp, seed=5, kernel=kernel, interleave=(h, world, rank))
            band = renderer.accumulator()
            assert band.shape == (len(rows), W, 4)
            assert np.array_equal(band.view(np.uint32), full[rows].view(np.uint32))
            seen[rows] = True
    assert seen.all()
    with pytest.raises(P.DeviceError, match="interleave"):
        renderer.render(W, H, 1, interleave=(8, 2, 5))


def test_device_pointer_view_matches_host_copy(renderer):
    """FramebufferGather.gather wraps cgpt_accumulator_device_ptr as a torch tensor (CUDA array interface) with no copy."""
    import torch
    from cpugpupathtracing_amd.distributed import _DevicePointer
    v, i = standin_mesh(2)
    _, s = reference_layout_pair(v, i, 1)
    renderer.upload(s)
    renderer.reset_accumulator()
    renderer.render(64, 48, 2, seed=1)
    ptr, nbytes = renderer.accumulator_device_ptr()
    assert nbytes == 48 * 64 * 16
    t = torch.as_tensor(_DevicePointer(ptr, (48, 64, 4)), device="cuda:0")
    assert t.data_ptr() == ptr
    assert np.array_equal(t.cpu().numpy().view(np.uint32), renderer.accumulator().view(np.uint32))


# ---- brute-force integrator (TracePath) and the COMPARISON split screen (ref: Main.cpp:581-689, 719-729) ------------------

@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT, P.KERNEL_AUTO])
@pytest.mark.parametrize("mode,mat,exact", [(P.MODE_BRUTE_FORCE, 1, True), (P.MODE_BRUTE_FORCE, 4, True), (P.MODE_BRUTE_FORCE, 3, False),
                                            (P.MODE_COMPARISON, 4, True), (P.MODE_COMPARISON, 3, False)])
def test_brute_force_and_comparison_modes_match_oracle(renderer, mode, mat, exact, kernel):
    v, i = standin_mesh(3)
    st = P.Settings(render_mode=mode)
    o, s = reference_layout_pair(v, i, mat, extra_materials=(MAT_SPEC_DIFFUSE,), settings=st)
    W, H, spp = 80, 56, 5
    o.render(W, H, spp, mode, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 0x12345678, nthreads=8)
    renderer.upload(s)
    renderer.reset_accumulator(); renderer.reset_stats()
    renderer.render(W, H, spp, seed=0x12345678, counters=True, kernel=kernel)
    a0, a1 = o.accumulator(), renderer.accumulator()
    assert rmse(a0[..., :3] / spp, a1[..., :3] / spp) < RMSE_TOL
    so, sg = o.stats(), renderer.stats()
    assert (so.traced_rays, so.inner_steps, so.tri_tests, so.bvh_depth_sum, so.closest_hits) == \
           (sg.traced_rays, sg.inner_steps, sg.tri_tests, sg.bvh_depth_sum, sg.closest_hits)
    if exact:
        assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
        assert np.array_equal(o.pixels(), renderer.pixels())
    if mode == P.MODE_COMPARISON:        # the two halves really are different estimators
        assert not np.allclose(a1[:, : W // 2, :3].mean(), a1[:, W // 2:, :3].mean(), rtol=1e-3)


def test_brute_force_limits(renderer):
    v, i = standin_mesh(2)
    _, s = reference_layout_pair(v, i, 1)
    renderer.upload(s)
    with pytest.raises(P.DeviceError, match="max_ray_depth"):
        renderer.render(16, 16, 1, kernel=P.KERNEL_MEGAKERNEL, settings=P.Settings(render_mode=P.MODE_BRUTE_FORCE, max_ray_depth=40))
    renderer.render(16, 16, 1, kernel=P.KERNEL_MEGAKERNEL, settings=P.Settings(render_mode=P.MODE_BRUTE_FORCE, max_ray_depth=31))
    assert np.all(renderer.accumulator()[..., 3] == 1.0)
    # the persistent kernel keeps the levels in HBM: no depth limit short of the ABI's 254
    v2, i2 = standin_mesh(2)
    st = P.Settings(render_mode=P.MODE_BRUTE_FORCE, max_ray_depth=40)
    o, s2 = reference_layout_pair(v2, i2, 4, extra_materials=(MAT_SPEC_DIFFUSE,), settings=st)
    o.render(24, 16, 2, P.MODE_BRUTE_FORCE, O.DEBUG_NONE, O.RNG_PIXEL_PCG, 5, nthreads=2)
    renderer.upload(s2); renderer.reset_accumulator()
    renderer.render(24, 16, 2, seed=5, kernel=P.KERNEL_PERSISTENT)
    assert np.array_equal(renderer.accumulator().view(np.uint32), o.accumulator().view(np.uint32))
    # ... and so does the wavefront pipeline (per-path level records, pools sized for max_ray_depth + 1 of them)
    renderer.reset_accumulator()
    renderer.render(24, 16, 2, seed=5, kernel=P.KERNEL_WAVEFRONT)
    assert np.array_equal(renderer.accumulator().view(np.uint32), o.accumulator().view(np.uint32))
    renderer.reset_accumulator()
    renderer.render(24, 16, 2, seed=5, kernel=P.KERNEL_WAVEFRONT, settings=P.Settings(render_mode=P.MODE_ADVANCED, max_ray_depth=40))   # back to pools without levels


# ---- the C++ host path end to end: examples/render_main.cpp (the headless main loop) ------------------------------------

def test_cpp_example_main_loop(tmp_path):
    """Builds the C++ example against the library, runs it (scene set-up as Main.cpp:775-819 on the host mirror, 6 samples in
    previews of 4), and checks its dumps against the Python-driven renderer on the same scene."""
    import os, subprocess
    from cpugpupathtracing_amd import build as B, scene as S
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    mesh = P.Mesh.dragon_standin(3)
    gltf = str(tmp_path / "m.gltf")
    mesh.save_gltf(gltf)
    out = subprocess.run([exe, gltf, "96", "64", "6", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "Mrays/s" in out.stdout
    acc, n = S.read_accumulator(str(tmp_path / "render.acc"), 96, 64)
    assert n == 6 and os.path.exists(tmp_path / "preview_0004.ppm") and os.path.exists(tmp_path / "preview_0006.ppm")
    r = P.Renderer(0)
    r.upload(P.Scene.reference_layout(P.Mesh.load_gltf(gltf), 3, 96 / 64))
    r.render(96, 64, 6, seed=0x12345678)
    assert np.array_equal(r.accumulator().view(np.uint32), acc.view(np.uint32))
    ppm = (tmp_path / "render.ppm").read_bytes()
    body = np.frombuffer(ppm[-96 * 64 * 3:], np.uint8).reshape(64, 96, 3)
    assert np.array_equal(body[..., 0], r.pixels() & 0xFF)
    # the same loop on a multi-device context (examples/render_main.cpp --gpus 1 --collective: tiling + RCCL exchange + reorder with one
    # rank, which is what a one-GPU box can run): identical dumps
    first_ppm = (tmp_path / "render.ppm").read_bytes()
    out = subprocess.run([exe, "--gpus", "1", "--collective", gltf, "96", "64", "6", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    acc2, n2 = S.read_accumulator(str(tmp_path / "render.acc"), 96, 64)
    assert n2 == 6 and np.array_equal(acc2.view(np.uint32), acc.view(np.uint32))
    assert (tmp_path / "render.ppm").read_bytes() == first_ppm
    # scripted Update(dt): after 4 of 10 samples the camera moves (0.5 right, 0.25 up, 1 forward), the accumulator is reset and
    # the last 6 samples are rendered from the new position (ref: Main.cpp:277-297, 238-243)
    out = subprocess.run([exe, gltf, "96", "64", "10", "2", "4", "0.5", "0.25", "1.0"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    acc, n = S.read_accumulator(str(tmp_path / "render.acc"), 96, 64)
    assert n == 6
    sc = P.Scene.reference_layout(P.Mesh.load_gltf(gltf), 3, 96 / 64)
    sc.set_camera((0 - 0.5, 0 + 0.25, 8 - 1.0), (0, 0, -1), 60.0, 96 / 64)          # x -= right, y += up, z -= forward (Main.cpp:116-118)
    r.upload(sc)
    r.reset_accumulator()
    r.render(96, 64, 6, seed=0x12345678)
    assert np.array_equal(r.accumulator().view(np.uint32), acc.view(np.uint32))
    r.close()


# ---- edge cases of the scene description -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_scene_edge_cases(renderer, kernel):
    v, i = standin_mesh(2)
    grey, light, glass = P.Material(albedo=(0.6, 0.6, 0.6)), P.Material(emissive=(1, 1, 1), intensity=4.0, is_light=True), P.REFERENCE_MATERIALS[3]
    cases = {
        # no light list at all: NEE is skipped (ref: Main.cpp:439), emissive objects are still seen by chance
        "no_lights": _pair_from([("mesh", v, i, 0, O.BUILD_SAH_INTERVALS), ("sphere", (0, 12, 0), 4.0, 1)], [grey, light], []),
        # exactly one light: RandomUInt32Range draws nothing (ref: Random.h:43-44)
        "one_light": _pair_from([("mesh", v, i, 0, O.BUILD_SAH_INTERVALS), ("sphere", (6, 9, 4), 3.0, 1), ("plane", (0, 1, 0), (0, -3, 0), 0)], [grey, light], [1]),
        # analytic objects only, camera inside a glass sphere (sphere test from inside, SURVEY A-12)
        "primitives_only": _pair_from([("sphere", (0, 0, 8), 2.0, 2), ("sphere", (0, 9, 0), 3.0, 1), ("plane", (0, 1, 0), (0, -3, 0), 0)], [grey, light, glass], [1]),
        # nothing in view: every path misses
        "all_miss": _pair_from([("sphere", (0, 0, 100), 1.0, 0)], [grey], []),
        # depth-0 paths only and the longest brute-force-compatible depth
        "depth31": _pair_from([("mesh", v, i, 2, O.BUILD_NAIVE), ("plane", (0, 1, 0), (0, -3, 0), 0), ("sphere", (4, 9, 4), 3.0, 1)], [grey, light, glass], [2],
                              settings=P.Settings(max_ray_depth=31, russian_roulette_enabled=False)),
    }
    for name, (o, s) in cases.items():
        a0, a1 = _render_pair(renderer, o, s, 56, 40, 3, kernel=kernel)
        assert rmse(a0[..., :3] / 3, a1[..., :3] / 3) < RMSE_TOL, name
        so, sg = o.stats(), renderer.stats()
        assert (so.traced_rays, so.inner_steps, so.tri_tests, so.closest_hits) == (sg.traced_rays, sg.inner_steps, sg.tri_tests, sg.closest_hits), name
        if name in ("no_lights", "one_light", "all_miss"):
            assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32)), name
        if name == "all_miss":
            assert not a1[..., :3].any() and sg.traced_rays == 56 * 40 * 3


# ---- rarely taken paths of the trace kernel ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_traversal_stack_deeper_than_lds_part(renderer, kernel):
    """2^17 quads (2^18 triangles, tree depth >= 18): stacks outgrow the 16 LDS levels of the wavefront trace kernel and
    spill to HBM; the centre column of pixels has an axis-parallel direction (the NaN-exact slab path, SURVEY A-18)."""
    v, i = _quad_stack(1 << 17)
    glass, grey, light = P.REFERENCE_MATERIALS[3], P.Material(albedo=(0.6, 0.6, 0.6)), P.Material(emissive=(1, 1, 1), intensity=4.0, is_light=True)
    # fov 800: the reference's screen plane sits at distance fov-in-radians (SURVEY A-13), so this is a narrow view down the stack
    o, s = _pair_from([("mesh", v, i, 0, O.BUILD_SAH_INTERVALS), ("sphere", (0, 12, 4), 4.0, 2), ("plane", (0, 1, 0), (0, -3, 0), 1)],
                      [glass, grey, light], [1], camera=((0, 0, 8), (0, 0, -1), 800.0, 33 / 24))
    assert s.bvh_info(0).max_depth >= 17
    a0, a1 = _render_pair(renderer, o, s, 33, 24, 2, kernel=kernel)
    so, sg = o.stats(), renderer.stats()
    assert (so.traced_rays, so.inner_steps, so.tri_tests, so.closest_hits) == (sg.traced_rays, sg.inner_steps, sg.tri_tests, sg.closest_hits)
    assert sg.inner_steps > 20 * sg.traced_rays                   # the rays really walk the deep tree
    assert rmse(a0[..., :3] / 2, a1[..., :3] / 2) < RMSE_TOL


@pytest.mark.parametrize("kernel", [P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_more_objects_than_the_lds_object_table(renderer, kernel):
    """40 objects (small meshes, spheres, a plane, in mixed order): beyond the 31 object records the trace kernel mirrors in
    LDS, so its object step reads them from HBM and mesh-to-mesh transitions are not folded into the steps."""
    o, s = forty_object_pair()
    a0, a1 = _render_pair(renderer, o, s, 72, 48, 3, kernel=kernel)
    so, sg = o.stats(), renderer.stats()
    assert (so.traced_rays, so.inner_steps, so.tri_tests, so.closest_hits) == (sg.traced_rays, sg.inner_steps, sg.tri_tests, sg.closest_hits)
    assert np.array_equal(a0.view(np.uint32), a1.view(np.uint32))


@pytest.mark.parametrize("W,H,spp", [(1, 1, 3), (8, 8, 5), (7, 3, 2), (1000, 3, 4), (3, 700, 4), (257, 129, 9), (64, 64, 130), (33, 17, 300)])
def test_wavefront_equals_megakernel_on_odd_sizes(renderer, W, H, spp):
    """Degenerate and ragged frames, sample counts that do not divide into the batch size: the wavefront pipeline (edge-tile
    padding, block walk, batch sizing) gives the megakernel's accumulator bit for bit."""
    v, i = standin_mesh(2)
    _, s = reference_layout_pair(v, i, 3, aspect=W / H)
    renderer.upload(s)
    renderer.reset_accumulator(); renderer.reset_stats()
    renderer.render(W, H, spp, seed=5, kernel=P.KERNEL_MEGAKERNEL)
    a, rays = renderer.accumulator().copy(), renderer.stats().traced_rays
    renderer.reset_accumulator(); renderer.reset_stats()
    renderer.render(W, H, spp, seed=5, kernel=P.KERNEL_WAVEFRONT)
    assert np.array_equal(a.view(np.uint32), renderer.accumulator().view(np.uint32))
    assert renderer.stats().traced_rays == rays
    assert np.all(a[..., 3] == spp)


def test_wavefront_list_orders_give_the_same_image(renderer):
    """The order in which rays are traced never changes a path, so the image, the ray count and the traversal counters are identical
    for every order of the path ids (pixel-major by default; tile-major, sample-major), for misses dropped early or late in shade and
    for ray lists ordered by image band (default for batches of 32 Mi paths and more; forced on here), alone and with the other knobs.
    9 samples per call in batches of 5 and 4: the pixel-major accumulate stages 8 samples per pass (accumulate.hpp)"""
    v, i = standin_mesh(3)
    o, s = reference_layout_pair(v, i, 3, aspect=130 / 70)
    a = P.Renderer(0)
    a.upload(s)
    a.render(130, 70, 9, seed=3, kernel=P.KERNEL_WAVEFRONT, counters=True)
    want, st0 = a.accumulator().copy(), a.stats()
    a.close()
    for knobs in ({"path_order": 0, "retire_misses": 0, "batch": 5}, {"path_order": 1, "batch": 5}, {"path_order": 2, "batch": 9},
                  {"bands": 8, "bands_min_paths": 0, "batch": 4}, {"bands": 32, "bands_min_paths": 0, "path_order": 0, "batch": 5},
                  {"bands": 5, "bands_min_paths": 0, "retire_misses": 0, "pools": 1}):
        c = P.Renderer(0)
        c.upload(s)
        c.set_tuning(**knobs)
        c.render(130, 70, 9, seed=3, kernel=P.KERNEL_WAVEFRONT, counters=True)
        st2 = c.stats()
        assert np.array_equal(c.accumulator().view(np.uint32), want.view(np.uint32)), knobs
        assert (st0.traced_rays, st0.inner_steps, st0.tri_tests, st0.closest_hits) == (st2.traced_rays, st2.inner_steps, st2.tri_tests, st2.closest_hits)
        c.close()
