"""Later rounds of the wavefront pipeline trace one ray per (pixel, specular chain) and batch (wf_shade: "Specular chains"): a path
whose bounces since the primary hit were all mirror / dielectric has a ray fixed by its pixel and its choices, so one leader traces it
and the followers take its hit.  The knobs spec_dedupe / spec_keys must never change a result.  These cases compare the pipeline with
and without the election against the megakernel (bit-identical accumulator and pixels) and the oracle (traced rays equal; RMSE for the
image, since glass carries Beer's-law expf ULPs) for glass, a mirror and the C2 specular + diffuse material, a camera
inside a glass sphere (chains of total internal reflections), depths 1-8, entry tables small enough to overflow, several batch sizes,
every path order, image bands on and off, an interleaved multi-rank share, TracePath renders, the debug views and a table whose
epochs wrap between layouts of different sizes.  stats.chain_followers shows that the election ran where it should and nowhere else.
The counting kernels do not elect: their five counters stay the oracle's."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd.distributed import interleaved_rows
from scenes import MAT_SPEC_DIFFUSE, reference_layout_pair, rmse, standin_mesh

pytestmark = pytest.mark.gpu

W, H = 45, 37                  # not multiples of the 8x8 tile: the edge tiles are padded
SEED = 0x13572468
GLASS, MIRROR, SPEC_DIFFUSE = 3, 4, 5
MAT_MIRROR = P.Material(albedo=(0.9, 0.9, 0.9), specular=1.0)
EXTRA = (MAT_MIRROR, MAT_SPEC_DIFFUSE)
ON, OFF = {"spec_dedupe": 1}, {"spec_dedupe": 0}
BANDS_ON = {"bands": 4, "bands_min_paths": 0}   # image bands even for these small batches


def _counters(st):
    return (st.traced_rays, st.inner_steps, st.tri_tests, st.bvh_depth_sum, st.closest_hits)


def _pair(material=GLASS, depth=5, glass_camera=False):
    o, s = reference_layout_pair(*standin_mesh(2), material, aspect=W / H, extra_materials=EXTRA,
                                 settings=P.Settings(max_ray_depth=depth))
    if glass_camera:   # off to the side of the camera: rays looking ahead reflect totally at its wall, rays to the left leave it
        assert o.add_sphere((1.6, 0.0, 8.0), 2.0, GLASS) == s.add_sphere((1.6, 0.0, 8.0), 2.0, GLASS)
    return o, s


def _oracle(o, spp, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE):
    o.reset_accumulator(); o.reset_stats()
    o.render(W, H, spp, mode, debug, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    return o.accumulator().copy(), o.pixels().copy(), _counters(o.stats())


def _render(s, kernel, spp, knobs=None, counters=False, settings=None, interleave=None):
    r = P.Renderer(0)
    try:
        r.upload(s)
        if knobs:
            r.set_tuning(**knobs)
        r.reset_stats()
        r.render(W, H, spp, seed=SEED, kernel=kernel, counters=counters, settings=settings, interleave=interleave)
        return r.accumulator().copy(), r.pixels().copy(), r.stats()
    finally:
        r.close()


def _check(s, o_run, spp, knobs, settings=None, interleave=None, elects=True):
    """wavefront with `knobs`, spec_dedupe on and off: bit-identical to the megakernel, traced rays = the oracle's; followers only with
    the election on, and some of them when `elects`"""
    ref_acc, ref_px, _ = _render(s, P.KERNEL_MEGAKERNEL, spp, settings=settings, interleave=interleave)
    for dedupe in (ON, OFF):
        acc, px, st = _render(s, P.KERNEL_WAVEFRONT, spp, {**knobs, **dedupe}, settings=settings, interleave=interleave)
        assert st.last_kernel == P.KERNEL_WAVEFRONT
        assert np.array_equal(acc.view(np.uint32), ref_acc.view(np.uint32)), dedupe
        assert np.array_equal(px, ref_px), dedupe
        assert (st.chain_followers > 0) == (elects and dedupe is ON), (dedupe, st.chain_followers)
        if o_run is not None:
            want, _, want_counters = o_run
            assert st.traced_rays == want_counters[0], dedupe
            assert np.array_equal(acc[..., 3], want[..., 3])
            assert rmse(acc[..., :3] / spp, want[..., :3] / spp) < 1e-4
    return acc, st


@pytest.mark.parametrize("material", [GLASS, MIRROR, SPEC_DIFFUSE])
def test_materials_match_megakernel_and_oracle(material):
    o, s = _pair(material)
    _check(s, _oracle(o, 64), 64, {"batch": 32})


@pytest.mark.parametrize("path_order", [0, 1, 2])
@pytest.mark.parametrize("batch,spp", [(1, 7), (3, 7), (64, 128)])
def test_camera_inside_glass(path_order, batch, spp):
    o, s = _pair(glass_camera=True)
    _check(s, _oracle(o, spp), spp, {"batch": batch, "path_order": path_order}, elects=batch > 1)   # one sample per batch: nothing to share


@pytest.mark.parametrize("depth", range(1, 9))
def test_max_depth(depth):
    o, s = _pair(depth=depth, glass_camera=True)
    _check(s, _oracle(o, 32), 32, {"batch": 16})


@pytest.mark.parametrize("keys", [1, 2, 16])
@pytest.mark.parametrize("bands", [BANDS_ON, {"bands": 1}])
def test_entry_overflow_and_bands(keys, bands):
    """spec_keys 1 and 2: most pixels of the glass-sphere view run out of entries after a few bounces, and those rays are traced as usual"""
    o, s = _pair(depth=8, glass_camera=True)
    _check(s, _oracle(o, 64), 64, {"batch": 64, "spec_keys": keys, **bands})


def test_interleaved_rank_share():
    """Bands of 3 rows dealt over 3 ranks (every rank's band 13 rows high: padded tiles on both edges): each rank matches the
    megakernel bit for bit and the ranks' traced rays add up to the oracle's full frame"""
    o, s = _pair(glass_camera=True)
    spp, world, band_rows = 32, 3, 3
    want, _, want_counters = _oracle(o, spp)
    rays, full = 0, np.zeros_like(want)
    for rank in range(world):
        il = (band_rows, world, rank)
        acc, st = _check(s, None, spp, {"batch": 16, **BANDS_ON}, interleave=il)
        rays += st.traced_rays
        full[interleaved_rows(H, rank, world, band_rows)] = acc
    assert rays == want_counters[0]
    assert rmse(full[..., :3] / spp, want[..., :3] / spp) < 1e-4


@pytest.mark.parametrize("mode", [P.MODE_COMPARISON, P.MODE_BRUTE_FORCE])
def test_tracepath_renders(mode):
    _, s = _pair(glass_camera=True)
    _check(s, None, 16, {"batch": 8}, settings=P.Settings(render_mode=mode), elects=False)   # the TracePath instantiation does not elect


@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views(debug):
    """the debug views keep every extend ray's hit record (no retired misses): followers read their leader's"""
    _, s = _pair(glass_camera=True)
    _check(s, None, 4, {"batch": 2}, settings=P.Settings(debug_render_mode=debug), elects=debug == P.DEBUG_RAY_DEPTH)   # BVH view: round 0 only


def test_counting_kernels_keep_the_oracle_counters():
    o, s = _pair(glass_camera=True)
    want, _, want_counters = _oracle(o, 64)
    acc, _, st = _render(s, P.KERNEL_WAVEFRONT, 64, {"batch": 32, **ON}, counters=True)
    assert _counters(st) == want_counters
    assert st.chain_followers == 0
    assert rmse(acc[..., :3] / 64, want[..., :3] / 64) < 1e-4


def test_epoch_wrap_after_a_smaller_layout():
    """A pool's table outlives a call.  With spec_epochs 12 and one batch of 6 shade launches per pool and call: two large calls
    (spec_keys 16) take epochs 1-6 and 7-12, a small call (spec_keys 8) wraps and takes 1-6, and a large call with another seed takes
    7-12 again, round for round with the second call's tags on other paths.  The wrap must have cleared the whole table, not the small
    layout's part of it."""
    _, s = _pair(glass_camera=True)
    calls = [((W, H), 16, SEED), ((W, H), 16, SEED), ((16, 16), 8, SEED), ((W, H), 16, SEED ^ 0x5A5A5A5A)]
    r, ref = P.Renderer(0), P.Renderer(0)
    try:
        r.upload(s); ref.upload(s)
        r.set_tuning(batch=8, pools=2, spec_epochs=12, **ON)
        for (w, h), keys, seed in calls:
            r.set_tuning(spec_keys=keys)
            r.reset_stats()
            r.render(w, h, 16, seed=seed, kernel=P.KERNEL_WAVEFRONT)
            ref.render(w, h, 16, seed=seed, kernel=P.KERNEL_MEGAKERNEL)
            assert np.array_equal(r.accumulator().view(np.uint32), ref.accumulator().view(np.uint32)), ((w, h), keys, seed)
            assert r.stats().chain_followers > 0
    finally:
        r.close(); ref.close()
