"""Round 0 of wf_shade ends the paths of a pixel whose primary ray left the scene before it forms their camera ray or seeds their
RNG (wavefront_kernels.hip: wf_shade, "Round 0 begins with the hit record"), and every part of a pass reads the kernel's arguments
where it uses them (shade_kernargs).  Neither may change a bit of any result.

One 70 x 36 frame -- neither side a multiple of the 8 x 8 tile, so padded lanes exist in both directions -- of the shipped scene
around the level-2 stand-in with one more light sphere in view: sky, ground, mesh and an emitter among the primary hits (asserted
below on the oracle's own primary rays).  Samples per call 5, 64 and 96: the batch is half the call, so a wave of 64 path ids holds
32 pixels (hit and miss lanes mixed), two pixels (whole waves of misses) or one pixel and a third of the next (a pixel straddles two
waves); 128 samples in batches of 64 make a wave exactly one pixel.

What is compared.  The wavefront pipeline against the megakernel and the persistent kernel: accumulator, pixels, traced_rays,
closest_hits, inner_steps and tri_tests bit for bit, always.  Against the oracle: the four counters and the sample counts bit for
bit, always; accumulator and pixels bit for bit where the frame has no glass (the mirror stand-in, the debug views, the all-miss
camera) -- with glass the device's expf in Beer's law differs from the host's by ULPs in every render path (DESIGN.md section 3:
RMSE 6e-10 at 64 x 64), so there every channel of every pixel is held to a relative bound worked out from those ULPs
(_against_oracle), the packed pixels to one code, and bit-identity is asserted against the two other device paths, whose code is
untouched.  The oracle has no resampled NEE: four candidates are compared across the
three device paths only."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from cpugpupathtracing_amd.distributed import interleaved_rows
from scenes import reference_layout_pair, rmse, standin_mesh

pytestmark = pytest.mark.gpu

W, H = 70, 36
SEED = 0x2468ACE1
GLASS, MIRROR = 3, 4
MAT_MIRROR = P.Material(albedo=(0.9, 0.9, 0.9), specular=1.0)
LIGHT_CENTRE, LIGHT_RADIUS = (-4.0, 2.0, 0.0), 0.9
CAMERA = ((0, 0, 8), (0, 0, -1), 60.0, W / H)
CAMERA_UP = ((0, 20, 8), (0, 1, 0), 60.0, W / H)          # from above the lights, straight up: nothing but sky
OTHERS = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT)
NO_HIT = 0xFFFFFFFF


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _counters(st):
    return (st.traced_rays, st.closest_hits, st.inner_steps, st.tri_tests)


def _pair(material=GLASS, camera=CAMERA):
    o, s = reference_layout_pair(*standin_mesh(2), material, aspect=W / H, extra_materials=(MAT_MIRROR,))
    li = o.add_sphere(LIGHT_CENTRE, LIGHT_RADIUS, 2)
    assert li == s.add_sphere(LIGHT_CENTRE, LIGHT_RADIUS, 2)
    o.add_light(li); s.add_light(li)
    o.set_camera(*camera); s.set_camera(*camera)
    return o, s, li


_PAIRS = {}


def _scene(material=GLASS, camera=CAMERA):
    key = (material, camera)
    if key not in _PAIRS:
        _PAIRS[key] = _pair(material, camera)
    return _PAIRS[key]


_ORACLE = {}


def _oracle(material, spp, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE, camera=CAMERA):
    """the oracle's frame, computed once per case and never changed"""
    key = (material, spp, mode, debug, camera)
    if key not in _ORACLE:
        o = _scene(material, camera)[0]
        o.reset_accumulator(); o.reset_stats()
        o.render(W, H, spp, mode, debug, O.RNG_PIXEL_PCG, SEED, nthreads=8)
        acc, px = o.accumulator().copy(), o.pixels().copy()
        acc.setflags(write=False); px.setflags(write=False)
        _ORACLE[key] = (acc, px, _counters(o.stats()))
    return _ORACLE[key]


def _render(s, kernel, spp, counters=True, settings=None, knobs=None, interleave=None, candidates=1):
    r = P.Renderer(0)
    try:
        if candidates != 1:
            r.set_nee_candidates(candidates)
        r.upload(s)
        if knobs:
            r.set_tuning(**knobs)
        r.reset_stats()
        r.render(W, H, spp, seed=SEED, kernel=kernel, counters=counters, settings=settings, interleave=interleave)
        st = r.stats()
        assert st.last_kernel == kernel
        return r.accumulator().copy(), r.pixels().copy(), _counters(st)
    finally:
        r.close()


def _same_on_all_device_paths(s, spp, **kw):
    """the wavefront frame, after it was found bit-identical to the megakernel's and the persistent kernel's"""
    knobs = kw.pop("knobs", None)
    got = _render(s, P.KERNEL_WAVEFRONT, spp, knobs=knobs, **kw)
    for k in OTHERS:
        acc, px, cnt = _render(s, k, spp, **kw)
        assert np.array_equal(_bits(got[0]), _bits(acc)), k
        assert np.array_equal(got[1], px), k
        assert got[2] == cnt, k
    return got


GLASS_ULPS = 72      # see _against_oracle


def _against_oracle(got, want, spp, exact):
    """exact: every bit.  Glass: the counters and the sample counts to the bit, and every channel of every pixel within
    (GLASS_ULPS + spp) * 2^-24 of its own size.  Where that comes from: the host's and the device's expf are each within 2 ULP of the true
    value, so a Beer factor differs by at most 4 ULP between them; it enters the throughput, and each of the about eight dependent
    multiplications and divisions of a bounce (albedo, Fresnel and lobe weights, the roulette division, the NEE product) rounds a
    differing input once more: 12 ULP per bounce, max_ray_depth + 1 = 6 bounces, 72 ULP (2^-24 each, relative) on every term of a
    path's radiance.  All terms are non-negative, so their sum carries the same relative error, and adding spp differing samples in
    the same order rounds at most spp times more.  A decision that flipped on such a difference would change the counters, which are
    asserted equal.  The packed 8-bit pixels may then differ by one code in a channel, and by no more."""
    acc, px, cnt = got
    assert cnt == want[2]
    assert np.array_equal(_bits(acc[..., 3]), _bits(want[0][..., 3]))
    if exact:
        assert np.array_equal(_bits(acc), _bits(want[0]))
        assert np.array_equal(px, want[1])
        return
    a, b = acc[..., :3].astype(np.float64), want[0][..., :3].astype(np.float64)
    rel = np.abs(a - b) / np.maximum(np.maximum(a, b), np.finfo(np.float32).tiny)
    code = max(int(np.abs(((px >> sh) & 0xFF).astype(np.int64) - ((want[1] >> sh) & 0xFF).astype(np.int64)).max()) for sh in (0, 8, 16))
    print(f"glass against the oracle at {spp} spp: largest relative difference {rel.max() * 2 ** 24:.2f} x 2^-24 "
          f"(bound {GLASS_ULPS + spp}), RMSE {rmse(a / spp, b / spp):.3e}, pixels differing {int((px != want[1]).sum())}, largest code step {code}")
    assert rel.max() <= (GLASS_ULPS + spp) * 2.0 ** -24
    assert code <= 1


def test_the_frame_has_sky_ground_mesh_and_a_visible_light():
    """on the oracle's own camera rays: the early-out, the hit lanes beside it and an emissive primary hit are all in the frame, and
    both an all-miss 8 x 8 tile (whole waves of misses at 64 samples per batch) and a tile of mixed lanes exist"""
    o, _, light = _scene()
    origins, dirs = o.camera_rays(W, H)
    _, obj, _, _ = o.intersect_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3))
    obj = obj.reshape(H, W)
    assert {0, 1, light, NO_HIT} <= set(np.unique(obj).tolist())
    miss = obj == NO_HIT
    tiles = [miss[y:y + 8, x:x + 8] for y in range(0, H, 8) for x in range(0, W, 8)]
    assert any(t.all() for t in tiles) and any(t.any() and not t.all() for t in tiles)
    assert 0.2 < miss.mean() < 0.8
    o_up = _scene(camera=CAMERA_UP)[0]
    origins, dirs = o_up.camera_rays(W, H)
    assert np.all(o_up.intersect_rays(origins.reshape(-1, 3), dirs.reshape(-1, 3))[1] == NO_HIT)


@pytest.mark.parametrize("spp", [5, 64, 96])
def test_samples_per_wave(spp):
    s = _scene()[1]
    got = _same_on_all_device_paths(s, spp)
    _against_oracle(got, _oracle(GLASS, spp), spp, exact=False)
    assert got[0][..., :3].any()


def test_one_pixel_per_wave():
    """128 samples in two batches of 64: the 64 lanes of every round-0 wave are one pixel, so a miss pixel is a whole wave leaving early"""
    s = _scene(MIRROR)[1]
    got = _render(s, P.KERNEL_WAVEFRONT, 128, knobs={"batch": 64})
    want = _render(s, P.KERNEL_MEGAKERNEL, 128)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def test_without_glass_the_oracle_is_met_to_the_bit():
    s = _scene(MIRROR)[1]
    _against_oracle(_same_on_all_device_paths(s, 5), _oracle(MIRROR, 5), 5, exact=True)


@pytest.mark.parametrize("debug", [P.DEBUG_NONE, P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views(debug):
    """the BVH-depth view colours the miss pixels too: the early-out must not take them (nor the ray-depth view's final depth)"""
    s = _scene()[1]
    st = P.Settings(debug_render_mode=debug)
    got = _same_on_all_device_paths(s, 5, settings=st)
    want = _oracle(GLASS, 5, debug=debug)
    if debug == P.DEBUG_NONE:
        _against_oracle(got, want, 5, exact=False)
    else:                                                        # the views bypass the accumulator (ref: Main.cpp:743-746): no glass radiance in them
        assert got[2] == want[2]
        assert np.array_equal(got[1], want[1])
        assert not got[0].any() and not want[0].any()


@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON])
@pytest.mark.parametrize("material,exact", [(GLASS, False), (MIRROR, True)])
def test_render_modes(mode, material, exact):
    """COMPARISON: TracePath lanes (left half) sit beside early-out lanes in the waves of the tiles the split runs through"""
    s = _scene(material)[1]
    got = _same_on_all_device_paths(s, 5, settings=P.Settings(render_mode=mode))
    _against_oracle(got, _oracle(material, 5, mode=mode), 5, exact=exact)


def test_counters_off():
    s = _scene()[1]
    on = _same_on_all_device_paths(s, 5, counters=True)
    off = _same_on_all_device_paths(s, 5, counters=False)
    assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(on[1], off[1])
    assert off[2][0] == on[2][0] == _oracle(GLASS, 5)[2][0]      # traced_rays is counted either way


@pytest.mark.parametrize("candidates", [1, 4])
def test_nee_candidates(candidates):
    s = _scene()[1]
    got = _same_on_all_device_paths(s, 5, candidates=candidates)
    one = _oracle(GLASS, 5)
    if candidates == 1:
        _against_oracle(got, one, 5, exact=False)
    else:
        assert not np.array_equal(_bits(got[0]), _bits(_render(s, P.KERNEL_WAVEFRONT, 5)[0]))   # four candidates really resample


@pytest.mark.parametrize("spp", [5, 64])
def test_camera_looking_straight_up(spp):
    """every path misses: zero radiance, the sample count where the project keeps it (the accumulator's w), one ray per path"""
    s = _scene(camera=CAMERA_UP)[1]
    got = _same_on_all_device_paths(s, spp)
    _against_oracle(got, _oracle(GLASS, spp, camera=CAMERA_UP), spp, exact=True)
    assert not got[0][..., :3].any() and np.all(got[0][..., 3] == spp)
    assert got[2][0] == W * H * spp and got[2][1] == 0


def test_interleaved_band():
    s = _scene()[1]
    full = _render(s, P.KERNEL_WAVEFRONT, 5)[0]
    band = _same_on_all_device_paths(s, 5, interleave=(4, 2, 1))[0]
    rows = interleaved_rows(H, 1, 2, 4)
    assert band.shape == (len(rows), W, 4)
    assert np.array_equal(_bits(band), _bits(full[rows]))


def test_one_context_renders_in_turn():
    """wavefront, megakernel, wavefront, persistent, wavefront on ONE context, frames of different content in between: the second and
    third wavefront renders meet held pools -- hit bytes, election-table epochs, st_en records that early-out lanes of the render before
    wrote or did not write -- and must give the first one's bits"""
    glass, sky = _scene()[1], _scene(camera=CAMERA_UP)[1]
    cam_up = sky.camera()
    r = P.Renderer(0)
    try:
        r.upload(glass)
        frames = []
        for kernel, camera, spp in ((P.KERNEL_WAVEFRONT, None, 5), (P.KERNEL_MEGAKERNEL, None, 5), (P.KERNEL_WAVEFRONT, cam_up, 5),
                                    (P.KERNEL_WAVEFRONT, None, 5), (P.KERNEL_PERSISTENT, None, 5), (P.KERNEL_WAVEFRONT, None, 3),
                                    (P.KERNEL_WAVEFRONT, None, 5)):
            r.reset_accumulator(); r.reset_stats()
            r.render(W, H, spp, seed=SEED, kernel=kernel, counters=True, camera=camera)
            frames.append((camera is None and spp == 5, r.accumulator().copy(), r.pixels().copy(), _counters(r.stats())))
            if camera is not None:
                assert not frames[-1][1][..., :3].any()
        same = [f for f in frames if f[0]]
        assert len(same) == 5
        for f in same[1:]:
            assert np.array_equal(_bits(f[1]), _bits(same[0][1])) and np.array_equal(f[2], same[0][2]) and f[3] == same[0][3]
    finally:
        r.close()
    _against_oracle(same[0][1:], _oracle(GLASS, 5), 5, exact=False)


@pytest.mark.parametrize("blocks", [1, 7])
def test_shade_blocks_per_cu(blocks):
    """the knob changes the shade grid, the number of output segments and the pools' sizes, never a result: plain lists and image bands,
    ADVANCED (election on) and COMPARISON (TracePath lanes)"""
    s = _scene()[1]
    for settings in (None, P.Settings(render_mode=P.MODE_COMPARISON)):
        want = _render(s, P.KERNEL_WAVEFRONT, 9, settings=settings)
        for knobs in ({"shade_blocks": blocks}, {"shade_blocks": blocks, "bands": 4, "bands_min_paths": 0, "batch": 4}):
            got = _render(s, P.KERNEL_WAVEFRONT, 9, settings=settings, knobs=knobs)
            assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2], knobs
