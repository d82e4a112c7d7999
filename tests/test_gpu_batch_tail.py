"""The tail of a batch in the wavefront pipeline: shade work items sized to the list (csrc/device/shade_items.h) and sky pixels that
neither store nor load their zero records (accumulate.hpp: pixel_adds_nothing).  Neither may change a bit of any result.

The frame is that of test_gpu_shade_prologue.py -- 70 x 36, sky, ground, mesh and a visible emitter among the primary hits, padded
lanes in both directions -- and so are its references: the oracle's frames are computed once there and shared.

What is compared, in every case: the wavefront pipeline's accumulator, pixels and the four counters against the megakernel's and the
persistent kernel's, bit for bit; against the oracle the counters and the sample counts bit for bit, and accumulator and pixels bit for
bit wherever the frame has no glass (the mirror stand-in, the debug views, the all-sky camera).  With glass the device's expf differs from
the host's by ULPs in every render path, so there the oracle is met within the bound test_gpu_shade_prologue.py works
out from those ULPs (_against_oracle); the item-length cases therefore run on the mirror stand-in, where the oracle is met to the bit,
and once on the glass.

Item length.  An item is never shorter than four blocks (shade_items.h), so a chunk of 1, 3 or 4 must behave exactly as the knob says and
32 is the one that shrinks.  shade_blocks = 1 makes 1 024 shade waves.  64 samples are two batches of 32: 1 440 blocks of 64 paths in
round 0 each (more than n_waves x chunk at chunk 1, fewer at 3, 4 and 32: items of 4 at 32) and later lists shorter than one block per
wave; 5 samples are batches of 2 and 3: 90 and 135 blocks, fewer than waves.  With the default grid (5 120 waves) every list of this
frame is shorter than the grid."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
import test_gpu_shade_prologue as base

pytestmark = pytest.mark.gpu

W, H, SEED = base.W, base.H, base.SEED
GLASS, MIRROR = base.GLASS, base.MIRROR
_bits = base._bits

_DEVICE = {}


def _others(material, spp, camera=base.CAMERA, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE, counters=True, interleave=None):
    """the megakernel's frame, found bit-identical to the persistent kernel's; computed once per case, never changed"""
    key = (material, spp, camera, mode, debug, counters, interleave)
    if key not in _DEVICE:
        s = base._scene(material, camera)[1]
        st = P.Settings(render_mode=mode, debug_render_mode=debug)
        a = base._render(s, P.KERNEL_MEGAKERNEL, spp, counters=counters, settings=st, interleave=interleave)
        b = base._render(s, P.KERNEL_PERSISTENT, spp, counters=counters, settings=st, interleave=interleave)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        a[0].setflags(write=False); a[1].setflags(write=False)
        _DEVICE[key] = a
    return _DEVICE[key]


def _check(material, spp, knobs=None, camera=base.CAMERA, mode=P.MODE_ADVANCED, debug=P.DEBUG_NONE, counters=True, exact=None):
    s = base._scene(material, camera)[1]
    st = P.Settings(render_mode=mode, debug_render_mode=debug)
    got = base._render(s, P.KERNEL_WAVEFRONT, spp, counters=counters, settings=st, knobs=knobs)
    want = _others(material, spp, camera, mode, debug, counters)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), knobs
    assert np.array_equal(got[1], want[1]), knobs
    assert got[2] == want[2], knobs
    if counters:
        ref = base._oracle(material, spp, mode=mode, debug=debug, camera=camera)
        if debug != P.DEBUG_NONE:                                # the views bypass the accumulator (ref: Main.cpp:743-746)
            assert got[2] == ref[2] and np.array_equal(got[1], ref[1]) and not got[0].any() and not ref[0].any()
        else:
            base._against_oracle(got, ref, spp, exact=material == MIRROR if exact is None else exact)
    return got


# ---- work items sized to the list ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [1, 3, 4, 32])
@pytest.mark.parametrize("bands", [0, 1, 32])
def test_item_length(chunk, bands):
    """bands 0: plain lists by the default threshold; 1 and 32: the threshold lowered to nothing, one band (plain lists again, through the
    banded chunk's choice) and 32 image bands"""
    knobs = {"shade_blocks": 1, "shade_chunk": chunk, "shade_chunk_banded": chunk}
    if bands:
        knobs.update(bands=bands, bands_min_paths=0)
    _check(MIRROR, 64, knobs)


@pytest.mark.parametrize("knobs", [
    {"shade_blocks": 1, "shade_chunk": 32, "shade_chunk_banded": 32, "bands": 32, "bands_min_paths": 0},
    {"shade_blocks": 1, "shade_chunk": 1},
    {},
], ids=["banded-32", "chunk-1", "default"])
def test_item_length_with_glass(knobs):
    _check(GLASS, 64, knobs)


@pytest.mark.parametrize("knobs", [{}, {"shade_chunk": 32}, {"shade_blocks": 1, "shade_chunk": 3}, {"shade_chunk_banded": 4, "bands": 32, "bands_min_paths": 0}],
                         ids=["default", "chunk-32", "one-block-chunk-3", "banded-4"])
def test_fewer_blocks_than_waves(knobs):
    _check(MIRROR, 5, knobs)


def test_item_length_with_trace_path_lanes():
    """COMPARISON: the TracePath kernels' grid and the counting instantiation walk the same items"""
    for knobs in ({"shade_blocks": 1, "shade_chunk": 4}, {"shade_blocks": 1, "shade_chunk_banded": 32, "bands": 4, "bands_min_paths": 0}):
        _check(MIRROR, 9, knobs, mode=P.MODE_COMPARISON)


# ---- sky pixels ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spp", [5, 64, 96])
def test_samples_per_wave(spp):
    """a wave of 64 path ids holds 32 pixels, two pixels or a pixel and a third of the next; the accumulate stage takes 2, 8 and 8 samples a pass"""
    got = _check(GLASS, spp)
    assert got[0][..., :3].any()


@pytest.mark.parametrize("spp", [5, 64])
def test_all_sky(spp):
    got = _check(GLASS, spp, camera=base.CAMERA_UP, exact=True)
    assert not got[0][..., :3].any() and np.all(got[0][..., 3] == spp)
    assert got[2][0] == W * H * spp and got[2][1] == 0


@pytest.mark.parametrize("path_order", [0, 1, 2])
def test_path_orders(path_order):
    """sample-major and tile-major ids read st_en per sample instead of through the stage"""
    _check(MIRROR, 9, {"path_order": path_order})


@pytest.mark.parametrize("debug", [P.DEBUG_RAY_DEPTH, P.DEBUG_BVH_DEPTH])
def test_debug_views_store_and_load(debug):
    """the predicate is false: the ray-depth view reads the stored depth of a miss, the BVH-depth view colours it"""
    _check(GLASS, 5, debug=debug)


@pytest.mark.parametrize("mode", [P.MODE_ADVANCED, P.MODE_BRUTE_FORCE, P.MODE_COMPARISON])
def test_render_modes(mode):
    """TracePath pixels (all of them, or the left half) are never skipped; in COMPARISON both kinds sit in one wave of the tiles the split runs through"""
    _check(MIRROR, 5, mode=mode)
    _check(GLASS, 5, mode=mode)


def test_counters_off():
    on = _check(GLASS, 5)
    off = _check(GLASS, 5, counters=False)
    assert np.array_equal(_bits(on[0]), _bits(off[0])) and np.array_equal(on[1], off[1])


def test_interleaved_band():
    s = base._scene(MIRROR)[1]
    il = (4, 2, 1)
    got = base._render(s, P.KERNEL_WAVEFRONT, 5, interleave=il)
    want = _others(MIRROR, 5, interleave=il)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    rows = base.interleaved_rows(H, 1, 2, 4)
    full = base._oracle(MIRROR, 5)
    assert np.array_equal(_bits(got[0]), _bits(full[0][rows])) and np.array_equal(got[1], full[1][rows])


def _sequence(kernel, steps, knobs=None):
    """renders into ONE accumulator on one context, no reset between them: (camera or None, samples) per step"""
    glass = base._scene()[1]
    r = P.Renderer(0)
    try:
        r.upload(glass)
        if knobs:
            r.set_tuning(**knobs)
        r.reset_stats()
        for camera, spp in steps:
            r.render(W, H, spp, seed=SEED, kernel=kernel, counters=True, camera=camera)
        return r.accumulator().copy(), r.pixels().copy(), base._counters(r.stats())
    finally:
        r.close()


def test_two_renders_into_one_accumulator():
    """The second and third render meet a non-zero accumulator and, on the pixels that are sky for them, st_en records the render before left
    there: 5 samples of the frame, 5 looking straight up (every pixel sky, over records of hit pixels), 3 of the frame again."""
    up = base._scene(camera=base.CAMERA_UP)[1].camera()
    steps = ((None, 5), (up, 5), (None, 3))
    got = _sequence(P.KERNEL_WAVEFRONT, steps)
    for k in base.OTHERS:
        acc, px, cnt = _sequence(k, steps)
        assert np.array_equal(_bits(got[0]), _bits(acc)) and np.array_equal(got[1], px) and got[2] == cnt, k
    o = base._pair()[0]                                          # an oracle of its own: its camera moves
    o.reset_accumulator(); o.reset_stats()
    o.render(W, H, 5, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    o.set_camera(*base.CAMERA_UP)
    o.render(W, H, 5, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    o.set_camera(*base.CAMERA)
    o.render(W, H, 3, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    base._against_oracle(got, (o.accumulator().copy(), o.pixels().copy(), base._counters(o.stats())), 13, exact=False)
    assert np.all(got[0][..., 3] == 13)


def test_one_pool_serves_three_batches():
    """1 024 samples in batches of 128 on two pools: every pool is reused by a third and a fourth batch, whose sky pixels find the records
    (and whose hit pixels the px_hit) of the batches before"""
    knobs = {"max_batch": 128, "pools": 2}
    s = base._scene()[1]
    got = base._render(s, P.KERNEL_WAVEFRONT, 1024, knobs=knobs)
    for k in base.OTHERS:
        acc, px, cnt = base._render(s, k, 1024)
        assert np.array_equal(_bits(got[0]), _bits(acc)) and np.array_equal(got[1], px) and got[2] == cnt, k
    base._against_oracle(got, base._oracle(GLASS, 1024), 1024, exact=False)


def test_wavefront_in_turn_with_the_persistent_kernel():
    """one context: the persistent kernel shares accumulate_batch (it reads every record) and the context's accumulator"""
    glass = base._scene()[1]
    up = base._scene(camera=base.CAMERA_UP)[1].camera()
    r = P.Renderer(0)
    try:
        r.upload(glass)
        frames = []
        for kernel, camera, spp in ((P.KERNEL_WAVEFRONT, None, 5), (P.KERNEL_PERSISTENT, None, 5), (P.KERNEL_WAVEFRONT, up, 64),
                                    (P.KERNEL_WAVEFRONT, None, 5), (P.KERNEL_PERSISTENT, up, 5), (P.KERNEL_WAVEFRONT, None, 5)):
            r.reset_accumulator(); r.reset_stats()
            r.render(W, H, spp, seed=SEED, kernel=kernel, counters=True, camera=camera)
            frame = (r.accumulator().copy(), r.pixels().copy(), base._counters(r.stats()))
            if camera is None:
                frames.append(frame)
            else:
                assert not frame[0][..., :3].any() and np.all(frame[0][..., 3] == spp)
    finally:
        r.close()
    want = _others(GLASS, 5)
    for f in frames:
        assert np.array_equal(_bits(f[0]), _bits(want[0])) and np.array_equal(f[1], want[1]) and f[2] == want[2]
