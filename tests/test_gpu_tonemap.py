"""The display stage on the device (cgpt_tonemap, cgpt_read_exposure, cgpt_exposure_reset; csrc/device/tonemap.hip)
against the host mirror, which tests/test_tonemap_reference.py holds to the numpy statement: the reading and, behind the linear transfer,
every output bit; behind sRGB the float64 model within the measured bound of tonemap_cases.SRGB_BOUND.

The shapes are the smallest that reach each way the kernels can go wrong: 1, 255, 256 and 257 pixels in a row (one block, a full one, one
lane into the second pass: a block strides over runs of 1 024 pixels); 300 x 217 (64 blocks, 3 to 4 passes each, a ragged tail); every
pixel in one bin (one LDS word takes every atomic); all 256 bins; the values that are not counted scattered through an image."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.tonemap import tonemap_params
import tonemap_ref as R
from scenes import reference_layout_pair, standin_mesh
from tonemap_cases import CURVE_NAMES, IMAGES, SEQUENCE, SEQUENCE_ALPHAS, SRGB_BOUND, SRGB_INPUTS

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 48, 32, 2, 0x12345678
AUTO = dict(key=0.25, ev_bias=1, exposure_scale=1.5, low_fraction=0.3, high_fraction=0.1, white=3.0)
MANUAL = dict(auto=False, ev_bias=-2, exposure_scale=0.75, white=4.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


@pytest.fixture(scope="module")
def ctx():
    r = P.Renderer(0)                                                          # the host source needs no scene
    yield r
    r.close()


@pytest.fixture(scope="module")
def scene():
    v, i = standin_mesh(1)
    _, s = reference_layout_pair(v, i, aspect=W / H)
    yield s
    s.close()


def rendered(scene, device=0, flags=0, **kw):
    r = P.Renderer(device, flags)
    r.upload(scene)
    r.render(W, H, SPP, seed=SEED, **kw)
    return r


def assert_equals_mirror(r, image, state=None, source="host", **kw):
    """one device call against the mirror's on `image`: outputs to the bit and, with auto exposure, the reading field by field"""
    auto = kw.get("auto", True)
    before = raw(r.exposure()) if not auto else None
    rgba, px = r.tonemap(source=source, image=image if source == "host" else None, **kw)
    want_rgba, want_px, want = P.tonemap_host(image, state, **kw)
    if auto:
        got = r.exposure()
        assert (got.valid, got.n_counted, got.n_ignored) == (want.valid, want.n_counted, want.n_ignored)
        assert np.array_equal(np.ctypeslib.as_array(got.histogram), np.ctypeslib.as_array(want.histogram))
        assert raw(got) == raw(want), (got.mean_index, want.mean_index, got.adapted_index, want.adapted_index, got.exposure, want.exposure)
    else:
        assert raw(r.exposure()) == before                                    # a manual call leaves the reading alone
    assert np.array_equal(bits(rgba), bits(want_rgba.reshape(rgba.shape)))
    assert np.array_equal(px, want_px.reshape(px.shape))
    return rgba, px


# ---- the reading and the linear outputs, to the bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_host_images_equal_the_mirror(ctx, name):
    image = IMAGES[name]
    for curve in CURVE_NAMES:
        ctx.exposure_reset()
        assert_equals_mirror(ctx, image, curve=curve, transfer="linear", **AUTO)
        assert_equals_mirror(ctx, image, curve=curve, transfer="linear", **MANUAL)
    ctx.exposure_reset()
    rgba, _ = ctx.tonemap(source="host", image=image, curve="clamp", transfer="linear", auto=False)
    # Vec4ToUint of the input, but for a NaN channel (255 there, 0 here)
    assert np.array_equal(ctx.tonemap(source="host", image=image, curve="clamp", transfer="linear", auto=False)[1],
                          R.pack_reference(np.where(np.isnan(image), np.float32(0.0), image)))
    assert (rgba[..., 3] == 1.0).all()


def test_either_output_alone(ctx):
    image = IMAGES["257"]
    p, keep = tonemap_params(source="host", image=image, transfer="linear", auto=False)
    rgba, px = ctx.tonemap(source="host", image=image, transfer="linear", auto=False)
    only_rgba = np.zeros_like(rgba); only_px = np.zeros_like(px)
    ctx._check(ctx.L.cgpt_tonemap(ctx._ctx, C.byref(p), only_rgba.ctypes.data_as(C.POINTER(C.c_float)), only_rgba.size, None, 0))
    ctx._check(ctx.L.cgpt_tonemap(ctx._ctx, C.byref(p), None, 0, only_px.ctypes.data_as(C.POINTER(C.c_uint32)), only_px.size))
    assert np.array_equal(bits(only_rgba), bits(rgba)) and np.array_equal(only_px, px)


# ---- 1. sRGB ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_srgb_follows_the_model(ctx, curve):
    bound = SRGB_BOUND[curve]
    for name in SRGB_INPUTS:
        image = IMAGES[name]
        for auto in (True, False):
            ctx.exposure_reset()
            rgba, px = ctx.tonemap(source="host", image=image, curve=curve, transfer="srgb", auto=auto)
            assert np.array_equal(px, R.pack(rgba[..., :3]))                  # Vec4ToUint of the call's own floats, exactly
            exposure = np.float32(ctx.exposure().exposure) if auto else np.float32(1.0)
            model = R.model(image, exposure, curve=curve, transfer="srgb")
            deviation = R.relative_deviation(rgba[..., :3], model)
            print(f"{curve} {name} auto={auto}: largest relative deviation from the model {deviation:.3e} (bound {bound:.3e})")
            assert deviation <= bound
            scaled = 255.0 * np.minimum(model, 1.0)
            want = np.floor(np.maximum(scaled, 0.0)).astype(np.int64)
            got = np.stack([(px >> s) & 0xFF for s in (0, 8, 16)], -1).astype(np.int64)
            differs = got != want
            assert (np.abs(got - want)[differs] == 1).all()
            assert (np.abs(scaled - np.rint(scaled))[differs] <= 255.0 * bound * np.abs(model[differs])).all()   # only at a code's edge: every pixel


# ---- 2. a sequence -----------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_adapts_as_the_mirror_does(ctx):
    ctx.exposure_reset()
    state = N.ExposureState()
    kw = dict(curve="reinhard", transfer="linear")
    assert_equals_mirror(ctx, SEQUENCE[0], state, alpha=SEQUENCE_ALPHAS[0], **kw)
    first = raw(ctx.exposure())
    with pytest.raises(P.DeviceError):                                         # a refused call between them changes nothing
        ctx.tonemap(source="host", image=SEQUENCE[1], alpha=1.5, **kw)
    assert_equals_mirror(ctx, SEQUENCE[2], None, auto=False, **kw)             # ... nor does a manual one
    assert raw(ctx.exposure()) == first
    assert_equals_mirror(ctx, SEQUENCE[1], state, alpha=SEQUENCE_ALPHAS[1], **kw)
    middle = ctx.exposure()
    assert middle.adapted_index not in (middle.mean_index, np.frombuffer(first, np.float64, 2)[1])   # half way
    assert_equals_mirror(ctx, SEQUENCE[2], state, alpha=SEQUENCE_ALPHAS[2], **kw)
    assert_equals_mirror(ctx, SEQUENCE[0], state, alpha=0.0, **kw)             # alpha 0 keeps the adaptation
    assert ctx.exposure().adapted_index != ctx.exposure().mean_index
    ctx.exposure_reset(); state.valid = 0
    assert_equals_mirror(ctx, SEQUENCE[3], state, alpha=SEQUENCE_ALPHAS[3], **kw)
    assert ctx.exposure().adapted_index == ctx.exposure().mean_index           # the reading after a reset sets it
    assert_equals_mirror(ctx, IMAGES["black"], state, alpha=1.0, **kw)         # no reading: kept
    assert ctx.exposure().valid == N.EXPOSURE_ADAPTED


# ---- 3. no state leaks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["300x217", "one_bin", "specials"])
def test_two_calls_in_a_row_give_the_same_bits(ctx, name):
    ctx.exposure_reset()
    a = ctx.tonemap(source="host", image=IMAGES[name], alpha=1.0); ia = raw(ctx.exposure())
    b = ctx.tonemap(source="host", image=IMAGES[name], alpha=1.0); ib = raw(ctx.exposure())
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    hist = lambda blob: blob[C.sizeof(N.ExposureInfo) - 1024:]
    assert hist(ia) == hist(ib) and np.frombuffer(ia, np.float64, 1)[0] == np.frombuffer(ib, np.float64, 1)[0]   # the table was cleared
    assert ia == ib                                                            # ... and m + (m - m) 1 is m


# ---- 4. sources -------------------------------------------------------------------------------------------------------------------------------------
def host_image_of(r):
    acc = r.accumulator()
    image = acc.copy()
    image[..., :3] = acc[..., :3] / np.float32(r.num_accumulated)             # pack_pixels_kernel's division
    return image


@pytest.mark.parametrize("band", [dict(), dict(rows=(5, 20)), dict(interleave=(4, 3, 1))], ids=["whole", "partial", "interleaved"])
def test_the_accumulator_equals_the_host_source(scene, ctx, band):
    r = rendered(scene, **band)
    image = host_image_of(r)
    for kw in (dict(curve="aces", transfer="linear", **AUTO), dict(curve="hable", transfer="linear", **MANUAL), dict()):
        r.exposure_reset(); ctx.exposure_reset()
        got = r.tonemap(source="accumulator", **kw)
        want = ctx.tonemap(source="host", image=image, **kw)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
        if kw.get("auto", True):
            assert raw(r.exposure()) == raw(ctx.exposure())
    assert np.array_equal(r.tonemap(curve="clamp", transfer="linear", auto=False)[1], r.pixels())   # the reference's bytes
    r.close()


def test_the_denoised_source_and_what_drops_it(scene, ctx):
    r = rendered(scene)
    calls = (lambda: r.denoise(iterations=2), lambda: r.denoise_temporal(iterations=1), lambda: r.denoise_variance_guided(iterations=2, temporal=True))
    for call in calls:
        rgba, _ = call()
        r.tonemap(source="accumulator")                                        # a call on another source in between
        for kw in (dict(curve="reinhard", transfer="linear", **AUTO), dict(curve="aces", transfer="linear", **MANUAL)):
            r.exposure_reset(); ctx.exposure_reset()
            got = r.tonemap(source="denoised", **kw)
            want = ctx.tonemap(source="host", image=rgba, **kw)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
    drops = (lambda: r.render(W, H, 1, seed=SEED), r.reset_accumulator, lambda: r.load_accumulator(np.ones((H, W, 4), np.float32), 1, W, H),
             lambda: r.render(W + 1, H, 1, seed=SEED))                         # ... and a framebuffer reallocation
    for drop in drops:
        if r.num_accumulated == 0:
            r.render(W, H, 1, seed=SEED)
        r.denoise(iterations=1)
        r.tonemap(source="denoised")
        drop()
        with pytest.raises(P.DeviceError) as e:
            r.tonemap(source="denoised")
        assert e.value.code == N.CGPT_ERR_INVALID
    r.close()


def test_a_call_changes_nothing_else(scene):
    r = rendered(scene)
    r.denoise_temporal(); r.reset_accumulator(); r.render(W, H, SPP, seed=SEED + 1)
    denoised, denoised_px = r.denoise_variance_guided(temporal=True)

    def snapshot():
        return dict(pixels=r.pixels().tobytes(), accumulator=r.accumulator().tobytes(), history=r.temporal_history().tobytes(), guides=r.guides().tobytes(),
                    variance=r.variance().tobytes(), stats=raw(r.stats()), num_accumulated=r.num_accumulated)

    before = snapshot()
    r.tonemap(source="accumulator"); r.tonemap(source="denoised", curve="hable"); r.tonemap(source="host", image=IMAGES["300x217"], auto=False)
    after = snapshot()
    assert [k for k in before if before[k] != after[k]] == []
    again = r.tonemap(source="denoised", curve="clamp", transfer="linear", auto=False)
    assert np.array_equal(again[1], denoised_px)                               # the filter's own bytes are still there
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(again[0][..., :3]), bits(np.where(denoised[..., :3] > 0, denoised[..., :3], np.float32(0.0))))
    r.close()


# ---- 5. multi-device, 6. streams ---------------------------------------------------------------------------------------------------------------------
def test_a_two_member_context_gives_the_one_device_bits(scene):
    one = rendered(scene)
    g = rendered(scene, [0, 0], P.CTX_GATHER_PEER_COPY)
    stats = raw(g.stats())
    for source in ("accumulator", "denoised", "host"):
        if source == "denoised":
            one.denoise(iterations=2); g.denoise(iterations=2)
        for kw in (dict(curve="aces", transfer="linear", **AUTO), dict(curve="reinhard", transfer="srgb", **MANUAL)):
            one.exposure_reset(); g.exposure_reset()
            image = IMAGES["300x217"] if source == "host" else None
            a, b = one.tonemap(source=source, image=image, **kw), g.tonemap(source=source, image=image, **kw)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
            if kw.get("auto", True):
                assert raw(one.exposure()) == raw(g.exposure())
    assert raw(g.stats()) == stats                                             # the gather was not counted
    one.close(); g.close()


def test_on_a_callers_stream(scene):
    import torch
    r = rendered(scene)
    image = IMAGES["300x217"]
    want = [r.tonemap(source="accumulator"), raw(r.exposure()), r.tonemap(source="host", image=image, curve="hable"), raw(r.exposure())]
    r.exposure_reset()
    side = torch.cuda.Stream()
    r.set_stream(side)
    try:
        got = [r.tonemap(source="accumulator"), raw(r.exposure()), r.tonemap(source="host", image=image, curve="hable"), raw(r.exposure())]
    finally:
        r.set_stream(None)
    for a, b in zip(got, want):
        assert a == b if isinstance(a, bytes) else (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]))
    r.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(source=3), dict(curve=4), dict(transfer=2), dict(flags=2), dict(flags=3), dict(exposure_scale=0.0), dict(exposure_scale=np.inf),
              dict(white=0.0), dict(white=np.nan), dict(key=0.0), dict(key=np.nan), dict(ev_bias=65), dict(ev_bias=-65), dict(low_fraction=-0.1),
              dict(low_fraction=1.0), dict(high_fraction=1.0), dict(low_fraction=0.5, high_fraction=0.5), dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=np.nan)]


def refused(r, code, **kw):
    with pytest.raises(P.DeviceError) as e:
        r.tonemap(**kw)
    assert e.value.code == code, e.value


def test_refusals_leave_the_reading_alone(scene):
    fresh = P.Renderer(0)
    with pytest.raises(P.DeviceError):
        fresh.exposure()                                                       # no auto-exposure call yet
    refused(fresh, N.CGPT_ERR_NO_SCENE, source="accumulator")
    refused(fresh, N.CGPT_ERR_NO_SCENE, source="denoised")
    fresh.upload(scene)
    refused(fresh, N.CGPT_ERR_INVALID, source="accumulator")                   # a scene, nothing rendered: as cgpt_read_pixels answers
    fresh.tonemap(source="host", image=IMAGES["255"], auto=False)
    with pytest.raises(P.DeviceError):
        fresh.exposure()                                                       # a manual call is no reading
    fresh.close()

    r = rendered(scene)
    image = IMAGES["257"]
    r.tonemap(source="host", image=image, alpha=1.0)
    r.tonemap(source="host", image=SEQUENCE[2], alpha=0.5)
    reading = raw(r.exposure())

    def unchanged():
        assert raw(r.exposure()) == reading
        r.tonemap(source="host", image=SEQUENCE[2], alpha=0.0)                 # m_adapted too: alpha 0 shows it
        assert raw(r.exposure()) == reading

    for bad in BAD_PARAMS:
        refused(r, N.CGPT_ERR_INVALID, **dict(dict(source="host", image=image), **bad))
    unchanged()
    refused(r, N.CGPT_ERR_INVALID, source="denoised")                          # no filter call yet
    p, keep = tonemap_params(source="host", image=image)
    rgba = np.zeros((1, 257, 4), np.float32); px = np.zeros((1, 257), np.uint32)
    fp, up = rgba.ctypes.data_as(C.POINTER(C.c_float)), px.ctypes.data_as(C.POINTER(C.c_uint32))
    L = r.L
    assert L.cgpt_tonemap(r._ctx, C.byref(p), None, 0, None, 0) == N.CGPT_ERR_INVALID
    assert L.cgpt_tonemap(r._ctx, C.byref(p), fp, rgba.size - 4, up, px.size) == N.CGPT_ERR_INVALID
    assert L.cgpt_tonemap(r._ctx, C.byref(p), fp, rgba.size, up, px.size + 1) == N.CGPT_ERR_INVALID
    assert L.cgpt_tonemap(r._ctx, None, fp, rgba.size, up, px.size) == N.CGPT_ERR_INVALID   # the defaults: the accumulator's 48 x 32 pixels
    for field, value in (("src_width", 0), ("src_height", 0)):
        q, _ = tonemap_params(source="host", image=image); setattr(q, field, value)
        assert L.cgpt_tonemap(r._ctx, C.byref(q), fp, rgba.size, up, px.size) == N.CGPT_ERR_INVALID
    q, _ = tonemap_params(source="host"); q.src_width, q.src_height = 257, 1   # a null image
    assert L.cgpt_tonemap(r._ctx, C.byref(q), fp, rgba.size, up, px.size) == N.CGPT_ERR_INVALID
    assert L.cgpt_read_exposure(r._ctx, None) == N.CGPT_ERR_INVALID
    assert not rgba.any() and not px.any()
    unchanged()
    r.reset_accumulator()
    refused(r, N.CGPT_ERR_INVALID, source="accumulator")                       # num_accumulated == 0
    st = P.Settings(); st.debug_render_mode = P.DEBUG_RAY_DEPTH
    r.render(W, H, 1, seed=SEED, settings=st)
    refused(r, N.CGPT_ERR_INVALID, source="accumulator")                       # a debug view
    unchanged()
    r.close()


def test_null_params_are_the_stated_defaults(scene):
    r = rendered(scene)
    rgba = np.zeros((H, W, 4), np.float32); px = np.zeros((H, W), np.uint32)
    r._check(r.L.cgpt_tonemap(r._ctx, None, rgba.ctypes.data_as(C.POINTER(C.c_float)), rgba.size, px.ctypes.data_as(C.POINTER(C.c_uint32)), px.size))
    info = raw(r.exposure())
    r.exposure_reset()
    want = r.tonemap(source="accumulator", curve="aces", transfer="srgb", auto=True, key=0.18, low_fraction=0.5, high_fraction=0.02, alpha=1.0, white=4.0,
                     exposure_scale=1.0, ev_bias=0)
    assert np.array_equal(bits(rgba), bits(want[0])) and np.array_equal(px, want[1]) and raw(r.exposure()) == info
    r.close()


# ---- the example ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_example_presents_through_the_stage(tmp_path):
    import subprocess
    from test_render_main_tonemap import build_example
    exe = build_example(tmp_path)

    def run(*options):
        d = tmp_path / ("run" + "".join(options).replace("-", "_"))
        d.mkdir()
        subprocess.run([exe, *options, "--denoise", "64", "48", "2"], cwd=d, check=True, capture_output=True, timeout=120)
        return (d / "render.ppm").read_bytes(), (d / "render_denoised.ppm").read_bytes()

    plain = run()
    assert run("--exposure", "0") == plain                                     # clamp, linear, exposure 1: Vec4ToUint, the run's own bytes
    d = tmp_path / "sequence"; d.mkdir()                                       # a sequence adapts frame to frame and writes every image
    subprocess.run([exe, "--tonemap", "hable", "--srgb", "--adapt", "0.5", "--temporal", "64", "48", "2"], cwd=d, check=True, capture_output=True, timeout=120)
    frames = sorted(d.glob("temporal_*_*.ppm"))
    assert len(frames) == 24 and all(len(f.read_bytes()) == len(plain[0]) for f in frames)
    assert (d / "temporal_00_raw.ppm").read_bytes() != plain[0]                # the same first frame (seed, camera, 2 spp), through the curve and sRGB


# ---- 8. memory -------------------------------------------------------------------------------------------------------------------------------------------
def test_device_memory_returns(scene):
    L = N.lib()
    start = L.cgpt_debug_live_device_bytes()
    r = rendered(scene)
    r.tonemap(source="accumulator"); r.denoise(iterations=1); r.tonemap(source="denoised", auto=False)
    r.tonemap(source="host", image=IMAGES["300x217"]); r.tonemap(source="host", image=IMAGES["257"])
    assert L.cgpt_debug_live_device_bytes() > start
    r.close()
    assert L.cgpt_debug_live_device_bytes() == start
