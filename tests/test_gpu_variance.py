"""The variance-guided filter on the device (cgpt_denoise_variance_guided, cgpt_read_variance; csrc/device/denoise.hip)
against its numpy statement (variance_ref.py): the variance map and the output without and with the temporal stage, the colour history
against cgpt_denoise_temporal's, what drops the moments, invariance over render paths and device groups, no side effects, refusals, the
quality it buys, and the example.

Tolerance: a float32 run of the statement is at most 2.06e-5 (in units of max(1, |ref|); variance map 2.06e-5, stored colour 1.53e-5,
output 1.03e-5) from the float64 one on these scenes, sizes and frames (test_variance_reference.py measures it and holds it under
variance_cases.DEV32 = 2.5e-5).  The device is held to max(1e-4, 4 x 2.5e-5) max(1, |ref|) = 1e-4 max(1, |ref|): the factor 4 allows for
__expf and another summation order, 1e-4 is the floor the temporal tests use.  The float32 run decides no pixel's var_t / var_s choice or
tap set differently from the float64 one on these frames, so at most 0.5 % of a frame may be left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from scenes import reference_layout_pair, standin_mesh
from test_gpu_denoise import BIG, KERNELS, TRI, all_kinds_pair, channels, light_materials, stats_bytes
from test_gpu_temporal import cameras, new_renderer, orbit_camera, render_frame
import denoise_ref as D
import temporal_cases as TC
import variance_ref as V
import variance_cases as VC

pytestmark = pytest.mark.gpu

W, H = VC.W, VC.H
SEED = VC.SEED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_close(got, ref, what, keep=None):
    err = VC.rel_err(got, ref)
    if keep is not None:
        err = np.where(keep.reshape(keep.shape + (1,) * (err.ndim - keep.ndim)), err, 0.0)
    print(f"{what}: largest error {float(err.max()):.3e} of {VC.TOL:.1e}")
    assert np.all(err <= VC.TOL), f"{what}: {float(err.max()):.3e} at {np.unravel_index(np.argmax(err), err.shape)}"


def assert_pixels_close(px, rgb):
    assert np.max(np.abs(channels(px)[..., :3] - channels(D.pack_pixels(rgb))[..., :3])) <= 1


@pytest.fixture(scope="module")
def pairs():
    return {which: TC.scene_pair(which) for which in TC.SCENES}


# ---- 1. one frame against the statement -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,spp", [((W, H), 3), (VC.SMALL, 1), (VC.SMALL, 4)])
@pytest.mark.parametrize("which", TC.SCENES)
def test_variance_map_and_output_match_the_reference_statement(which, size, spp):
    w, h = size
    _, s = TC.scene_pair(which) if size == (W, H) else (reference_layout_pair(*standin_mesh(2), 3, aspect=w / h) if which == "reference"
                                                        else all_kinds_pair(w / h))
    lights = light_materials(s)
    r = new_renderer(s)
    try:
        r.render(w, h, spp, seed=SEED)
        acc, g = r.accumulator(), r.guides()
        for it in (0, 1, 3, 5):
            for demod in (False, True):
                for sigmas in ((4.0, 0.2, 0.3),) + (((1.5, 0.5, 2.0),) if it == 3 else ()):
                    rgba, px = r.denoise_variance_guided(it, *sigmas, demodulate=demod)
                    var = r.variance()
                    ref_rgba, ref_px, ref_var = V.variance_guided(acc, spp, g, iterations=it, sigma_luminance=sigmas[0], sigma_normal=sigmas[1],
                                                                  sigma_position=sigmas[2], demodulate=demod, light_materials=lights)
                    what = f"{which} {w}x{h} {spp} spp, {it} iterations, demodulate {demod}, sigmas {sigmas}"
                    assert_close(var, ref_var, what + ": variance")
                    assert_close(rgba, ref_rgba, what + ": output")
                    assert_pixels_close(px, ref_rgba[..., :3])
                    assert np.all(rgba[..., 3] == 1.0) and np.all(var >= 0)
                    if it == 0:                                                # cgpt_denoise's identity, bit for bit
                        plain = r.denoise(iterations=0, demodulate=demod)
                        assert np.array_equal(bits(rgba), bits(plain[0])) and np.array_equal(px, plain[1]) and np.array_equal(px, r.pixels())
        assert ref_var.max() > 1e-3                                           # there is noise to measure
    finally:
        r.close()


def test_a_contiguous_band_is_filtered_on_its_own(pairs):
    _, s = pairs["all_kinds"]
    rows = (10, 37)
    r = new_renderer(s)
    try:
        r.render(W, H, 2, seed=SEED, rows=rows)
        acc, g = r.accumulator(), r.guides()
        assert g.shape == (27, W, 12)
        rgba, px = r.denoise_variance_guided()
        ref_rgba, _, ref_var = V.variance_guided(acc, 2, g, light_materials=light_materials(s))
        assert r.variance().shape == (27, W)
        assert_close(r.variance(), ref_var, "band: variance")
        assert_close(rgba, ref_rgba, "band: output")
    finally:
        r.close()


# ---- 2. the temporal sequence -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mhf", VC.MIN_HISTORY)
@pytest.mark.parametrize("which", TC.SCENES)
def test_temporal_sequence_matches_the_reference_statement(pairs, which, mhf):
    """Six frames, static and then moving, each one step of the statement from the device's own colour history (the moments are the
    statement's own: the ABI does not return them): the stored colour and the variance map against the statement, the output against
    the statement's passes on the device's own colour and variance.  A second context driven by cgpt_denoise_temporal on the same
    frames stores the same bytes.  Left out: the pixels a float32 run of the statement decides differently and those whose history
    comes through one -- at most that count plus 0.5 % of the frame."""
    _, s = pairs[which]
    cams = cameras(s)
    lights, vd = light_materials(s), TC.view_dependent_materials(s)
    mod = D.demodulation
    r, plain = new_renderer(s), new_renderer(s)
    try:
        m64, m32 = V.VarianceGuided(), V.VarianceGuided()
        tainted = np.zeros((H, W), bool)
        for k, (name, n) in enumerate(VC.SEQUENCE):
            cam = cams[name]
            for q in (r, plain):
                render_frame(q, cam, n, SEED + k)
            acc, g = r.accumulator(), r.guides(camera=cam)
            kw = dict(height=H, light_materials=lights, view_dependent_materials=vd, temporal=True, min_history_frames=mhf)
            prev_cam = m64.camera if m64.history is not None else cam
            ref_rgba, _ = m64.frame(acc, n, g, cam, **kw)
            m32.frame(acc, n, g, cam, dtype=np.float32, **kw)
            diff = (m64.taps != m32.taps) | (m64.used_temporal != m32.used_temporal)
            tainted = diff | VC.carried(tainted, g, prev_cam, cam, H, m64.taps)
            print(f"{which} min_history_frames {mhf} frame {k}: {int(diff.sum())} pixels decided differently in float32, {int(tainted.sum())} left out, "
                  f"{float(m64.used_temporal.mean()):.1%} take var_t")
            assert tainted.mean() <= diff.mean() + VC.CAP
            if name == "base":                                                 # the switch, on the static frames
                assert np.all(m64.used_temporal == (k >= VC.FIRST_TEMPORAL[mhf]))
            else:
                assert 0.2 < m64.used_temporal.mean() < 1.0
            rgba, px = r.denoise_variance_guided(temporal=True, min_history_frames=mhf, camera=cam)
            hist, var = r.temporal_history(), r.variance()
            plain.denoise_temporal(camera=cam)
            assert np.array_equal(bits(hist), bits(plain.temporal_history()))   # cgpt_denoise_temporal's colour history, bit for bit
            keep = ~tainted
            assert_close(hist, m64.history, f"frame {k}: colour history", keep)
            assert_close(var, m64.var, f"frame {k}: variance", keep)
            c = hist[..., :3].astype(np.float64)
            out = V.passes(c, var.astype(np.float64), g, 5)[0] * mod(g, lights)
            assert_close(rgba[..., :3], out, f"frame {k}: output from the device's colour and variance")
            assert_pixels_close(px, out)
            assert np.all(rgba[..., 3] == 1.0)
            if not tainted.any():
                assert_close(rgba, ref_rgba, f"frame {k}: output against the whole statement")
            m64.history = hist.astype(np.float64)                              # the next step starts from the device's colour history
            m32.history = m64.history.copy()
    finally:
        r.close()
        plain.close()


def test_iterations_0_behind_the_temporal_stage_is_cgpt_denoise_temporals_output(pairs):
    _, s = pairs["all_kinds"]
    cams = cameras(s)
    a, b = new_renderer(s), new_renderer(s)
    try:
        for k, name in enumerate(("base", "translation")):
            for q in (a, b):
                render_frame(q, cams[name], 2, SEED + k)
            got = a.denoise_variance_guided(iterations=0, temporal=True, camera=cams[name])
            want = b.denoise_temporal(iterations=0, camera=cams[name])
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            assert np.array_equal(bits(a.temporal_history()), bits(b.temporal_history()))
            assert a.variance().max() > 0
    finally:
        a.close()
        b.close()


# ---- 3. what drops the moments ---------------------------------------------------------------------------------------------------------

def spatial_only(r, g):
    """the variance map of the frame when no moments are used: var_s of the image the passes read, which the stored colour is"""
    return V.spatial_variance(r.temporal_history()[..., :3].astype(np.float64), g)


def test_a_cgpt_denoise_temporal_call_drops_the_moments_and_keeps_the_colour_history(pairs):
    _, s = pairs["all_kinds"]
    cam = cameras(s)["base"]
    r = new_renderer(s)
    try:
        def frame(seed, call):
            render_frame(r, cam, 2, seed)
            call()
            return r.temporal_history()[..., 3]

        def guided():
            r.denoise_variance_guided(temporal=True, min_history_frames=2, camera=cam)

        assert np.all(frame(SEED, guided) == 2)
        assert np.all(frame(SEED + 1, guided) == 4)
        g = r.guides(camera=cam)
        v_t = r.variance()
        assert not np.all(VC.rel_err(v_t, spatial_only(r, g)) <= VC.TOL)        # var_t, not var_s
        assert np.all(frame(SEED + 2, lambda: r.denoise_temporal(camera=cam)) == 6)
        assert np.all(frame(SEED + 3, guided) == 8)                            # the colour history went on
        assert_close(r.variance(), spatial_only(r, g), "after cgpt_denoise_temporal: the variance is spatial")
        assert np.all(frame(SEED + 4, guided) == 10)
        assert not np.all(VC.rel_err(r.variance(), spatial_only(r, g)) <= VC.TOL)   # K = 2 + 2 >= 2 x 2: temporal again
    finally:
        r.close()


def test_whatever_drops_the_colour_history_drops_the_moments():
    _, s = all_kinds_pair(W / H)
    cam = s.camera()
    r = new_renderer(s)
    try:
        size = [W, H]
        flags = dict(demodulate=True)

        def frame(seed):
            """(history lengths, the variance is the spatial estimate)"""
            render_frame(r, cam, 2, seed, size[0], size[1])
            r.denoise_variance_guided(temporal=True, min_history_frames=2, camera=cam, **flags)
            var_s = V.spatial_variance(r.temporal_history()[..., :3].astype(np.float64), r.guides(camera=cam))
            return r.temporal_history()[..., 3], bool(np.all(VC.rel_err(r.variance(), var_s) <= VC.TOL))

        def material():
            s.set_material(1, P.Material(albedo=(0.3, 0.9, 0.5)))
            r.update_materials(s)

        def refit():
            v, i = standin_mesh(2)
            w = v.copy()
            w[:, :3] += np.float32([0.4, 0.3, 0.0])
            r.refit_mesh(BIG, P.triangles_from_arrays(w, i))

        def transform():
            mats = np.tile(np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (7, 1))
            mats[TRI, 3] = 0.5
            r.update_transforms(mats)

        def smaller():
            size[1] = H - 3

        def flag():
            flags["demodulate"] = False

        Hn, spatial = frame(SEED)
        assert np.all(Hn == 2) and spatial
        for k, edit in enumerate((material, refit, transform, smaller, flag, r.temporal_reset)):
            Hn, spatial = frame(SEED + 2 * k + 1)
            assert np.all(Hn == 4) and not spatial, f"no moments before {edit.__name__}"
            edit()
            Hn, spatial = frame(SEED + 2 * k + 2)
            assert np.all(Hn == 2) and spatial, edit.__name__
    finally:
        r.close()


# ---- 4. invariance, side effects -----------------------------------------------------------------------------------------------------

def three_calls(r, cams, kernel=P.KERNEL_AUTO):
    render_frame(r, cams["base"], 2, SEED, kernel=kernel)
    outs = list(r.denoise_variance_guided(camera=cams["base"])) + [r.variance()]
    outs += list(r.denoise_variance_guided(temporal=True, min_history_frames=2, camera=cams["base"])) + [r.variance()]
    render_frame(r, cams["translation"], 2, SEED + 1, kernel=kernel)
    outs += list(r.denoise_variance_guided(temporal=True, min_history_frames=2, camera=cams["translation"])) + [r.variance(), r.temporal_history()]
    return [bits(a).copy() for a in outs]


def test_same_bytes_for_every_render_path_and_a_device_group(pairs):
    _, s = pairs["all_kinds"]
    cams = cameras(s)
    outs = []
    for kernel in KERNELS[:3]:
        r = new_renderer(s)
        try:
            outs.append(three_calls(r, cams, kernel))
        finally:
            r.close()
    r = new_renderer(s, [0, 0, 0], N.CTX_GATHER_PEER_COPY)                      # three ranks on one GPU
    try:
        assert r.is_group
        outs.append(three_calls(r, cams))
    finally:
        r.close()
    assert np.any(outs[0][-1].view(np.float32)[..., 3] == 4)                   # the last frame did reproject
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("group", [False, True])
def test_nothing_else_moves_and_the_other_denoisers_are_unchanged(pairs, group):
    _, s = pairs["reference"]
    cam = cameras(s)["base"]
    dev, flags = ([0, 0, 0], N.CTX_GATHER_PEER_COPY) if group else (0, 0)
    r = new_renderer(s, dev, flags)
    try:
        r.render(W, H, 3, seed=SEED, camera=cam, counters=True)

        def state():
            return (bits(r.accumulator()).copy(), r.pixels().copy(), stats_bytes(r), bits(r.guides(camera=cam)).copy())

        plain = [bits(a).copy() for a in r.denoise(camera=cam)]
        temporal = [bits(a).copy() for a in r.denoise_temporal(camera=cam)]
        r.temporal_reset()
        before = state()
        r.denoise_variance_guided(camera=cam)
        r.denoise_variance_guided(camera=cam, iterations=0, demodulate=False)
        r.variance()
        assert r.L.cgpt_read_temporal_history(r._ctx, None, 0) == N.CGPT_ERR_INVALID   # without the flag no history is written
        r.denoise_variance_guided(camera=cam, temporal=True)
        r.temporal_reset()
        after = state()
        for a, b in zip(before, after):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        again = [bits(a) for a in r.denoise(camera=cam)]
        assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
        again = [bits(a) for a in r.denoise_temporal(camera=cam)]            # from no history, as the first one
        assert np.array_equal(temporal[0], again[0]) and np.array_equal(temporal[1], again[1])
        assert r.stats().num_accumulated == 3
    finally:
        r.close()


def test_interleaved_calls_equal_calls_made_alone():
    """The three filtering calls share a context's buffers and validity flags: on one context (A) they are interleaved -- D cgpt_denoise,
    T cgpt_denoise_temporal, V cgpt_denoise_variance_guided, VT with the temporal flag -- and every call's output, variance map and
    colour history must be the bytes of the same call where only the history's calls are made (B: A's T and VT calls) or only the
    others (C: A's D and V calls).  37x21: partial tiles both ways and step-2 taps outside the band; the diffuse reference layout."""
    w, h, spp = 37, 21, 2
    _, s = reference_layout_pair(*standin_mesh(2), 1, aspect=w / h)
    cam = s.camera()
    a, b, c = new_renderer(s), new_renderer(s), new_renderer(s)
    try:
        a.render(w, h, spp, seed=SEED, camera=cam)
        acc = a.accumulator()
        for q in (a, b, c):
            q.load_accumulator(acc, spp, w, h)
        calls = {"D": lambda q, it: q.denoise(iterations=it, camera=cam),
                 "T": lambda q, it: q.denoise_temporal(iterations=it, camera=cam),
                 "V": lambda q, it: q.denoise_variance_guided(iterations=it, camera=cam),
                 "VT": lambda q, it: q.denoise_variance_guided(iterations=it, temporal=True, min_history_frames=2, camera=cam)}

        def state(q, kind, it):
            out = list(calls[kind](q, it))
            if kind in ("V", "VT"):
                out.append(q.variance())
            if kind in ("T", "VT"):
                out.append(q.temporal_history())
            return [bits(x).copy() for x in out]

        for k, kind in enumerate(("T", "D", "V", "T", "V", "D", "VT", "D", "V", "VT", "T", "VT")):
            it = 2 * (k % 2)
            got, want = state(a, kind, it), state(b if kind in ("T", "VT") else c, kind, it)
            assert len(got) == len(want) >= 2
            for x, y in zip(got, want):
                assert np.array_equal(x, y), f"call {k} ({kind}, {it} iterations)"
    finally:
        for q in (a, b, c):
            q.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------

def raw_call(r, cam, params, temporal, variance, rgba_n=None, px_n=None, rgba=True, px=True):
    n = r.n_rows * r.width
    rgba_n = 4 * n if rgba_n is None else rgba_n
    px_n = n if px_n is None else px_n
    fb = np.full(max(rgba_n, 1), 7.0, np.float32)
    pb = np.full(max(px_n, 1), 7, np.uint32)
    ref = lambda x: C.byref(x) if x is not None else None                      # noqa: E731
    rc = r.L.cgpt_denoise_variance_guided(r._ctx, ref(cam), ref(params), ref(temporal), ref(variance),
                                          fb.ctypes.data_as(C.POINTER(C.c_float)) if rgba else None, rgba_n,
                                          pb.ctypes.data_as(C.POINTER(C.c_uint32)) if px else None, px_n)
    return rc, fb, pb


def raw_read(r, name, n_floats):
    b = np.full(max(n_floats, 1), 7.0, np.float32)
    return getattr(r.L, name)(r._ctx, b.ctypes.data_as(C.POINTER(C.c_float)), n_floats), b


def untouched(*bufs):
    return all(np.all(b == 7) for b in bufs)


def test_refusals_change_nothing(pairs):
    _, s = pairs["reference"]
    cam = cameras(s)["base"]
    ok = N.DenoiseParams(5, N.DENOISE_DEMODULATE_ALBEDO, 4.0, 0.2, 0.3)
    tok = N.TemporalParams(64.0, 0.9, 0.01, 0)
    vok = N.VarianceParams(4.0, 4, N.VARIANCE_TEMPORAL)
    n = W * H
    r = P.Renderer(0)
    try:
        r.width, r.n_rows = W, H
        rc, fb, pb = raw_call(r, cam, ok, tok, vok)                            # no scene
        assert rc == N.CGPT_ERR_NO_SCENE and untouched(fb, pb)
        r.upload(s)
        rc, fb, pb = raw_call(r, cam, ok, tok, vok)                            # a scene, no band yet
        assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb)
        rc, vb = raw_read(r, "cgpt_read_variance", n)                          # no call yet
        assert rc == N.CGPT_ERR_INVALID and untouched(vb)
        r.width = 0
        r.render(W, H, 2, seed=SEED, camera=cam, counters=True)
        rc, vb = raw_read(r, "cgpt_read_variance", n)                          # rendered, still no call
        assert rc == N.CGPT_ERR_INVALID and untouched(vb)

        def state():
            rc_h, hb = raw_read(r, "cgpt_read_temporal_history", 4 * n)
            rc_v, vb = raw_read(r, "cgpt_read_variance", n)
            return r.accumulator().tobytes(), r.pixels().tobytes(), stats_bytes(r), rc_h, hb.tobytes(), rc_v, vb.tobytes()

        rc, fb, pb = raw_call(r, cam, None, None, None)                        # NULL parameters are the defaults: no temporal stage
        assert rc == 0 and not untouched(fb) and not untouched(pb)
        assert np.array_equal(bits(r.denoise_variance_guided(camera=cam)[0]), bits(fb).reshape(H, W, 4))
        assert state()[3] == N.CGPT_ERR_INVALID and state()[5] == 0
        rc, fb, pb = raw_call(r, cam, ok, None, vok)                           # NULL temporal: cgpt_denoise_temporal's defaults
        assert rc == 0
        r.temporal_reset()
        assert np.array_equal(bits(r.denoise_variance_guided(camera=cam, temporal=True)[0]), bits(fb).reshape(H, W, 4))
        before = state()
        assert before[3] == 0 and before[5] == 0
        inf, nan = float("inf"), float("nan")
        for vargs in ((0.0, 4, 1), (-1.0, 4, 1), (inf, 4, 1), (nan, 4, 1), (4.0, 0, 1), (4.0, 4, 2), (4.0, 4, 0x80000001), (4.0, 4, 4), (nan, 4, 0),
                      (4.0, 0, 0)):
            rc, fb, pb = raw_call(r, cam, ok, tok, N.VarianceParams(*vargs))
            assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb), vargs
        for targs in ((0.5, 0.9, 0.01, 0), (inf, 0.9, 0.01, 0), (nan, 0.9, 0.01, 0), (64.0, 1.5, 0.01, 0), (64.0, nan, 0.01, 0), (64.0, 0.9, 0.0, 0),
                      (64.0, 0.9, inf, 0), (64.0, 0.9, 0.01, 2)):               # cgpt_denoise_temporal's own, with the flag
            rc, fb, pb = raw_call(r, cam, ok, N.TemporalParams(*targs), vok)
            assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb), targs
        for args in ((11, 1, 4.0, 0.2, 0.3), (5, 2, 4.0, 0.2, 0.3), (5, 4, 4.0, 0.2, 0.3), (5, 1, 0.0, 0.2, 0.3), (5, 1, 4.0, -0.2, 0.3), (5, 1, 4.0, 0.2, nan),
                     (5, 1, inf, 0.2, 0.3)):                                   # cgpt_denoise's own; sigma_color is validated though unused
            rc, fb, pb = raw_call(r, cam, N.DenoiseParams(*args), tok, vok)
            assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb), args
        for kw in (dict(rgba_n=4 * n - 4), dict(px_n=n + 1), dict(rgba=False, px=False)):
            rc, fb, pb = raw_call(r, cam, ok, tok, vok, **kw)
            assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb), kw
        rc, fb, pb = raw_call(r, None, ok, tok, vok)                           # no camera
        assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb)
        for size in (n - 1, 4 * n, 0):                                         # a wrong size
            rc, vb = raw_read(r, "cgpt_read_variance", size)
            assert rc == N.CGPT_ERR_INVALID and untouched(vb)
        assert state() == before
        rc, fb, pb = raw_call(r, cam, ok, N.TemporalParams(0.5, 7.0, nan, 9), N.VarianceParams(4.0, 4, 0))   # without the flag `temporal` is not read
        assert rc == 0 and state()[3:5] == before[3:5]
        rc, fb, pb = raw_call(r, cam, N.DenoiseParams(10, 0, 1e-3, 1e3, 1e-6), N.TemporalParams(1.0, -1.0, 1e-30, 1),
                              N.VarianceParams(1e-30, 0xFFFFFFFF, 1))          # the limits are accepted
        assert rc == 0 and not untouched(fb) and not untouched(pb)
        r.temporal_reset()
        r.denoise_variance_guided(camera=cam, temporal=True)
        before = state()
        r.reset_accumulator()                                                  # nothing accumulated
        acc0 = state()[:3]
        rc, fb, pb = raw_call(r, cam, ok, tok, vok)
        assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb) and state()[:3] == acc0 and state()[3:] == before[3:]
        r.render(W, H, 1, seed=SEED, camera=cam, settings=P.Settings(debug_render_mode=P.DEBUG_RAY_DEPTH))   # a debug view
        rc, fb, pb = raw_call(r, cam, ok, tok, vok)
        assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb) and state()[3:] == before[3:]
        r.reset_accumulator()
        r.render(W, H - 3, 1, seed=SEED, camera=cam)                           # another band: the map belongs to the earlier one
        rc, vb = raw_read(r, "cgpt_read_variance", W * (H - 3))
        assert rc == N.CGPT_ERR_INVALID and untouched(vb)
    finally:
        r.close()
    r = new_renderer(s)
    try:
        r.render(W, H, 2, seed=SEED, camera=cam, interleave=(4, 2, 1))         # an interleaved band
        rc, fb, pb = raw_call(r, cam, ok, tok, vok)
        assert rc == N.CGPT_ERR_INVALID and untouched(fb, pb)
        rc, vb = raw_read(r, "cgpt_read_variance", r.n_rows * W)
        assert rc == N.CGPT_ERR_INVALID and untouched(vb)
    finally:
        r.close()


# ---- 6. usefulness ----------------------------------------------------------------------------------------------------------------------

def rmse_to(want):
    return lambda a: float(np.sqrt(np.mean((np.clip(a[..., :3], 0, 1).astype(np.float64) - want) ** 2)))


@pytest.mark.parametrize("mat", [1, 3])
def test_variance_guided_4spp_is_closer_to_1024spp_than_raw(mat):
    """RMSE of radiance clamped to [0, 1] against a raw 1024-spp render, 160x120, default parameters, the diffuse (material 1) and the
    glass (material 3) reference layout: the variance-guided output must beat the raw 4-spp frame.  The ratio next to cgpt_denoise's is
    printed (DESIGN.md 5.23 records it); it is not required to win."""
    w, h = 160, 120
    _, s = reference_layout_pair(*standin_mesh(3), mat, aspect=w / h)
    ref, r = new_renderer(s), new_renderer(s)
    try:
        ref.render(w, h, 1024, seed=SEED)
        rmse = rmse_to(np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64))
        r.render(w, h, 4, seed=SEED)
        raw = r.accumulator()[..., :3] / np.float32(4)
        guided, plain = r.denoise_variance_guided()[0], r.denoise()[0]
        print(f"material {mat} at 4 spp: RMSE raw {rmse(raw):.4f} cgpt_denoise {rmse(plain):.4f} variance-guided {rmse(guided):.4f}; "
              f"ratio to raw {rmse(guided) / rmse(raw):.3f} (cgpt_denoise {rmse(plain) / rmse(raw):.3f})")
        assert rmse(guided) < rmse(raw)
    finally:
        ref.close()
        r.close()


def test_variance_guided_orbit_at_1spp_is_closer_to_1024spp_than_the_last_frame_raw():
    """test_gpu_temporal's orbit (six frames, 2 degrees a frame, 1 spp, the diffuse reference layout, 160x120) with the temporal flag: the
    output must beat the last frame raw.  The ratio next to cgpt_denoise_temporal's is printed; it is not required to win."""
    w, h = 160, 120
    _, s = reference_layout_pair(*standin_mesh(3), 1, aspect=w / h)
    cams = [orbit_camera(s, k, w, h) for k in range(6)]
    ref, r, t = new_renderer(s), new_renderer(s), new_renderer(s)
    try:
        ref.render(w, h, 1024, seed=SEED, camera=cams[-1])
        rmse = rmse_to(np.clip(ref.accumulator()[..., :3] / np.float32(1024), 0, 1).astype(np.float64))
        for k, cam in enumerate(cams):
            for q in (r, t):
                render_frame(q, cam, 1, SEED + 1 + k, w, h)
            guided = r.denoise_variance_guided(temporal=True, camera=cam)[0]
            temporal = t.denoise_temporal(camera=cam)[0]
        raw = r.accumulator()[..., :3]
        print(f"orbit at 1 spp: RMSE raw {rmse(raw):.4f} cgpt_denoise_temporal {rmse(temporal):.4f} variance-guided {rmse(guided):.4f}; "
              f"ratio to raw {rmse(guided) / rmse(raw):.3f} (cgpt_denoise_temporal {rmse(temporal) / rmse(raw):.3f})")
        assert rmse(guided) < rmse(raw)
    finally:
        for q in (ref, r, t):
            q.close()


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------------

def test_example_writes_variance_guided_previews(tmp_path):
    from cpugpupathtracing_amd import build as B
    repo = B.REPO_DIR
    exe = str(tmp_path / "render_main")
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(repo, "include"), "-I" + os.path.join(B.CSRC, "host"),
                           os.path.join(repo, "examples", "render_main.cpp"), "-L" + B.LIB_DIR, "-lcpugpupt",
                           "-Wl,-rpath," + B.LIB_DIR, "-o", exe])
    out = subprocess.run([exe, "--denoise", "--variance-guided", "64", "48", "4", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    plain, guided = (tmp_path / "render_denoised.ppm").read_bytes(), (tmp_path / "render_variance_guided.ppm").read_bytes()
    assert len(plain) == len(guided) and plain != guided
    for flags in (["--temporal"], ["--temporal", "--variance-guided"]):       # the second run writes _variance_guided in place of _temporal
        out = subprocess.run([exe] + flags + ["64", "48", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    for k in range(8):
        assert os.path.exists(tmp_path / f"temporal_{k:02d}_variance_guided.ppm"), k
    assert (tmp_path / "temporal_07_variance_guided.ppm").read_bytes() != (tmp_path / "temporal_07_temporal.ppm").read_bytes()
