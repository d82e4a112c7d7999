"""The host path loop of tests/replay_ref.py on its own, no GPU: its seed and primary rays against the C oracle's bit for bit, the loop
itself (with the oracle's intersect_rays and the float64 shade model as its two steps) against an oracle render at first_sample > 0 on a
band of rows, and the dry run of every configuration of test_gpu_path_replay.py with the model traversal and the float32 shade model:
the share of undecided samples, from the model alone, and that the populations are worth having."""
import numpy as np
import pytest

import oracle as O
import replay_ref as RP
import shade_ref as S

MAX_UNDECIDED_DRY = 0.01          # half of the 2 % cap (test_shade_reference.MAX_UNDECIDED): the device's paths drift from the dry run's by rounding
SIZES = ((RP.W, RP.H), (16, 16), (7, 5), (33, 19))                                 # 1 / 40, 1 / 28, 1 / 7, 1 / 5, 1 / 33 and 1 / 19 are inexact


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pcg_seed_is_the_oracles():
    L = O.lib()
    rng = np.random.default_rng(1)
    pixel = np.concatenate([np.arange(64), rng.integers(0, 1 << 32, 200, dtype=np.uint64), [0xFFFFFFFF, RP.W * RP.H - 1]]).astype(np.uint64)
    sample = np.concatenate([np.arange(64) % 7, rng.integers(0, 1 << 32, 200, dtype=np.uint64), [0xFFFFFFFF, 4]]).astype(np.uint64)
    for seed in (0, 1, RP.SEED, 0xFFFFFFFF):
        mine = RP.pcg_seed(pixel, sample, seed)
        theirs = np.array([L.orc_pcg_seed(int(p), int(s), seed) for p, s in zip(pixel, sample)], np.uint32)
        assert np.array_equal(mine, theirs), hex(seed)


def _oracle_with_camera(camera):
    o = O.OracleScene()
    o.add_material(albedo=(0.5, 0.5, 0.5))
    o.add_plane((0, 1, 0), (0, 0, 0), 0)
    o.set_camera(*camera)
    return o


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_primary_rays_are_the_oracles_bit_for_bit(size):
    """camera_rays (float32 numpy, the device's operation order) on the host library's camera against orc_camera_ray, for both views."""
    import cpugpupathtracing_amd as P
    w, h = size
    s = P.Scene()
    try:
        for view in RP.VIEWS:
            pos, look, fov, _ = view["camera"]
            camera = (pos, look, fov, w / h)
            s.set_camera(*camera)
            mo, md = RP.camera_rays(s.camera(), w, h)
            o = _oracle_with_camera(camera)
            try:
                oo, od = o.camera_rays(w, h)
            finally:
                o.close()
            assert np.array_equal(_bits(mo), _bits(oo)) and np.array_equal(_bits(md), _bits(od)), (view["name"], size)
    finally:
        s.close()


def test_pack_pixels_is_the_oracles():
    L = O.lib()
    import ctypes as C
    acc = np.array([[0.0, 0.5, 1.0, 1], [2.0, -1.0, 0.999, 1], [3.0, 1.5, 0.004, 3], [1e-3, 254.6 / 255 * 5, 5.0, 5]], np.float32)
    for n in (1, 3, 5):
        mine = RP.pack_pixels(acc, n)
        for k in range(acc.shape[0]):
            v = (acc[k] / np.float32(n)).astype(np.float32)
            assert mine[k] == L.orc_vec4_to_uint(v.ctypes.data_as(C.POINTER(C.c_float))), (n, k)


# ---- the loop against an oracle render --------------------------------------------------------------------------------------------------------
def _oracle_scene(sc):
    """The level-0 ModelScene in the oracle; the stand-alone triangle as a mesh of one triangle (the oracle has no triangle objects; the
    object index, the intersector and the shading normal -- v0's -- are the same)."""
    o = O.OracleScene()
    for m in sc.materials:
        assert not m["roughness"] and not m["transmission_roughness"]
        o.add_material(**{k: v for k, v in m.items() if k not in ("roughness", "transmission_roughness")})
    for ob in sc.objects:
        if ob["kind"] == "plane":
            o.add_plane(ob["normal"], ob["point"], ob["mat"])
        elif ob["kind"] == "sphere":
            o.add_sphere(ob["center"], float(ob["radius"]), ob["mat"])
        elif ob["kind"] == "triangle":
            o.add_mesh(np.concatenate([ob["positions"], ob["normals"]], 1).astype(np.float32), np.arange(3, dtype=np.uint32), ob["mat"])
        else:
            assert not ob["smooth"] and ob["transform"] is None
            o.add_mesh(ob["vertices"], ob["indices"], ob["mat"])
    for l in sc.lights:
        o.add_light(l)
    return o


BAND = (5, 23)                                                                     # rows of the oracle test: neither end on a tile edge


def test_the_loop_reproduces_an_oracle_render_after_earlier_samples_on_a_band():
    """The first view at level 0, RNG_PIXEL_PCG: the oracle renders samples 0 and 1 on rows 5..22, then samples 2, 3, 4; the replay -- the
    oracle's intersect_rays as its trace step, the float64 model as its shade step -- starts from the accumulator after the first two and
    must give the accumulator after all five.  The rule of test_float64_model_reproduces_an_oracle_render_pixel_by_pixel: pixels one of
    whose paths is undecided are left out, at most 5 % of them; the rest lie within 1e-4 relative + 1e-6 of the oracle's accumulator.
    Undecided here is a sample the shade model calls so, and a shadow ray the tracer does not decide: one that ends on the sphere light's
    rim, where the chord is shorter than intersect_sphere's error and the light itself is met before or behind the ray's end (tmax, two
    nudges short of the light) depending on the last bit of the ray -- found by tracing it 32 more times with every float of the ray moved by up to 4 ulps (the oracle's own shadow ray differs from the model's by such amounts).
    traced_rays does not depend on a shadow ray's answer, so it is compared when no sample is undecided by the shade model: then every path
    took the oracle's branches and the replay's ray count (extend, shadow, kept and in-place re-traces) must be the oracle's exactly.  The
    seed is one for which that holds, which is asserted, so that the comparison cannot lapse unseen."""
    sc, _ = RP.build_scene()
    sc.device_scene().close()                                                  # records the mesh light's total_area as the host library computes it
    view = RP.VIEWS[0]
    st = RP.view_settings(view)
    o = _oracle_scene(sc)
    shaky = []                                                                 # per shadow trace: the rays whose answer changes when the ray moves by a few ulps

    jitter = np.random.default_rng(11)

    def trace(origins, dirs, tmax=None):
        out = o.intersect_rays(origins, dirs, tmax)
        if tmax is not None:
            differs = np.zeros(tmax.shape[0], bool)
            for _ in range(32):
                e = [(1.0 + jitter.uniform(-4.0, 4.0, a.shape) * 2.0 ** -24) for a in (origins, dirs, tmax)]
                hit = o.intersect_rays((origins * e[0]).astype(np.float32), (dirs * e[1]).astype(np.float32), (tmax * e[2]).astype(np.float32))[1]
                differs |= (hit == S.NO_HIT) != (out[1] == S.NO_HIT)
            shaky.append(differs)
        return out
    try:
        o.set_camera(*view["camera"])
        o.set_settings(st["max_ray_depth"], st["nee"], st["cosine"], st["rr"])
        o.render(RP.W, RP.H, view["first_sample"], O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, RP.SEED, rows=BAND)
        before = o.accumulator()[BAND[0]:BAND[1]].copy()
        assert o.num_accumulated() == view["first_sample"] and before[..., 3].min() == view["first_sample"]
        o.reset_stats()
        o.render(RP.W, RP.H, view["n_samples"], O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, RP.SEED, rows=BAND)
        full = o.accumulator()
        after = full[BAND[0]:BAND[1]].copy()
        assert not full[:BAND[0]].any() and not full[BAND[1]:].any()
        rays = o.stats().traced_rays
        out = RP.replay(trace, lambda smp, s_: S.shade(sc, s_, smp, np.float64), o.camera_rays(RP.W, RP.H), RP.W, RP.H,
                        range(*BAND), view["first_sample"], view["n_samples"], RP.SEED, st, accumulator=before)
    finally:
        o.close()
    n_pix = (BAND[1] - BAND[0]) * RP.W
    und, rim = np.zeros(n_pix * view["n_samples"], bool), np.zeros(n_pix * view["n_samples"], bool)
    calls = iter(shaky)
    for step in out["steps"]:
        und[step["idx"]] |= step["results"]["undecided"]
        sh = (step["results"]["flags"] & S.SHADOW) != 0
        if sh.any():
            rim[step["idx"][sh]] |= next(calls)
    assert next(calls, None) is None
    keep = ~(und | rim).reshape(n_pix, view["n_samples"]).any(1)
    acc, ref = out["accumulator"].reshape(n_pix, 4).astype(np.float64), after.reshape(n_pix, 4).astype(np.float64)
    err = np.abs(acc[:, :3] - ref[:, :3])
    lit = float(((ref[:, :3] - before.reshape(n_pix, 4)[:, :3]).sum(1) > 0).mean())
    print(f"kept share {keep.mean():.4f} (undecided samples {int(und.sum())}, shadow rays on the rim {int(rim.sum())})  lit pixels {lit:.3f}  "
          f"largest error / bound on the kept pixels {(err / (1e-4 * np.abs(ref[:, :3]) + 1e-6))[keep].max():.3f}  steps {len(out['steps'])}  "
          f"rays {out['rays']} (oracle {rays})  unwalked {out['unwalked']}")
    assert keep.mean() >= 0.95 and lit > 0.5
    assert np.array_equal(acc[:, 3], ref[:, 3])
    assert np.all(err[keep] <= 1e-4 * np.abs(ref[keep, :3]) + 1e-6)
    assert not und.any(), "the seed was chosen so that no sample is undecided and the ray counts are compared"
    assert out["rays"] == rays and out["unwalked"] > 0


# ---- the dry run ---------------------------------------------------------------------------------------------------------------------------------
_scenes = {}


def _scene_at(level):
    """(ModelScene, device Scene) at `level`, raised by the ladder's model edits."""
    if level not in _scenes:
        sc, names = RP.build_scene()
        for k in range(1, level + 1):
            RP.ladder(names)[k][0](sc)
        assert sc.lobe_level() == level
        _scenes[level] = (sc, sc.device_scene(), names)
    return _scenes[level]


@pytest.mark.parametrize("candidates", RP.CANDIDATES)
@pytest.mark.parametrize("level", RP.LEVELS)
def test_dry_run_has_few_undecided_samples_and_a_population_worth_having(level, candidates):
    sc, ds, names = _scene_at(level)
    trace = RP.model_trace(sc, ds)
    n = und = ill = 0
    chains, flags_or, hit_objs, by_view = set(), 0, set(), {}
    for view in RP.VIEWS:
        rays = RP.camera_rays(RP.view_camera(ds, view), RP.W, RP.H)
        out = RP.replay(trace, lambda smp, st: S.shade(sc, st, smp, np.float32, candidates=candidates), rays, RP.W, RP.H, range(RP.H),
                        view["first_sample"], view["n_samples"], RP.SEED, RP.view_settings(view))
        by_view[view["name"]] = out
        for step in out["steps"]:
            res, smp = step["results"], step["samples"]
            n += smp.shape[0]; und += int(res["undecided"].sum()); ill += int(res["ill"].sum())
            chains |= set(np.unique((res["flags"] >> S.CHAIN_SHIFT) & 3).tolist())
            flags_or |= int(np.bitwise_or.reduce(res["flags"]))
            hit_objs |= set(np.unique(smp["obj"][(smp["depth"] > 0) & (smp["obj"] != S.NO_HIT)]).tolist())
    share = und / n
    outside, inside = by_view["outside"], by_view["inside_glass"]
    lit = float((outside["accumulator"][..., :3].sum(-1) > 0).mean())
    print(f"level {level} M {candidates}: {n} samples in {len(outside['steps'])} + {len(inside['steps'])} steps, undecided {und} = {share:.4f} "
          f"(ill-conditioned {ill}); lit {lit:.3f} outside, {float((inside['accumulator'][..., :3].sum(-1) > 0).mean()):.3f} inside; "
          f"rays {outside['rays']} + {inside['rays']}, unwalked {outside['unwalked']} + {inside['unwalked']}")
    assert share <= MAX_UNDECIDED_DRY, share
    assert lit > 0.5, "more than half of the first view's pixels carry radiance (the second view has no NEE and sees the lamp through glass)"
    assert {S.CHAIN_REFLECT, S.CHAIN_REFRACT} <= chains and flags_or & S.SHADOW and flags_or & S.ENERGY
    # NEE is off there, so total internal reflection is the in-place loop, whose results carry no chain choice; the kept ray (chain choice
    # TIR without the terminate bit) needs NEE and a polished dielectric hit from inside at an angle a sphere never gives: the mesh, levels 0 and 1
    assert inside["unwalked"] > 100, "total internal reflection in the inside-glass view"
    assert outside["unwalked"] > 0 or level >= 2
    assert hit_objs == set(range(len(sc.objects))), ("every object is hit above depth 0", hit_objs)
    assert {sc.objects[k]["mat"] for k in hit_objs} == set(range(len(sc.materials)))
