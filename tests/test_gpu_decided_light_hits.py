"""wf_shade ends the path of a fresh extend ray that its probe decides as a hit on a light (wf_shade: "Probe"; rt_device.hpp probe_scene,
ProbeLight): the next round's pass would do nothing for such a path but shade_bounce's light branch, so the emission is added -- or, with
NEE on after a diffuse bounce, not added -- in the pass that made the ray, and no slot, state or list entry is written.  The knob
`probe_lights` must never change a result: accumulator and pixels bit for bit and traced_rays equal between the wavefront pipeline with
probe_lights 1 and 0, the megakernel and the persistent kernel, and traced_rays equal to the oracle's (every decided ray is still one
IntersectScene call; the oracle has no resampled NEE, so four candidates are compared across the device paths only).

The frame is the 70 x 36 one of test_gpu_shade_prologue.py (padded edge tiles in both directions; sky, ground, glass and a visible
emitter among the primary hits) with its sample counts 5, 64 and 96.  The bounce rays of its ground pixels reach the three light spheres
without entering a box of the stand-in.  stats.probe_resolved shows that the new path ran: it is strictly larger with probe_lights 1.

The ordering rule.  A listed shadow ray adds its pending radiance in the next trace, before the next shade adds the emission; so where
the emission would be added and the bounce's shadow ray is undecided, the extend ray stays with the lists.  That needs a specular lobe of
a material that also samples lights: test_ordering_rule puts a sphere, or a wall, of the C2 material (half mirror, half diffuse) beside a
light with a mesh between them, reached by diffuse bounces off the ground (a camera ray that hits it is a specular chain and is not probed)."""
import numpy as np
import pytest

import oracle as O
import cpugpupathtracing_amd as P
from scenes import MAT_SPEC_DIFFUSE, pair_from, reference_layout_pair, standin_mesh

pytestmark = pytest.mark.gpu

W, H = 70, 36
SEED = 0x2468ACE1
GLASS = 3
LIGHT_CENTRE, LIGHT_RADIUS = (-4.0, 2.0, 0.0), 0.9
DEVICE_REFERENCES = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _settings(nee):
    return P.Settings(next_event_estimation_enabled=nee)


_SCENES = {}


def _bench_like(nee):
    """test_gpu_shade_prologue.py's scene: the shipped layout around the level-2 glass stand-in, one more light sphere in view"""
    if nee not in _SCENES:
        o, s = reference_layout_pair(*standin_mesh(2), GLASS, aspect=W / H, settings=_settings(nee))
        li = o.add_sphere(LIGHT_CENTRE, LIGHT_RADIUS, 2)
        assert li == s.add_sphere(LIGHT_CENTRE, LIGHT_RADIUS, 2)
        o.add_light(li); s.add_light(li)
        _SCENES[nee] = (o, s)
    return _SCENES[nee]


def _plane_and_light(nee):
    """no mesh: every bounce ray that reaches the light is decided"""
    return pair_from([("plane", (0, 1, 0), (0, -3, 0), 1), ("sphere", (3.0, 1.0, -2.0), 2.5, 2)], list(P.REFERENCE_MATERIALS), [1],
                     camera=((0, 0, 8), (0, 0, -1), 60.0, W / H), settings=_settings(nee))


# name: light centre, light radius, mesh scale, mesh centre, the C2 surface (a sphere's centre and radius, or the z of a wall facing +z)
ORDERING_SCENES = {
    "sphere": ((6.0, 3.0, -2.0), 3.0, 0.4, (1.0, 0.5, -2.0), ((-3.0, -1.0, -2.0), 2.0)),
    "wall": ((4.0, 3.0, 0.0), 2.5, 0.8, (1.5, 1.0, -3.0), -5.0),
    "wall_centred": ((0.0, 4.0, 0.0), 2.0, 0.6, (0.0, 1.5, -3.0), -6.0),
}


def _ordering_scene(name):
    """ground plane, a light, a surface of the half-mirror half-diffuse C2 material beside it and a mesh between the two: from that
    surface some shadow rays cross the mesh's boxes (undecided) while the mirror ray of the same bounce passes them by and ends on the
    light.  The case is rare -- at 64 samples 2 rays of the sphere scene, 13 and 9 of the two wall scenes (counted as the difference of
    probe_resolved between this code and a build without the rule) -- and in the wall scenes that build's accumulator differs from
    the persistent kernel's, so these are the cases that hold the rule."""
    light_c, light_r, scale, mesh_c, surface = ORDERING_SCENES[name]
    v, i = standin_mesh(2)
    v = v.copy()
    v[:, :3] = v[:, :3] * np.float32(scale) + np.array(mesh_c, np.float32)
    mats = list(P.REFERENCE_MATERIALS) + [MAT_SPEC_DIFFUSE]
    c2 = ("sphere", surface[0], surface[1], 4) if isinstance(surface, tuple) else ("plane", (0, 0, 1), (0, 0, surface), 4)
    objs = [("plane", (0, 1, 0), (0, -3, 0), 1), ("sphere", light_c, light_r, 2), c2, ("mesh", v, i, 0, O.BUILD_SAH_INTERVALS)]
    return pair_from(objs, mats, [1], camera=((0, 0, 8), (0, 0, -1), 60.0, W / H))


def _render(s, kernel, spp, knobs=None, candidates=1):
    r = P.Renderer(0)
    try:
        if candidates != 1:
            r.set_nee_candidates(candidates)
        r.upload(s)
        if knobs:
            r.set_tuning(**knobs)
        r.reset_stats()
        r.render(W, H, spp, seed=SEED, kernel=kernel)
        st = r.stats()
        assert st.last_kernel == kernel
        return r.accumulator().copy(), r.pixels().copy(), st
    finally:
        r.close()


def _oracle_rays(o, spp):
    o.reset_accumulator(); o.reset_stats()
    o.render(W, H, spp, O.MODE_ADVANCED, O.DEBUG_NONE, O.RNG_PIXEL_PCG, SEED, nthreads=8)
    return o.stats().traced_rays


def _check(s, spp, knobs=None, candidates=1, o=None):
    """probe_lights 1 and 0 against the megakernel and the persistent kernel (and the oracle's ray count); returns probe_resolved of both"""
    ref_acc, ref_px, ref_st = _render(s, DEVICE_REFERENCES[0], spp, candidates=candidates)
    acc, px, st = _render(s, DEVICE_REFERENCES[1], spp, candidates=candidates)
    assert np.array_equal(_bits(acc), _bits(ref_acc)) and np.array_equal(px, ref_px) and st.traced_rays == ref_st.traced_rays
    assert ref_acc[..., :3].any()
    if o is not None:
        assert _oracle_rays(o, spp) == ref_st.traced_rays
    resolved = {}
    for lights in (1, 0):
        acc, px, st = _render(s, P.KERNEL_WAVEFRONT, spp, {**(knobs or {}), "probe_lights": lights}, candidates=candidates)
        assert np.array_equal(_bits(acc), _bits(ref_acc)), (lights, knobs)
        assert np.array_equal(px, ref_px), (lights, knobs)
        assert st.traced_rays == ref_st.traced_rays, (lights, knobs, st.traced_rays, ref_st.traced_rays)
        resolved[lights] = st.probe_resolved
    print(f"spp {spp} knobs {knobs} candidates {candidates}: probe_resolved {resolved[1]} with probe_lights 1, {resolved[0]} with 0, "
          f"of {ref_st.traced_rays} rays")
    return resolved


@pytest.mark.parametrize("spp", [5, 64, 96])
@pytest.mark.parametrize("nee", [True, False], ids=["nee", "no_nee"])
def test_bit_identity(nee, spp):
    """NEE off: every light hit adds energy (and there is no shadow ray); NEE on: after a diffuse bounce the path ends with nothing added"""
    o, s = _bench_like(nee)
    resolved = _check(s, spp, o=o)
    assert resolved[1] > resolved[0] > 0                             # (without NEE the bounce rays into the sky are still decided)


def test_four_nee_candidates():
    _, s = _bench_like(True)
    resolved = _check(s, 5, candidates=4)
    assert resolved[1] > resolved[0] > 0


@pytest.mark.parametrize("nee", [True, False], ids=["nee", "no_nee"])
def test_probe_off(nee):
    o, s = _bench_like(nee)
    assert _check(s, 5, {"probe": 0}, o=o) == {1: 0, 0: 0}


@pytest.mark.parametrize("knobs", [{"bands": 4, "bands_min_paths": 0, "batch": 4}, {"retire_misses": 0}, {"spec_dedupe": 0}, {"batch": 1}], ids=str)
def test_lists_and_election_knobs(knobs):
    _, s = _bench_like(True)
    resolved = _check(s, 9, knobs)
    assert resolved[1] > resolved[0] > 0


@pytest.mark.parametrize("nee", [True, False], ids=["nee", "no_nee"])
def test_the_new_path_is_exercised(nee):
    """a plane, a light sphere and no mesh: nothing is ever undecided (but a direction with a zero component), so every bounce ray that
    reaches the light ends in the pass that made it"""
    o, s = _plane_and_light(nee)
    resolved = _check(s, 64, o=o)
    assert resolved[1] > resolved[0]


@pytest.mark.parametrize("name", list(ORDERING_SCENES))
def test_ordering_rule(name):
    o, s = _ordering_scene(name)
    resolved = _check(s, 64, o=o)
    assert resolved[1] > resolved[0] > 0
