"""One context walked up and down the lobe ladder by edits alone (csrc/device/kernel_variant.h): 0 a fresh upload, 1 update_roughness,
2 update_transmission_roughness, 3 update_smooth_normals, 4 update_transforms, then each edit undone in reverse order with zeros and
identity matrices (LayoutTransforms stores the flag 0 for an identity matrix, so the undo needs no re-upload).  At every step the frame is
rendered by each of the three kernels, through the object list and the top-level tree, with 1 and 4 NEE candidates: every instantiation
the variant choice can name is launched, and the choice made after an edit is the one a fresh context of that level would make.

Everything is byte equality -- across the kernels (RenderEnqueue: "all three kernels give bit-identical images"), across the tree
(cgpt_set_top_level: "the image does not depend on it"), across the counting kernels and between the way up and the way down -- except the
last test: cgpt_shade_samples on a second context walked up the same ladder, against the float64 model at that level, by the comparison
rule of test_gpu_shade_step.py (its _check, not restated here).  That context holds the scene of shade_cases.py, whose samples name its
objects; the probe and the render choose their variant by the same function, which is what the test pins."""
import copy

import numpy as np
import pytest

import cpugpupathtracing_amd as P
import shade_cases as CASES
import shade_ref as S
import test_gpu_shade_step as STEP
import transform_ref as TR
from scenes import reference_layout_pair, standin_mesh

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 32, 24, 4, 0x13579BDF
GLASS = 3
KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_PERSISTENT, P.KERNEL_WAVEFRONT)
TREES, CANDIDATES = (0, 1), (1, 4)
ADVANCED = P.Settings(max_ray_depth=5, next_event_estimation_enabled=True, cosine_weighted_diffuse_reflection_enabled=True,
                      russian_roulette_enabled=True)
COMPARISON = P.Settings(max_ray_depth=5, next_event_estimation_enabled=True, cosine_weighted_diffuse_reflection_enabled=True,
                        russian_roulette_enabled=True, render_mode=P.MODE_COMPARISON)
ROUGHNESS, TRANSMISSION_ROUGHNESS = 0.3, 0.2
MOVED = TR.affine(TR.rotation((0.3, 1.0, -0.2), 0.7) @ np.diag([1.25, 0.75, 1.0]), (0.4, -0.3, 0.2))   # of the mesh: no identity
# of the quad of shade_cases.py: a turn in its own plane about the point its samples hit, so that they still are hits of the mesh
SPUN = TR.affine(TR.rotation((0, 0, 1), 0.7), np.array([0.5, 0.5, 0.0]) - TR.rotation((0, 0, 1), 0.7) @ np.array([0.5, 0.5, 0.0]))
N_OBJECTS, MESH = 4, 0                     # the layout of tests/scenes.py: the mesh, the ground quad, two sphere lights
N_MATERIALS = len(P.REFERENCE_MATERIALS)


def _matrices(n, k, m):
    out = np.tile(np.asarray(TR.IDENTITY, np.float32).reshape(1, 3, 4), (n, 1, 1))
    out[k] = np.asarray(m, np.float32).reshape(3, 4)
    return out


def _flags(n, k, value):
    out = np.zeros(n, np.uint32)
    out[k] = value
    return out


def _edits(n_objects, n_materials, mesh, moved=MOVED):
    """(level after the edit, the edit) on the way up, then on the way down."""
    ident = np.asarray(TR.IDENTITY, np.float32)
    up = [(1, lambda r: r.update_roughness(np.full(n_materials, ROUGHNESS, np.float32))),
          (2, lambda r: r.update_transmission_roughness(np.full(n_materials, TRANSMISSION_ROUGHNESS, np.float32))),
          (3, lambda r: r.update_smooth_normals(_flags(n_objects, mesh, 1))),
          (4, lambda r: r.update_transforms(_matrices(n_objects, mesh, moved)))]
    down = [(3, lambda r: r.update_transforms(_matrices(n_objects, mesh, ident))),
            (2, lambda r: r.update_smooth_normals(_flags(n_objects, mesh, 0))),
            (1, lambda r: r.update_transmission_roughness(np.zeros(n_materials, np.float32))),
            (0, lambda r: r.update_roughness(np.zeros(n_materials, np.float32)))]
    return up, down


def _frames(r, settings=ADVANCED, counters=False):
    """{(kernel, tree, candidates): accumulator} of the context as it is."""
    out = {}
    for m in CANDIDATES:
        r.set_nee_candidates(m)
        for tree in TREES:
            r.set_top_level(bool(tree))
            for kernel in KERNELS:
                r.reset_accumulator()
                r.render(W, H, SPP, seed=SEED, kernel=kernel, settings=settings, counters=counters)
                out[kernel, tree, m] = r.accumulator().copy()
    return out


@pytest.fixture(scope="module")
def walk():
    """Every frame of the walk, rendered once: up[level], counted[level], down[level] (levels 3..0) and the COMPARISON frames at level 4."""
    _, s = reference_layout_pair(*standin_mesh(0), GLASS, aspect=W / H, settings=ADVANCED)
    edits_up, edits_down = _edits(N_OBJECTS, N_MATERIALS, MESH)
    r = P.Renderer(0)
    try:
        r.upload(s)
        up, counted, down = {0: _frames(r)}, {0: _frames(r, counters=True)}, {}
        for level, edit in edits_up:
            edit(r)
            up[level] = _frames(r)
            counted[level] = _frames(r, counters=True)
        comparison = _frames(r, COMPARISON), _frames(r, COMPARISON, counters=True)
        for level, edit in edits_down:
            edit(r)
            down[level] = _frames(r)
    finally:
        r.close()
    return dict(up=up, counted=counted, down=down, comparison=comparison)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_one_image_per_candidate_count(frames, what):
    for a in frames.values():
        assert np.isfinite(a).all(), what
    for m in CANDIDATES:
        ref = frames[KERNELS[0], 0, m]
        assert ref[..., :3].any(), (what, m)
        for kernel in KERNELS:
            for tree in TREES:
                assert np.array_equal(_bits(frames[kernel, tree, m]), _bits(ref)), (what, "kernel", kernel, "tree", tree, "candidates", m)


def _assert_same_frames(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (what, key)


def test_every_step_gives_one_image_in_all_kernels_and_through_the_tree(walk):
    assert sorted(walk["up"]) == [0, 1, 2, 3, 4] and sorted(walk["down"]) == [0, 1, 2, 3]
    for way in ("up", "down"):
        for level, frames in walk[way].items():
            assert len(frames) == len(KERNELS) * len(TREES) * len(CANDIDATES)
            _assert_one_image_per_candidate_count(frames, (way, level))


def test_comparison_mode_at_the_top_level_indexes_the_brute_tables(walk):
    plain, counted = walk["comparison"]
    _assert_one_image_per_candidate_count(plain, "COMPARISON")
    _assert_same_frames(plain, counted, "COMPARISON, counters")


def test_undoing_the_edits_gives_back_each_level_s_image(walk):
    for level, frames in walk["down"].items():
        _assert_same_frames(frames, walk["up"][level], ("level", level, "after the undo"))
    _assert_same_frames(walk["down"][0], walk["up"][0], "the last frame against the first")


def test_the_counting_kernels_give_the_same_image(walk):
    for level, frames in walk["counted"].items():
        _assert_same_frames(frames, walk["up"][level], ("level", level, "counters"))


def test_the_shade_probe_chooses_as_the_render_does_at_every_level():
    sc, _, objs = CASES._reference_scene()
    base = CASES._reference_samples(objs)
    smp = base[np.linspace(0, base.shape[0] - 1, 64).astype(np.int64)].copy()   # every object kind and material of the case, the mesh included
    assert np.unique(smp["obj"]).size > 8 and np.any(smp["obj"] == objs["mesh"])
    n_obj, n_mat, mesh = len(sc.objects), len(sc.materials), objs["mesh"]
    edits_up, _ = _edits(n_obj, n_mat, mesh, SPUN)
    model = [(0, lambda m: None),
             (1, lambda m: [mat.update(roughness=ROUGHNESS) for mat in m.materials]),
             (2, lambda m: [mat.update(transmission_roughness=TRANSMISSION_ROUGHNESS) for mat in m.materials]),
             (3, lambda m: m.objects[mesh].update(smooth=True)),
             (4, lambda m: m.objects[mesh].update(transform=np.asarray(SPUN, np.float32).reshape(3, 4)))]
    st = S.settings()
    r = P.Renderer(0)
    try:
        r.upload(sc.device_scene())
        for (level, model_edit), device_edit in zip(model, [None] + [e for _, e in edits_up]):
            if device_edit:
                device_edit(r)
            model_edit(sc)
            assert sc.lobe_level() == level
            for m in ((1, 4) if level == 4 else (1,)):
                r.set_nee_candidates(m)
                c = CASES.call(f"variant_ladder_level{level}_M{m}", copy.deepcopy(sc), st, smp, m)
                STEP._device[c["name"], None] = r.shade_samples(smp, S.device_settings(st))   # what STEP._run would hand to STEP._check
                STEP._check(c)
    finally:
        r.close()
