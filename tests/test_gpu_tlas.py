"""The top-level tree on the device (cgpt_set_top_level): mode 1 against mode 0 to the bit in all three render paths,
cgpt_intersect_rays against the numpy model of tests/tlas_ref.py, the boxes after every edit that moves one, and the state rules."""
import ctypes as C

import numpy as np
import pytest

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
from cpugpupathtracing_amd.scene import triangles_from_arrays
import tlas_ref as TL
import tlas_scenes as TS
import transform_ref as T

pytestmark = pytest.mark.gpu

KERNELS = (P.KERNEL_MEGAKERNEL, P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT)
W, H, SPP = 64, 48, 4
SAME_COUNTERS = ("traced_rays", "tri_tests", "bvh_depth_sum", "closest_hits")
MODES = {"ADVANCED": P.Settings(render_mode=P.MODE_ADVANCED), "BRUTE_FORCE": P.Settings(render_mode=P.MODE_BRUTE_FORCE),
         "COMPARISON": P.Settings(render_mode=P.MODE_COMPARISON),
         "BVH_DEPTH": P.Settings(render_mode=P.MODE_ADVANCED, debug_render_mode=P.DEBUG_BVH_DEPTH)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _frame(r, kernel, settings, counters=False, w=W, h=H, spp=SPP):
    r.reset_accumulator(); r.reset_stats()
    r.render(w, h, spp, kernel=kernel, settings=settings, counters=counters)
    return r.accumulator().copy(), r.pixels().copy(), r.stats()


def _plain(spec):
    return [dict(ob, transform=None) if "transform" in ob else dict(ob) for ob in spec]


_forty = {}


def forty():
    """The 40 objects of the CPU test as a scene, their model and rays: built once, never changed."""
    if not _forty:
        spec = TL.forty_objects()
        scene, model = TS.to_scene(spec, lamp=1)
        rays, axis = TS.all_rays(model)
        _forty.update(spec=spec, scene=scene, model=model, rays=rays, axis=axis)
    return _forty


# ---- 1. mode 1 equals mode 0 to the bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("transforms", [False, True], ids=["no_transforms", "transforms"])
@pytest.mark.parametrize("n_objects", [12, 40], ids=["object_table_in_lds", "object_table_in_hbm"])
def test_mode_1_equals_mode_0_to_the_bit(n_objects, transforms, M):
    """Accumulator, pixels, traced_rays and (with counters) tri_tests, bvh_depth_sum, closest_hits, in every kernel and mode.
    The scene has an infinite ground plane: a path that lands on it 10^4-10^6 units away sends its NEE shadow ray at the lamp from there, and
    from that distance the list walk's sphere test reports hits on spheres the ray passes far from.  The node test's own pad
    (tlas_ref.FAR_PAD) keeps the tree from skipping them; without it 1-2 of the 3072 pixels differ in 6 of the 8 cases."""
    spec = TL.forty_objects()[:n_objects]
    assert sum(ob.get("transform") is not None for ob in spec) >= 3
    scene, _ = TS.to_scene(spec if transforms else _plain(spec), lamp=1)
    r = P.Renderer(0)
    try:
        r.set_nee_candidates(M)
        r.upload(scene)
        differing = []
        for mode, st in MODES.items():
            for kernel in KERNELS:
                for counters in (False, True):
                    r.set_top_level(False)
                    acc0, px0, s0 = _frame(r, kernel, st, counters)
                    r.set_top_level(True)
                    acc1, px1, s1 = _frame(r, kernel, st, counters)
                    what = (n_objects, transforms, M, mode, kernel, counters)
                    assert s0.last_kernel == kernel and s1.last_kernel == kernel
                    assert (len(np.unique(px0)) > 2) if mode == "BVH_DEPTH" else acc0[..., :3].any(), what
                    if not (np.array_equal(_bits(acc0), _bits(acc1)) and np.array_equal(px0, px1)):
                        differing.append((mode, kernel, counters, int(((_bits(acc0) != _bits(acc1)).any(-1) | (px0 != px1)).sum())))
                    assert s0.traced_rays == s1.traced_rays, what
                    if counters:
                        assert [getattr(s0, c) for c in SAME_COUNTERS] == [getattr(s1, c) for c in SAME_COUNTERS], what
                        assert s0.tri_tests > 0 and 0 < s1.inner_steps < s0.inner_steps, what
                        assert s0.closest_hits > 0 or mode == "BVH_DEPTH", what  # the depth view shades no hit: the list walk counts none either
                    if kernel == P.KERNEL_WAVEFRONT:
                        assert s1.probe_resolved == 0, what                  # the shade-side probe walks the list: off with the tree
        print(f"{n_objects} objects, transforms {transforms}, M {M}: (mode, kernel, counters, differing pixels of {W * H}) = {differing}")
        assert not differing, differing
    finally:
        r.close(); scene.close()


# ---- 2. cgpt_intersect_rays: the modes against each other and against the model; inner_steps -----------------------------------------------------
def test_intersect_rays_equal_between_the_modes_and_equal_to_the_model():
    f = forty()
    (o, d, tmax), (ao, ad) = f["rays"], f["axis"]
    model = f["model"]
    r = P.Renderer(0)
    try:
        r.upload(f["scene"])
        for name, (ro, rd, rt) in {"random": (o, d, tmax), "axis": (ao, ad, None)}.items():
            want_t, want_obj, want_tri, want_depth, info_list = model.walk(ro, rd, rt, tree=False)
            _, _, _, _, info_tree = model.walk(ro, rd, rt, tree=True)
            r.set_top_level(False); r.reset_stats()
            t0, obj0, tri0, dep0 = r.intersect_rays(ro, rd, rt)
            list_inner, list_tris = r.stats().inner_steps, r.stats().tri_tests
            r.set_top_level(True); r.reset_stats()
            t1, obj1, tri1, dep1 = r.intersect_rays(ro, rd, rt)
            tree_inner, tree_tris = r.stats().inner_steps, r.stats().tri_tests
            assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(obj0, obj1) and np.array_equal(tri0, tri1) and np.array_equal(dep0, dep1), name
            differ = (_bits(t1) != _bits(want_t)) | (obj1 != want_obj) | (tri1 != want_tri) | (dep1 != want_depth)
            print(f"{name}: {int(differ.sum())} of {ro.shape[0]} rays differ from the model; inner steps list {list_inner} tree {tree_inner}, "
                  f"model {info_list['inner']} / {info_tree['inner']}, skipped inner-root meshes {info_tree['skipped_inner_roots']}")
            assert differ.sum() == 0, (name, np.nonzero(differ)[0][:8])
            # inner_steps counts mesh inner steps only: one fewer for every skipped mesh with an inner root
            assert list_inner == info_list["inner"] and tree_inner == info_tree["inner"], name
            assert list_tris == tree_tris == info_list["tris"], name
            if name == "random":
                assert tree_inner < list_inner and list_inner - tree_inner == info_tree["skipped_inner_roots"]
            else:
                assert tree_inner == list_inner                               # an axis-parallel ray skips nothing
    finally:
        r.close()


def test_shadow_rays_from_far_out_on_the_ground_plane_are_equal_between_the_modes():
    """tlas_ref.far_rays: the list walk's sphere test errs on them, and the tree must report what it reports (FAR_PAD)."""
    f = forty()
    o, d, tmax = TL.far_rays()
    r = P.Renderer(0)
    try:
        r.upload(f["scene"])
        r.set_top_level(False)
        a = r.intersect_rays(o, d, tmax)
        r.set_top_level(True)
        b = r.intersect_rays(o, d, tmax)
        differ = (_bits(a[0]) != _bits(b[0])) | (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3])
        spheres = [k for k, ob in enumerate(f["spec"]) if ob["kind"] == "sphere" and k != 1]
        print(f"far shadow rays: {int(differ.sum())} of {o.shape[0]} differ; {int(np.isin(a[1], spheres).sum())} report a sphere other than the lamp")
        assert differ.sum() == 0 and np.isin(a[1], spheres).sum() > 0
    finally:
        r.close()


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_same_quad_as_objects_3_and_17_is_reported_as_object_3():
    s = P.Scene()
    mat = s.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
    quad = TL.quad_mesh((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    for k in range(20):
        if k in (3, 17):
            mesh = P.Mesh.from_arrays(*quad)
            assert s.add_mesh(mesh, mat) == k
            mesh.close()
        else:
            s.add_sphere((6.0 + 2.5 * k, 5.0, -3.0), 0.5, mat)
    s.set_camera((0, 0, 5), (0, 0, -1), 60.0, 1.0)
    rng = np.random.default_rng(4)
    n = 512
    target = np.concatenate([rng.uniform(-0.95, 0.95, (n, 2)), np.zeros((n, 1))], 1)
    o = target + np.array([0.0, 0.0, 4.0]) + rng.uniform(-1.0, 1.0, (n, 3))
    d = target - o; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    r = P.Renderer(0)
    try:
        r.upload(s)
        for on in (False, True):
            r.set_top_level(on)
            t, obj, tri, _ = r.intersect_rays(o.astype(np.float32), d.astype(np.float32))
            assert np.all(obj == 3), (on, np.unique(obj))
    finally:
        r.close(); s.close()


# ---- 4. the boxes follow the edits -------------------------------------------------------------------------------------------------------------------
def _edit_scene():
    s = P.Scene()
    mat = s.add_material(P.Material(albedo=(0.8, 0.8, 0.8)))
    emitter = s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=20.0, is_light=True))
    s.add_plane((0.0, 1.0, 0.0), (0.0, -30.0, 0.0), mat)
    lamp = s.add_sphere((0.0, 20.0, 10.0), 2.0, emitter)
    s.add_light(lamp)
    ball = s.add_sphere((-6.0, 0.0, 0.0), 1.0, mat)
    box = s.add_mesh(P.Mesh.from_arrays(*TL.box_mesh((0.0, 0.0, 0.0), 1.0)), mat)            # moved by a transform
    crate = s.add_mesh(P.Mesh.from_arrays(*TL.box_mesh((6.0, 0.0, 0.0), 1.0)), mat)          # moved by a refit
    for k in range(6):
        s.add_sphere((-10.0 + 4.0 * k, -12.0, -6.0), 0.5, mat)
    s.set_camera((0.0, 4.0, 30.0), (0.0, -0.1, -1.0), 60.0, W / H)
    return s, ball, box, crate


def _rays_at(centre, n=256, seed=1):
    rng = np.random.default_rng(seed)
    target = np.asarray(centre, np.float64) + rng.uniform(-0.6, 0.6, (n, 3))
    o = np.array([0.0, 3.0, 25.0]) + rng.uniform(-2.0, 2.0, (n, 3))
    d = target - o; d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


OLD = {"ball": (-6.0, 0.0, 0.0), "box": (0.0, 0.0, 0.0), "crate": (6.0, 0.0, 0.0)}
NEW = {"ball": (-6.0, 9.0, 3.0), "box": (0.5, 9.0, -4.0), "crate": (7.0, -9.0, 2.0)}


def _edit(r, name, obj, n):
    """One edit: the sphere by cgpt_scene_update_primitive, the box by cgpt_scene_update_transforms, the crate by cgpt_scene_refit_mesh."""
    if name == "ball":
        r.update_primitive(obj, 0, center=NEW["ball"], radius=1.0)
    elif name == "box":
        m = np.tile(T.IDENTITY, (n, 1, 1)); m[obj] = T.affine(T.rotation((0.0, 1.0, 0.0), 0.4), NEW["box"])
        r.update_transforms(m)
    else:
        r.refit_mesh(obj, triangles_from_arrays(*TL.box_mesh(NEW["crate"], 1.0)))


def _apply_edits(r, ball, box, crate, n):
    for name, obj in (("ball", ball), ("box", box), ("crate", crate)):
        _edit(r, name, obj, n)


@pytest.mark.parametrize("edited", ["ball", "box", "crate"], ids=["update_primitive", "update_transforms", "refit_mesh"])
def test_each_edit_alone_rewrites_the_tree(edited):
    """A fresh context with the mode on and one edit: every edit rewrites the whole device tree, so only an edit on its own shows that
    it does.  The edited object is hit at its new place and missed at its old one; the other two stay where they were."""
    s, ball, box, crate = _edit_scene()
    ids = {"ball": ball, "box": box, "crate": crate}
    r = P.Renderer(0)
    try:
        r.set_top_level(True)
        r.upload(s)
        _check_places(r, ids, OLD, True)
        _edit(r, edited, ids[edited], s.flatten().n_objects)
        _check_places(r, {edited: ids[edited]}, NEW, True)
        _check_places(r, {edited: ids[edited]}, OLD, False)
        _check_places(r, {k: v for k, v in ids.items() if k != edited}, OLD, True)
        r.set_top_level(False)                                                 # and the list walk agrees
        _check_places(r, {edited: ids[edited]}, NEW, True)
    finally:
        r.close(); s.close()


def _check_places(r, ids, where, hit):
    for name, obj in ids.items():
        o, d = _rays_at(where[name])
        _, got, _, _ = r.intersect_rays(o, d)
        if hit:
            assert np.all(got == obj), (name, "new place", np.unique(got))
        else:
            assert np.all(got != obj), (name, "old place", np.unique(got))


def test_the_boxes_follow_the_edits_and_a_mode_turned_on_after_them_gives_the_same():
    s, ball, box, crate = _edit_scene()
    ids = {"ball": ball, "box": box, "crate": crate}
    n = s.flatten().n_objects
    before, after = P.Renderer(0), P.Renderer(0)
    try:
        before.set_top_level(True)                                  # the mode first, before a scene exists
        before.upload(s)
        _check_places(before, ids, OLD, True)
        _check_places(before, ids, NEW, False)
        _apply_edits(before, ball, box, crate, n)                   # every edit rewrites the tree: a stale box would hide the object
        _check_places(before, ids, NEW, True)
        _check_places(before, ids, OLD, False)
        after.upload(s)
        _apply_edits(after, ball, box, crate, n)                    # the edits in mode 0, the mode turned on afterwards
        frames = {}
        for name, r in (("list", after), ("before", before)):
            frames[name] = _frame(r, P.KERNEL_AUTO, MODES["ADVANCED"])
        after.set_top_level(True)
        assert after.top_level
        _check_places(after, ids, NEW, True)
        _check_places(after, ids, OLD, False)
        frames["after"] = _frame(after, P.KERNEL_AUTO, MODES["ADVANCED"])
        assert frames["list"][0][..., :3].any()
        for name in ("before", "after"):
            assert np.array_equal(_bits(frames[name][0]), _bits(frames["list"][0])), name
        o, d = _rays_at(NEW["box"], 512, seed=2)
        a, b = before.intersect_rays(o, d), after.intersect_rays(o, d)
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
    finally:
        before.close(); after.close(); s.close()


# ---- 5. mode semantics ---------------------------------------------------------------------------------------------------------------------------------
def test_setter_refusals_and_the_mode_survives_an_upload():
    f = forty()
    r = P.Renderer(0)
    L = r.L
    try:
        assert L.cgpt_set_top_level(r._ctx, 2) == N.CGPT_ERR_INVALID and b"neither 0" in L.cgpt_last_error(r._ctx)
        assert L.cgpt_set_top_level(r._ctx, 0xFFFFFFFF) == N.CGPT_ERR_INVALID
        assert not r.top_level
        r.upload(f["scene"])
        (o, d, tmax) = f["rays"]
        r.reset_stats(); r.intersect_rays(o[:1024], d[:1024]); list_inner = r.stats().inner_steps
        r.set_top_level(True)
        assert L.cgpt_set_top_level(r._ctx, 7) == N.CGPT_ERR_INVALID           # refused: nothing changed, the tree stays on
        r.reset_stats(); r.intersect_rays(o[:1024], d[:1024]); tree_inner = r.stats().inner_steps
        assert tree_inner < list_inner
        r.upload(f["scene"])                                                   # context state: the upload keeps it and rebuilds the tree
        r.reset_stats(); r.intersect_rays(o[:1024], d[:1024])
        assert r.stats().inner_steps == tree_inner
        r.set_top_level(False)
        r.reset_stats(); r.intersect_rays(o[:1024], d[:1024])
        assert r.stats().inner_steps == list_inner
    finally:
        r.close()


def test_guides_and_denoised_output_are_equal_between_the_modes():
    f = forty()
    a, b = P.Renderer(0), P.Renderer(0)
    try:
        b.set_top_level(True)
        out = []
        for r in (a, b):
            r.upload(f["scene"])
            r.render(W, H, SPP, settings=MODES["ADVANCED"])
            out.append((r.guides().copy(), r.denoise()))
        assert np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
        assert len(np.unique(out[0][0][..., 7].view(np.uint32))) > 8           # the guides see many objects
        assert np.array_equal(_bits(out[0][1][0]), _bits(out[1][1][0])) and np.array_equal(out[0][1][1], out[1][1][1])
        a.set_top_level(True)                                                  # the setter leaves the cached guides valid, and they are the same
        assert np.array_equal(_bits(a.guides()), _bits(out[0][0]))
    finally:
        a.close(); b.close()


def test_two_ranks_with_peer_copy_equal_one_device():
    f = forty()
    one = P.Renderer(0)
    g = P.Renderer([0, 0], flags=P.CTX_GATHER_PEER_COPY)
    try:
        one.upload(f["scene"])
        single = _frame(one, P.KERNEL_AUTO, MODES["ADVANCED"], w=48, h=40, spp=6)[0]
        g.set_top_level(True)                                                  # every member
        g.upload(f["scene"])
        assert g.L.cgpt_set_top_level(g._ctx, 3) == N.CGPT_ERR_INVALID
        both = _frame(g, P.KERNEL_AUTO, MODES["ADVANCED"], w=48, h=40, spp=6)[0]
        assert single[..., :3].any() and np.array_equal(_bits(both), _bits(single))
        (o, d, _) = f["rays"]
        a, b = one.intersect_rays(o[:512], d[:512]), g.intersect_rays(o[:512], d[:512])
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))
        g.set_top_level(False)
        assert np.array_equal(_bits(_frame(g, P.KERNEL_AUTO, MODES["ADVANCED"], w=48, h=40, spp=6)[0]), _bits(single))
    finally:
        one.close(); g.close()


# ---- 6. one and two objects ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_objects", [1, 2])
def test_one_and_two_objects(n_objects):
    s = P.Scene()
    emitter = s.add_material(P.Material(emissive=(1.0, 1.0, 1.0), intensity=5.0, is_light=True))
    mat = s.add_material(P.Material(albedo=(0.8, 0.6, 0.4)))
    lamp = s.add_sphere((0.0, 0.5, 0.0), 1.0, emitter)
    s.add_light(lamp)
    if n_objects == 2:
        mesh = P.Mesh.from_arrays(*TL.box_mesh((0.5, -2.0, 0.0), (2.0, 0.5, 2.0)))
        s.add_mesh(mesh, mat, transform=T.affine(T.rotation((0.0, 0.0, 1.0), 0.2), (0.0, 0.0, 0.0)))
        mesh.close()
    s.set_camera((0.0, 0.0, 7.0), (0.0, 0.0, -1.0), 60.0, W / H)
    r = P.Renderer(0)
    try:
        r.upload(s)
        assert s.top_level()[0].shape[0] == 2 * n_objects - 1
        for kernel in KERNELS:
            r.set_top_level(False)
            acc0, _, s0 = _frame(r, kernel, MODES["ADVANCED"], counters=True)
            r.set_top_level(True)
            acc1, _, s1 = _frame(r, kernel, MODES["ADVANCED"], counters=True)
            assert acc0[..., :3].any() and np.array_equal(_bits(acc0), _bits(acc1)), (n_objects, kernel)
            assert [getattr(s0, c) for c in SAME_COUNTERS] == [getattr(s1, c) for c in SAME_COUNTERS], (n_objects, kernel)
    finally:
        r.close(); s.close()
