"""The production traversal -- wf_trace's voted steps, LDS stack with HBM overflow, object table, tree-top mirror, triangle cache, any-hit
exit and round 0's lean walk -- held to the oracle record by record through the trace probe (cgpt_trace_rays, cgpt_trace_first_hits;
DESIGN.md 5.22).  The ray sets are tests/trace_cases.py's; tests/test_trace_cases.py shows on the CPU that each does what it is for.

Everything is equality.  Per extend ray t (as uint32 words), obj, tri where hit and bvh_depth equal the oracle's (oracle.intersect_rays,
pinned by test_oracle_pins.py) and cgpt_intersect_rays's, in both list orders, with and without the counting kernels and for every knob
value below; where the oracle has no statement (transforms, the top-level tree) cgpt_intersect_rays alone is the reference.  One field is
not there to compare: with the retire_misses knob at 1 (the default) wf_trace stores no record for an extend ray that misses, so the
probe returns such a ray's bvh_depth as 0; it is compared with 0 there and with the oracle's count in every run with retire_misses = 0.
Per shadow ray the occluded byte equals `oracle obj != ~0u` for the same tmax."""
import ctypes as C

import numpy as np
import pytest
import torch

import cpugpupathtracing_amd as P
from cpugpupathtracing_amd import _native as N
import replay_ref as RP
import shade_ref as S
import tlas_ref as TL
import tlas_scenes as TS
import trace_cases as TC
import transform_ref as TR
import transform_scenes as XS

pytestmark = pytest.mark.gpu

NO_HIT = TC.NO_HIT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _counters(st):
    return (st.traced_rays, st.inner_steps, st.tri_tests, st.bvh_depth_sum)


@pytest.fixture(scope="module")
def renderer():
    r = P.Renderer(0)
    yield r
    r.close()


@pytest.fixture
def fresh():
    """A context of its own, for the tests that turn knobs."""
    r = P.Renderer(0)
    yield r
    r.close()


def _same_records(got, want, what, miss_depth=True, tri_free=None):
    """(t, obj, tri, bvh_depth) against (t, obj, tri, bvh_depth); miss_depth False: a miss's bvh_depth must be 0 (retire_misses = 1);
    tri_free: per ray, True where a hit's tri is not compared (default: compared on every hit)."""
    t, obj, tri, dep = (np.asarray(a) for a in got[:4])
    wt, wobj, wtri, wdep = want
    assert np.array_equal(obj, wobj), (what, "obj", np.nonzero(obj != wobj)[0][:8].tolist())
    assert np.array_equal(_bits(t), _bits(wt)), (what, "t", np.nonzero(_bits(t) != _bits(wt))[0][:8].tolist())
    hit = wobj != NO_HIT
    with_tri = hit if tri_free is None else hit & ~tri_free
    assert np.array_equal(tri[with_tri], wtri[with_tri]), (what, "tri", np.nonzero(with_tri & (tri != wtri))[0][:8].tolist())
    assert np.array_equal(dep[hit], wdep[hit]), (what, "bvh_depth of the hits", np.nonzero(hit & (dep != wdep))[0][:8].tolist())
    if miss_depth:
        assert np.array_equal(dep[~hit], wdep[~hit]), (what, "bvh_depth of the misses", np.nonzero(~hit & (dep != wdep))[0][:8].tolist())
    else:
        assert not dep[~hit].any(), (what, "bvh_depth of a retired miss")


def _full(rays):
    return rays if len(rays) == 3 else (rays[0], rays[1], None)


def _check(r, orc, ext, sh, what, retire=True, tri_free=None):
    """Four launches of ext extend and sh shadow rays -- both list orders, plain and counting kernels -- against the oracle (orc None: cgpt_intersect_rays alone)
    and cgpt_intersect_rays, records and counters.  Returns (hits, occluded)."""
    eo, ed, et = _full(ext) if ext is not None else (None, None, None)
    so, sd, st = _full(sh) if sh is not None else (None, None, None)
    n_ext = 0 if eo is None else eo.shape[0]
    n_sh = 0 if so is None else so.shape[0]
    r.reset_stats()
    want = r.intersect_rays(eo, ed, et) if n_ext else None
    want_sh = r.intersect_rays(so, sd, st) if n_sh else None
    want_counters = _counters(r.stats())
    if orc is not None:
        orc.reset_stats()
        if n_ext:
            _same_records(want, orc.intersect_rays(eo, ed, et), (what, "cgpt_intersect_rays against the oracle"))
        if n_sh:
            _same_records(want_sh, orc.intersect_rays(so, sd, st), (what, "cgpt_intersect_rays against the oracle, shadow rays"))
        assert _counters(orc.stats()) == want_counters, (what, "counters of cgpt_intersect_rays against the oracle's")
    occluded = (want_sh[1] != NO_HIT) if n_sh else np.zeros(0, bool)
    for reverse in (False, True):
        for count in (False, True):
            tag = (what, "reversed" if reverse else "identity", "counting" if count else "plain")
            r.reset_stats()
            got = r.trace_rays(eo, ed, et, so, sd, st, counters=count, reverse=reverse)
            stats = r.stats()
            if n_ext:
                _same_records(got, want, tag, miss_depth=not retire, tri_free=None if tri_free is None else tri_free(want[1]))
            assert np.array_equal(got[4] != 0, occluded), (tag, "occluded", np.nonzero((got[4] != 0) != occluded)[0][:8].tolist())
            assert set(np.unique(got[4]).tolist()) <= {0, 1}
            if count:
                assert _counters(stats) == want_counters, (tag, "counters", _counters(stats), want_counters)
            else:
                assert stats.traced_rays == n_ext + n_sh and (stats.inner_steps, stats.tri_tests, stats.bvh_depth_sum) == (0, 0, 0), tag
            assert stats.kernel_launches == 0
    return (0 if want is None else int((want[1] != NO_HIT).sum())), int(occluded.sum())


def _parity_shadow(level, n=4000):
    """Shadow rays cut from the parity set: a third with tmax 1e34, a third with a tmax around the hit, the NEE rays behind them."""
    o, d = TC.parity_rays()
    t, obj, _, _ = TC.parity_hits(level)
    tm = np.full(n, TC.T_FAR, np.float32)
    k = np.arange(n)
    near = (k % 3 == 1) & (obj[:n] != NO_HIT)
    tm[near] = (t[:n][near] * np.where(k[near] % 2 == 0, np.float32(0.5), np.float32(1.5))).astype(np.float32)
    no, nd, nt = TC.nee_shadow_rays(level)
    return np.concatenate([o[:n], no]), np.concatenate([d[:n], nd]), np.concatenate([tm, nt])


# ---- parity, zero components, tmax edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 4])
def test_parity_rays_and_zero_components(renderer, level):
    orc, s = TC.parity_pair(level)
    renderer.upload(s)
    o, d = TC.parity_rays()
    zo, zd = TC.zero_component_rays(level)
    hits, occluded = _check(renderer, orc, (np.concatenate([o, zo]), np.concatenate([d, zd])), _parity_shadow(level), ("parity", level))
    print(f"level {level}: {o.shape[0] + zo.shape[0]} extend rays, {hits} hits; {4000 + 1500} shadow rays, {occluded} occluded")
    assert hits > 5000 and 500 < occluded < 5000


@pytest.mark.parametrize("level", [2, 4])
def test_tmax_one_float_either_side_of_a_hit(renderer, level):
    orc, s = TC.parity_pair(level)
    renderer.upload(s)
    edges = TC.tmax_edge_rays(level)
    hits, occluded = _check(renderer, orc, edges, edges, ("tmax edges", level))
    n = edges[0].shape[0] // 5
    print(f"level {level}: {5 * n} extend and {5 * n} shadow rays, {hits} hits, {occluded} occluded")
    assert hits == occluded and 2 * n - 5 <= hits <= 2 * n                      # the float above t and 1e34 hit; t, the float below and t / 2 do not


# ---- list edges --------------------------------------------------------------------------------------------------------------------------------------
def test_list_lengths_around_a_wave(renderer):
    orc, s = TC.parity_pair(2)
    renderer.upload(s)
    o, d = TC.parity_rays()
    so, sd, st = _parity_shadow(2)
    for n_ext in TC.LIST_EXTEND:
        for n_sh in TC.LIST_SHADOW:
            a = 6 + 7 * n_sh                                                   # another cut of the set for every pair
            ext = (o[a:a + n_ext], d[a:a + n_ext])
            sh = (so[a:a + n_sh], sd[a:a + n_sh], st[a:a + n_sh]) if n_sh else None
            _check(renderer, orc, ext, sh, ("list", n_ext, n_sh))
    for n_sh in (1, 65):                                                       # shadow rays alone: the extend part of the list is empty
        _check(renderer, orc, None, (so[:n_sh], sd[:n_sh], st[:n_sh]), ("list", 0, n_sh))


# ---- several blocks per wave, with the knobs that change when a wave refills and how it votes -------------------------------------------------
@pytest.mark.parametrize("knobs", [dict(refill=1, inner_repeat=1, leaf_repeat=1, obj_shift=0), dict(refill=64, inner_repeat=65, leaf_repeat=65, obj_shift=6),
                                   dict(refill=1, inner_repeat=65, leaf_repeat=1, obj_shift=6), dict(refill=64, inner_repeat=1, leaf_repeat=65, obj_shift=0)])
def test_a_wave_fetches_several_blocks_and_refills_mid_walk(fresh, knobs):
    orc, s = TC.parity_pair(2)
    fresh.upload(s)
    fresh.set_tuning(trace_blocks=1, **knobs)
    n = TC.rays_beyond_one_block_per_wave(torch.cuda.get_device_properties(0).multi_processor_count)
    o, d = TC.tiled(*TC.parity_rays(), n)
    so, sd, st = _parity_shadow(2)
    hits, occluded = _check(fresh, orc, (o, d), (so, sd, st), ("blocks", tuple(knobs.items())))
    print(f"{knobs}: {n} extend rays, {hits} hits, {occluded} of {so.shape[0]} shadow rays occluded")
    assert hits > n // 4


# ---- knobs that change the walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [dict(lds_tris=0), dict(top_records=0), dict(shadow_any_hit=0), dict(retire_misses=0),
                                   dict(lds_tris=0, top_records=0, shadow_any_hit=0, retire_misses=0), dict(lds_tris=1, top_records=127, shadow_any_hit=1, retire_misses=1)])
def test_knobs_that_change_the_walk(fresh, knobs):
    orc, s = TC.parity_pair(2)
    fresh.upload(s)
    fresh.set_tuning(**knobs)
    hits, _ = _check(fresh, orc, TC.parity_rays(), _parity_shadow(2), ("knobs", tuple(knobs.items())), retire=bool(knobs.get("retire_misses", 1)))
    assert hits > 5000


# ---- deep stack ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("retire", [1, 0])
def test_stack_deeper_than_the_lds_levels(fresh, retire):
    orc, s = TC.deep_pair()
    fresh.upload(s)
    fresh.set_tuning(retire_misses=retire)
    o, d = TC.deep_rays()
    far = np.full(o.shape[0], 2000.0, np.float32)
    hits, occluded = _check(fresh, orc, (o, d), (o, d, far), ("deep stack", retire), retire=bool(retire))
    assert hits >= 200 and occluded >= 200


# ---- more objects than the LDS table, and ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["forty", "twin_quads", "coincident"])
@pytest.mark.parametrize("retire", [1, 0])
def test_object_list_beyond_the_lds_table_and_ties(fresh, case, retire):
    (orc, s), (o, d) = {"forty": (TC.forty_pair(), TC.forty_rays()), "twin_quads": (TC.twin_quad_pair(), TC.twin_quad_rays()),
                        "coincident": (TC.coincident_pair(), TC.coincident_rays())}[case]
    fresh.upload(s)
    fresh.set_tuning(retire_misses=retire)
    tm = np.full(o.shape[0], 30.0, np.float32)
    hits, occluded = _check(fresh, orc, (o, d), (o, d, tm), (case, retire), retire=bool(retire))
    t, obj, tri, _, _ = fresh.trace_rays(o, d)
    if case == "twin_quads":
        assert hits == o.shape[0] and np.all(obj == 3)                         # never 17: strict t <, first in visiting order
    if case == "coincident":
        assert (obj == 0).sum() >= 50 and np.all(tri[obj == 0] == orc.intersect_rays(o, d)[2][obj == 0])
    assert hits > 0 and occluded > 0


# ---- XFORM and TREE ----------------------------------------------------------------------------------------------------------------------------------
def _meets_a_triangle_object(spec, o, d, tmax):
    """Per ray: does it cross a stand-alone triangle object of `spec` below its tmax (tlas_ref's float32 triangle test, in the object's
    space)?  Every ray whose walk can have taken a hit from one is among them."""
    o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
    t = np.full(o.shape[0], 1e34, np.float32) if tmax is None else np.asarray(tmax, np.float32)
    met = np.zeros(o.shape[0], bool)
    for ob in spec:
        if ob["kind"] != "triangle":
            continue
        oo, od = o, d
        m = ob.get("transform")
        if m is not None and not TR.is_identity(m):
            oo, od = TR.ray_to_object(TR.invert(m), o, d)
        p = np.asarray(ob["positions"], np.float32).reshape(3, 3)
        met |= TL.hit_triangle(p[0], (p[1] - p[0]).astype(np.float32), (p[2] - p[0]).astype(np.float32), oo, od, t)[0]
    return met


def _plain(spec):
    return [dict(ob, transform=None) if "transform" in ob else dict(ob) for ob in spec]


@pytest.mark.parametrize("case", ["xform", "tree", "xform_tree"])
def test_transformed_objects_and_the_top_level_tree(fresh, case):
    """No oracle statement here: cgpt_intersect_rays (test_gpu_transforms.py, test_gpu_tlas.py hold it to theirs) is the reference.
    The 40 objects of tlas_ref hold stand-alone triangle objects, whose hits carry no triangle index: intersect_scene leaves the payload's
    tri as an earlier mesh wrote it, leaf_step writes the object's leaf record's (0), and no reader of a hit record looks at either (the
    ABI: "a triangle object ignores tri").  So on a ray that crosses a triangle object the tri of a final hit on anything but a mesh is
    not compared; every mesh hit's is, and so is the stale tri of every sphere, plane and triangle hit on the rays that cross none."""
    spec = None
    if case == "xform":
        scene, meshes = XS.box_world()
        a = TR.rotation((0.3, 1.0, -0.2), 0.7) @ np.diag([1.2, 0.8, 1.0])
        scene.set_transform(meshes[1], TR.affine(a, (0.3, 0.4, -0.2)))
        rng = np.random.default_rng(17)
        n = 4096
        o = (np.array([0.37, 2.3, 5.9]) + rng.normal(0, 0.5, (n, 3))).astype(np.float32)
        d = rng.uniform(-2.2, 2.2, (n, 3)) - o
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        tmax = np.full(n, 1e34, np.float32); tmax[::4] = rng.uniform(4.0, 9.0, tmax[::4].size).astype(np.float32)
        zo = zd = None
    else:
        spec = TL.forty_objects()
        scene, _ = TS.to_scene(spec if case == "xform_tree" else _plain(spec), lamp=1)
        assert sum(ob["kind"] == "mesh" for ob in spec) == 20 and sum(ob["kind"] == "triangle" for ob in spec) == 8
        o, d, tmax = TL.random_rays()
        zo, zd = TL.axis_rays()
    try:
        fresh.set_top_level(case != "xform")
        fresh.upload(scene)
        def tri_free_of(oo, dd, tm):
            if spec is None:
                return None
            met = _meets_a_triangle_object(spec if case == "xform_tree" else _plain(spec), oo, dd, tm)
            mesh = np.array([ob["kind"] == "mesh" for ob in spec] + [False])
            print(f"{case}: {int(met.sum())} of {met.size} rays cross a triangle object")
            assert met.sum() < met.size // 8
            return lambda obj: met & ~mesh[np.minimum(obj, len(spec))]
        hits, occluded = _check(fresh, None, (o, d, tmax), (o, d, tmax), (case,), tri_free=tri_free_of(o, d, tmax))
        assert hits > o.shape[0] // 8 and occluded == hits
        if zo is not None:
            hits, _ = _check(fresh, None, (zo, zd), (zo, zd), (case, "zero components"), tri_free=tri_free_of(zo, zd, None))
            assert hits > 0
    finally:
        scene.close()


# ---- round 0 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_lean", [1, 0])
@pytest.mark.parametrize("view", [0, 1])
def test_round0_records_equal_the_oracle_primary_hits(fresh, view, first_lean):
    _, s = TC.round0_pair()
    fresh.upload(s)
    fresh.set_tuning(first_lean=first_lean)
    for W, H, rows in TC.ROUND0_FRAMES:
        want = TC.round0_want(view, W, H, rows)
        wobj, wtri, wdep, wt = want["records"]
        for count in (False, True):
            what = ("round 0", view, first_lean, W, H, rows, "counting" if count else "plain")
            fresh.reset_stats()
            obj, tri, dep, t = fresh.trace_first_hits(W, H, rows=rows, camera=want["camera"], counters=count)
            stats = fresh.stats()
            assert obj.shape == wobj.shape
            _same_records((t.ravel(), obj.ravel(), tri.ravel(), dep.ravel()), (wt.ravel(), wobj.ravel(), wtri.ravel(), wdep.ravel()), what)
            assert stats.traced_rays == wobj.size and stats.kernel_launches == 0, what
            if count:
                assert _counters(stats) == want["counters"], what
            else:
                assert (stats.inner_steps, stats.tri_tests, stats.bvh_depth_sum) == (0, 0, 0), what


# ---- no side effects ---------------------------------------------------------------------------------------------------------------------------------
def _render_state(r, W, H, spp, kernel):
    r.reset_accumulator(); r.reset_stats()
    r.render(W, H, spp, seed=77, kernel=kernel)
    st = r.stats()
    return r.accumulator().copy(), r.pixels().copy(), (st.traced_rays, st.probe_resolved, st.kernel_launches, st.num_accumulated)


@pytest.mark.parametrize("kernel", [P.KERNEL_WAVEFRONT, P.KERNEL_PERSISTENT])
def test_a_render_after_the_probe_is_the_render_without_it(fresh, kernel):
    _, s = TC.parity_pair(2)
    fresh.upload(s)
    W, H, spp = 45, 37, 6
    _render_state(fresh, W, H, spp, kernel)                                    # the pools are allocated
    acc0, px0, st0 = _render_state(fresh, W, H, spp, kernel)
    held = fresh.L.cgpt_debug_live_device_bytes()
    fresh.reset_accumulator(); fresh.reset_stats()
    fresh.render(W, H, 2, seed=77, kernel=kernel)                              # an accumulator in progress
    mid_acc, mid_px, mid_n = fresh.accumulator().copy(), fresh.pixels().copy(), fresh.stats().num_accumulated
    o, d = TC.parity_rays()
    for count in (False, True):
        fresh.trace_rays(o[:3000], d[:3000], None, o[3000:4000], d[3000:4000], None, counters=count, reverse=count)
        fresh.trace_first_hits(W, H, rows=(5, 30), counters=count)
    assert fresh.L.cgpt_debug_live_device_bytes() == held                      # the probe's buffers are gone, the render's pools are kept
    assert np.array_equal(_bits(fresh.accumulator()), _bits(mid_acc)) and np.array_equal(fresh.pixels(), mid_px) and fresh.stats().num_accumulated == mid_n
    acc1, px1, st1 = _render_state(fresh, W, H, spp, kernel)
    assert np.array_equal(_bits(acc0), _bits(acc1)) and np.array_equal(px0, px1)
    assert st0 == st1, (st0, st1)
    assert fresh.L.cgpt_debug_live_device_bytes() == held


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    o, d = TC.parity_rays()
    o, d = np.ascontiguousarray(o[:64]), np.ascontiguousarray(d[:64])
    t = np.zeros(64, np.float32); obj = np.zeros(64, np.uint32); tri = np.zeros(64, np.uint32); dep = np.zeros(64, np.uint32); occ = np.zeros(64, np.uint8)
    of, df = o.ctypes.data_as(fp), d.ctypes.data_as(fp)
    outs = (t.ctypes.data_as(fp), obj.ctypes.data_as(up), tri.ctypes.data_as(up), dep.ctypes.data_as(up), occ.ctypes.data_as(bp))
    r = P.Renderer(0)
    try:
        L, ctx = r.L, r._ctx
        cam = N.Camera()
        assert L.cgpt_trace_rays(ctx, of, df, None, 64, of, df, None, 64, 0, *outs) == N.CGPT_ERR_NO_SCENE
        assert L.cgpt_trace_first_hits(ctx, C.byref(cam), 8, 8, 0, 8, 0, outs[1], outs[2], outs[3], outs[0]) == N.CGPT_ERR_NO_SCENE
        _, s = TC.parity_pair(2)
        r.upload(s)
        cam = s.camera()
        acc0, px0, st0 = _render_state(r, 45, 37, 3, P.KERNEL_WAVEFRONT)
        r.reset_stats()
        invalid = [
            lambda: L.cgpt_trace_rays(ctx, None, df, None, 64, None, None, None, 0, 0, *outs),
            lambda: L.cgpt_trace_rays(ctx, of, None, None, 64, None, None, None, 0, 0, *outs),
            lambda: L.cgpt_trace_rays(ctx, of, df, None, 64, None, None, None, 0, 0, None, outs[1], outs[2], outs[3], outs[4]),
            lambda: L.cgpt_trace_rays(ctx, of, df, None, 64, None, None, None, 0, 0, outs[0], outs[1], outs[2], None, outs[4]),
            lambda: L.cgpt_trace_rays(ctx, None, None, None, 0, of, None, None, 64, 0, *outs),
            lambda: L.cgpt_trace_rays(ctx, None, None, None, 0, of, df, None, 64, 0, outs[0], outs[1], outs[2], outs[3], None),
            lambda: L.cgpt_trace_rays(ctx, of, df, None, (1 << 22) + 1, None, None, None, 0, 0, *outs),
            lambda: L.cgpt_trace_rays(ctx, None, None, None, 0, of, df, None, (1 << 22) + 1, 0, *outs),
            lambda: L.cgpt_trace_rays(ctx, of, df, None, 64, None, None, None, 0, 4, *outs),
            lambda: L.cgpt_trace_first_hits(ctx, None, 8, 8, 0, 8, 0, outs[1], outs[2], outs[3], outs[0]),
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 8, 8, 0, 8, 0, outs[1], outs[2], outs[3], None),
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 0, 8, 0, 8, 0, outs[1], outs[2], outs[3], outs[0]),
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 8, 8, 4, 4, 0, outs[1], outs[2], outs[3], outs[0]),
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 8, 8, 0, 9, 0, outs[1], outs[2], outs[3], outs[0]),
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 4096, 2048, 0, 2048, 0, outs[1], outs[2], outs[3], outs[0]),   # 8 Mi pixels
            lambda: L.cgpt_trace_first_hits(ctx, C.byref(cam), 8, 8, 0, 8, N.TRACE_REVERSED, outs[1], outs[2], outs[3], outs[0]),
        ]
        for k, call in enumerate(invalid):
            assert call() == N.CGPT_ERR_INVALID, k
            assert L.cgpt_last_error(ctx)
        # no ray: CGPT_OK, nothing launched, whatever the pointers
        assert L.cgpt_trace_rays(ctx, None, None, None, 0, None, None, None, 0, 0, None, None, None, None, None) == N.CGPT_OK
        st = r.stats()
        assert (st.traced_rays, st.kernel_launches) == (0, 0)
        assert not t.any() and not obj.any() and not occ.any()                 # no refused call wrote a result
        acc1, px1, st1 = _render_state(r, 45, 37, 3, P.KERNEL_WAVEFRONT)
        assert np.array_equal(_bits(acc0), _bits(acc1)) and np.array_equal(px0, px1) and st0 == st1
        # and the context still probes
        got = r.trace_rays(o, d)
        _same_records(got, TC.parity_pair(2)[0].intersect_rays(o, d), "after the refusals", miss_depth=False)
    finally:
        r.close()


def test_a_multi_device_context_is_refused():
    g = P.Renderer(0, flags=N.CTX_FORCE_COLLECTIVE)
    try:
        _, s = TC.parity_pair(2)
        g.upload(s)
        g.render(16, 16, 2, seed=3)
        acc0 = g.accumulator().copy()
        o, d = TC.parity_rays()
        with pytest.raises(P.DeviceError) as e:
            g.trace_rays(o[:64], d[:64])
        assert e.value.code == N.CGPT_ERR_UNSUPPORTED
        with pytest.raises(P.DeviceError) as e:
            g.trace_first_hits(16, 16)
        assert e.value.code == N.CGPT_ERR_UNSUPPORTED
        g.reset_accumulator()
        g.render(16, 16, 2, seed=3)
        assert np.array_equal(_bits(g.accumulator()), _bits(acc0))
    finally:
        g.close()


# ---- the replay of DESIGN.md 5.21 through the production walk ---------------------------------------------------------------------------------
def _production_trace(r):
    """replay_ref's trace callable on the probe: extend rays through the extend part of a launch, shadow_tmax rays through the shadow
    part (the replay reads only whether such a ray hit anything)."""
    def trace(o, d, tmax=None):
        if tmax is None:
            return r.trace_rays(o, d)[:4]
        occluded = r.trace_rays(shadow_origins=o, shadow_dirs=d, shadow_tmax=tmax)[4] != 0
        zero = np.zeros(o.shape[0], np.uint32)
        return np.zeros(o.shape[0], np.float32), np.where(occluded, np.uint32(0), np.uint32(NO_HIT)).astype(np.uint32), zero, zero
    return trace


@pytest.mark.parametrize("level", [0, 4])
def test_renders_equal_the_replay_through_the_production_walk(level):
    sc, names = RP.build_scene()
    ds = sc.device_scene()
    r = P.Renderer(0)
    try:
        r.upload(ds)
        ladder = RP.ladder(names)
        for k in range(1, level + 1):
            ladder[k][0](sc); ladder[k][1](r)
        assert sc.lobe_level() == level
        view = RP.VIEWS[0]
        cam = RP.view_camera(ds, view)
        st = S.device_settings(RP.view_settings(view))
        rep = RP.replay(_production_trace(r), r.shade_samples, RP.camera_rays(cam, RP.W, RP.H), RP.W, RP.H, range(RP.H), view["first_sample"], view["n_samples"], RP.SEED, st)
        whole = RP.expected(rep, view, np.arange(RP.H))
        assert whole["acc"][..., :3].any() and whole["rays"] > 2 * RP.W * RP.H * view["n_samples"]
        print(f"level {level}: {len(rep['steps'])} steps, rays {whole['rays']}, unwalked {whole['unwalked']}")
        for kernel in RP.KERNELS:
            RP.assert_render_is(RP.render_view(r, view, cam, st, kernel, False), whole, False, (level, "production walk", "kernel", kernel))
    finally:
        r.close()
        ds.close()
