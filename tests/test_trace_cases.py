"""The ray sets of tests/trace_cases.py against the oracle alone: each set does what it is for, so a pass of tests/test_gpu_trace_probe.py
cannot be an empty pass (DESIGN.md 5.22 has the measured values)."""
import numpy as np
import pytest

import trace_cases as TC

NO_HIT = TC.NO_HIT


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("level", [2, 4])
def test_a_quarter_of_the_parity_rays_hit(level):
    o, d = TC.parity_rays()
    _, obj, _, _ = TC.parity_hits(level)
    share = float((obj != NO_HIT).mean())
    print(f"level {level}: {o.shape[0]} rays, hit share {share:.4f}, objects hit {np.unique(obj[obj != NO_HIT]).tolist()}")
    assert o.shape[0] == 20000 and share > 0.25
    assert np.all(np.isfinite(d)) and np.all(np.abs(d).sum(1) > 0)


@pytest.mark.parametrize("level", [2, 4])
def test_zero_component_rays_have_zeros_of_both_signs_and_start_on_the_root_box(level):
    orc, s = TC.parity_pair(level)
    o, d = TC.zero_component_rays(level)
    zeros = (d == 0).sum(1)
    assert np.all(np.isfinite(d)) and np.all(np.abs(d).sum(1) > 0)
    assert (zeros[:768] == 1).sum() == 384 and (zeros[:768] == 2).sum() == 384
    assert np.signbit(d[d == 0]).sum() > 100 and (~np.signbit(d[d == 0])).sum() > 100
    lo, hi = TC.root_box(s)
    on_face = ((o[768:] == lo) | (o[768:] == hi)).any(1)
    assert on_face.all() and ((d[768:] == 0).sum(1) == 1).sum() >= 100
    _, obj, _, dep = orc.intersect_rays(o, d)
    print(f"level {level}: {o.shape[0]} rays, {int((obj == 0).sum())} hit the mesh, {int((obj != NO_HIT).sum())} hit anything, "
          f"face rays that hit the mesh {int((obj[768:] == 0).sum())}")
    assert (obj[:768] == 0).sum() > 50 and (obj[768:] == 0).sum() > 50 and (obj == NO_HIT).sum() > 50


def test_tmax_one_float_either_side_of_a_hit_flips_it():
    for level in (2, 4):
        orc, _ = TC.parity_pair(level)
        o, d, tmax = TC.tmax_edge_rays(level)
        n = o.shape[0] // 5
        t, obj, _, _ = orc.intersect_rays(o, d, tmax)
        hit = (obj != NO_HIT).reshape(5, n)
        flips = int((~hit[0] & hit[2]).sum())
        print(f"level {level}: {n} rays per kind; hits at tmax = t {int(hit[0].sum())}, below {int(hit[1].sum())}, above {int(hit[2].sum())}, "
              f"t / 2 {int(hit[3].sum())}, 1e34 {int(hit[4].sum())}; flips between t and the float above: {flips}")
        assert flips >= 100 and hit[4].all()
        assert np.array_equal(_bits(t.reshape(5, n)[2][hit[2]]), _bits(tmax[:n][hit[2]]))   # the hit found again is the hit the tmax came from


def test_nee_shadow_rays_are_partly_occluded():
    for level in (2, 4):
        orc, _ = TC.parity_pair(level)
        o, d, tmax = TC.nee_shadow_rays(level)
        _, obj, _, _ = orc.intersect_rays(o, d, tmax)
        occluded = int((obj != NO_HIT).sum())
        print(f"level {level}: {o.shape[0]} shadow rays from surfaces, {occluded} occluded")
        assert 100 < occluded < o.shape[0] - 100


def test_deep_stack_rays_walk_deeper_than_the_lds_levels():
    orc, s = TC.deep_pair()
    assert s.bvh_info(0).max_depth >= 17
    o, d = TC.deep_rays()
    _, obj, _, dep = orc.intersect_rays(o, d)
    print(f"{o.shape[0]} rays: bvh_depth min {dep.min()} median {int(np.median(dep))} max {dep.max()}; {int((dep >= 17).sum())} at 17 or more; "
          f"{int((obj == 0).sum())} hit the stack")
    assert (dep >= 17).sum() >= 200 and (obj == 0).sum() >= 200


def test_tie_scenes_hold_candidates_of_equal_t():
    o, d = TC.twin_quad_rays()
    both = TC.twin_quad_pair()[0].intersect_rays(o, d)
    a = TC.twin_quad_pair((3,))[0].intersect_rays(o, d)
    b = TC.twin_quad_pair((17,))[0].intersect_rays(o, d)
    tie = (a[1] == 3) & (b[1] == 17) & (_bits(a[0]) == _bits(b[0]))
    print(f"twin quads: {int(tie.sum())} of {o.shape[0]} rays hit objects 3 and 17 at equal t bits; reported: {np.unique(both[1][tie]).tolist()}")
    assert tie.sum() >= 400 and np.all(both[1][tie] == 3)                       # strict t <, first in visiting order

    o, d = TC.coincident_rays()
    many = TC.coincident_pair()[0].intersect_rays(o, d)
    one = TC.coincident_pair(1)[0].intersect_rays(o, d)
    tie = (one[1] == 0) & (many[1] == 0) & (_bits(one[0]) == _bits(many[0]))
    print(f"coincident triangles: {int(tie.sum())} of {o.shape[0]} rays hit all {TC.COINCIDENT_COPIES} copies at one t; reported tri {np.unique(many[2][tie]).tolist()}; "
          f"{int((many[1] == 1).sum())} reach the plane behind")
    assert tie.sum() >= 50 and (many[1] == 1).sum() >= 50 and np.array_equal(one[1], many[1])
    assert TC.coincident_pair()[1].bvh_info(0).max_leaf_size == TC.COINCIDENT_COPIES


def test_forty_objects_are_more_than_the_lds_table_holds():
    orc, s = TC.forty_pair()
    o, d = TC.forty_rays()
    _, obj, _, _ = orc.intersect_rays(o, d)
    kinds = np.unique(obj[obj != NO_HIT])
    print(f"{o.shape[0]} rays hit {kinds.size} of 40 objects; misses {int((obj == NO_HIT).sum())}")
    assert s.flatten().n_objects == 40 > 31 and kinds.size >= 30 and kinds.max() >= 32


def test_round0_frames_have_hits_misses_and_padded_tiles():
    pads = set()
    for view in (0, 1):
        for W, H, rows in TC.ROUND0_FRAMES:
            obj = TC.round0_want(view, W, H, rows)["records"][0]
            n_rows = obj.shape[0]
            pad = TC.padded_tiles(W, n_rows)
            pads.add((pad[0] > 0, pad[1] > 0))
            hits = int((obj != NO_HIT).sum())
            print(f"view {view} {W}x{H} rows {rows}: {hits} hits, {obj.size - hits} misses, padding {pad}, objects {np.unique(obj[obj != NO_HIT]).tolist()}")
            if rows is None and W * H > 1:                                      # (one pixel is one or the other; the band of rows is checked for hits)
                assert 0 < hits < obj.size, (view, W, H, rows)
            elif rows is not None:
                assert hits > 0, (view, W, H, rows)
    assert (True, True) in pads


def test_tiled_rays_are_new_rays_of_the_same_population():
    o, d = TC.parity_rays()
    n = TC.rays_beyond_one_block_per_wave(256)
    assert n == 70000
    oo, dd = TC.tiled(o, d, n)
    assert oo.shape == dd.shape == (n, 3) and np.array_equal(oo[:20000], o) and not np.array_equal(oo[20000:40000], o)
    assert np.array_equal(dd[20000:40000], d)
