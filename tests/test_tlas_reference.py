"""The numpy model of the top-level tree (tests/tlas_ref.py) against its own list walk: the tree only skips, so the two
walks give the same (t, obj, tri, depth) for every ray -- the condition is zero differing rays."""
import numpy as np
import pytest

import tlas_ref as TL
import tlas_scenes as TS


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def forty():
    spec = TL.forty_objects()
    scene, model = TS.to_scene(spec, lamp=1)
    rays, axis = TS.all_rays(model)
    yield spec, model, rays, axis
    scene.close()


def test_the_forty_objects_are_what_the_issue_asks_for(forty):
    spec, model, _, _ = forty
    kinds = [ob["kind"] if ob["kind"] != "mesh" else ob["shape"] for ob in spec]
    assert len(spec) == 40 and kinds.count("plane") == 2 and kinds.count("sphere") == 10 and kinds.count("triangle") == 8
    assert kinds.count("quad") == 10 and kinds.count("box") == 10
    moved = [ob for ob in spec if ob.get("transform") is not None]
    assert len(moved) == 13
    dets = [np.linalg.det(np.asarray(ob["transform"], np.float64)[:, :3]) for ob in moved]
    assert min(dets) < 0                                                       # a mirror
    sv = [np.linalg.svd(np.asarray(ob["transform"], np.float64)[:, :3], compute_uv=False) for ob in moved]
    assert any(abs(s[0] / s[2] - 5.0) < 1e-5 for s in sv)                      # a 1:5 non-uniform scale
    assert np.isinf(model.leaf_boxes[0]).all() and np.isinf(model.leaf_boxes[20]).all() and np.isfinite(np.delete(model.leaf_boxes, [0, 20], 0)).all()


def test_tree_walk_equals_list_walk_on_every_ray(forty):
    _, model, (o, d, tmax), (ao, ad) = forty
    assert o.shape[0] == 4096 and ao.shape[0] == 256
    zeros = (ad == 0.0).sum(-1)
    assert set(np.unique(zeros)) == {1, 2}
    assert (tmax < 1e33).sum() >= 512                                          # rays with a finite tmax
    a = model.walk(o, d, tmax, tree=False)
    b = model.walk(o, d, tmax, tree=True)
    differ = (_bits(a[0]) != _bits(b[0])) | (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3])
    print(f"random rays: {int(differ.sum())} of {o.shape[0]} differ; hit rate {(a[1] != TL.NO_HIT).mean():.3f}; objects tested per ray "
          f"{a[4]['leaves'].mean():.1f} -> {b[4]['leaves'].mean():.2f}; mesh inner steps {a[4]['inner']} -> {b[4]['inner']}")
    assert differ.sum() == 0
    assert len(np.unique(a[1])) >= 30 and a[3].max() >= 3                      # the rays reach most objects, and below the mesh roots
    on_surface = slice(4096 - 512, 4096)                                       # the rays that start on a surface
    assert (a[1][on_surface] != TL.NO_HIT).mean() > 0.3
    assert b[4]["leaves"].mean() < 0.25 * a[4]["leaves"].mean()                # and the tree does skip
    assert a[4]["inner"] - b[4]["inner"] == b[4]["skipped_inner_roots"] > 0    # one root step per skipped inner-root mesh
    assert a[4]["tris"] == b[4]["tris"]
    a2 = model.walk(ao, ad, None, tree=False)
    b2 = model.walk(ao, ad, None, tree=True)
    differ2 = (_bits(a2[0]) != _bits(b2[0])) | (a2[1] != b2[1]) | (a2[2] != b2[2]) | (a2[3] != b2[3])
    print(f"rays with zero direction components: {int(differ2.sum())} of {ao.shape[0]} differ; hit rate {(a2[1] != TL.NO_HIT).mean():.3f}")
    assert differ2.sum() == 0 and (a2[1] != TL.NO_HIT).mean() > 0.5


def test_tree_walk_equals_list_walk_on_shadow_rays_from_far_out_on_the_ground_plane(forty):
    """From 10^4 to 10^6 units away the list walk's sphere test reports hits on spheres the ray passes far from; the node test's FAR_PAD
    keeps the tree from skipping them (with FAR_PAD = 0 this test finds differing rays)."""
    _, model, _, _ = forty
    o, d, tmax = TL.far_rays()
    a = model.walk(o, d, tmax, tree=False)
    b = model.walk(o, d, tmax, tree=True)
    differ = (_bits(a[0]) != _bits(b[0])) | (a[1] != b[1]) | (a[2] != b[2]) | (a[3] != b[3])
    spheres = [k for k, ob in enumerate(model.spec) if ob["kind"] == "sphere" and k != 1]
    spurious = np.isin(a[1], spheres)                                          # none of them lies between the plane's far field and the lamp
    print(f"far shadow rays: {int(differ.sum())} of {o.shape[0]} differ; {int(spurious.sum())} report a sphere other than the lamp; "
          f"objects tested per ray {a[4]['leaves'].mean():.1f} -> {b[4]['leaves'].mean():.2f}")
    assert differ.sum() == 0
    assert spurious.sum() > 0                                                  # (a condition on the rays: the list walk does err on some)


def test_an_axis_parallel_ray_visits_every_leaf(forty):
    _, model, _, (ao, ad) = forty
    _, _, _, _, info = model.walk(ao, ad, None, tree=True)
    assert np.all(info["leaves"] == model.n)
    o = np.array([[0.3, 30.0, 0.2]], np.float32); d = np.array([[0.0, -1.0, 0.0]], np.float32)
    assert model.walk(o, d, None, tree=True)[4]["leaves"][0] == 40
    d2 = np.array([[1e-3, -1.0, 1e-3]], np.float32); d2 /= np.linalg.norm(d2)
    assert model.walk(o, d2, None, tree=True)[4]["leaves"][0] < 40             # its neighbour with no zero component skips


def test_tree_shape_and_entry_table():
    for n in (1, 2, 3, 5, 31, 32, 40):
        rng = np.random.default_rng(n)
        lo = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
        boxes = np.concatenate([lo, lo + rng.uniform(0.1, 1, (n, 3)).astype(np.float32)], 1)
        nodes, entry = TL.build_tree(boxes)
        words = nodes.view(np.uint32)
        assert nodes.shape == (2 * n - 1, 8) and entry.shape == (n + 1,) and entry[0] == 0 and entry[n] == 2 * n - 1
        leaves = np.nonzero(words[:, 7] != TL.INNER)[0]
        assert np.array_equal(words[leaves, 7], np.arange(n))                 # preorder meets the objects in index order
        assert np.array_equal(words[leaves, 3], leaves + 1)
        assert np.array_equal(entry[1:], leaves + 1)                          # entry[o + 1] is the node behind leaf o
        assert np.all(words[:, 3] > np.arange(2 * n - 1)) and words[0, 3] == 2 * n - 1
        for k in range(2 * n - 1):                                            # a node's box holds every box below it
            below = slice(k, int(words[k, 3]))
            assert np.all(nodes[below, 0:3] >= nodes[k, 0:3]) and np.all(nodes[below, 4:7] <= nodes[k, 4:7])


def test_a_morton_ordered_forest_visits_fewer_than_a_third_of_the_leaves():
    spec = TL.forest_of_boxes(64, spacing=6.0)
    scene, shuffled = TS.to_scene([dict(ob) for ob in spec])
    order = TL.morton_order(shuffled.leaf_boxes)
    assert sorted(order.tolist()) == list(range(64))
    scene2, ordered = TS.to_scene([dict(spec[k]) for k in order])
    try:
        o, d, _ = TL.random_rays(1024, seed=9, radius=40.0, target=14.0)
        ts, objs, _, _, info_s = shuffled.walk(o, d, None, tree=True)
        to, objo, _, _, info_o = ordered.walk(o, d, None, tree=True)
        tl, objl, _, _, _ = ordered.walk(o, d, None, tree=False)
        print(f"per ray, of 64 leaves and 127 nodes: Morton order {info_o['leaves'].mean():.2f} leaves, {info_o['nodes'].mean():.1f} nodes; "
              f"shuffled {info_s['leaves'].mean():.2f} leaves, {info_s['nodes'].mean():.1f} nodes")
        assert np.array_equal(_bits(to), _bits(tl)) and np.array_equal(objo, objl)
        assert np.array_equal(_bits(to), _bits(ts)) and np.array_equal(order[objo[objo != TL.NO_HIT]], objs[objs != TL.NO_HIT])   # the same boxes are hit
        assert 0.1 < (objo != TL.NO_HIT).mean() < 0.95                       # (a condition on the scene: enough rays hit a box, enough miss)
        assert info_o["leaves"].mean() < 64 / 3.0
        assert info_o["nodes"].mean() < 0.5 * info_s["nodes"].mean()          # a leaf is visited when its own box is hit, in any order: the order pays in the nodes met
    finally:
        scene.close(); scene2.close()


def test_padding_is_outward_and_unbounded_where_it_must_be():
    box = np.array([1.0, -2.0, 0.0, 3.0, -1.0, 0.0], np.float32)                 # a flat box: its zero extent is padded too
    p = TL.pad_box(box)
    assert np.all(p[:3] < box[:3]) and np.all(p[3:] > box[3:])
    assert np.isinf(TL.pad_box(np.array([0, 0, 0, np.inf, 1, 1], np.float32))).all()
    assert np.isinf(TL.pad_box(np.array([0, 0, 0, np.nan, 1, 1], np.float32))).all()
    assert np.isinf(TL.pad_box(np.array([-3e38, 0, 0, 3e38, 1, 1], np.float32))).all()       # hi - lo overflows
    assert np.isinf(TL.leaf_box({"kind": "plane"})).all()
    m = np.array([[0, -2, 0, 5], [2, 0, 0, 1], [0, 0, 1, -3]], np.float32)          # a quarter turn, scaled, shifted
    w = TL.transform_box(m, np.array([0, 0, 0, 1, 1, 1], np.float32))
    assert np.array_equal(w, np.array([3, 1, -3, 5, 3, -2], np.float32))
