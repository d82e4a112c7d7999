"""tests/tree_cost_ref.py -- the statement of the tree-cost metric -- held to closed forms worked by hand here."""
import numpy as np

from tree_cost_ref import half_area, tolerance, tree_cost


def node(lo, hi, left_first, prim_count):
    w = np.zeros(8, np.uint32)
    w[0:3] = np.float32(lo).view(np.uint32); w[4:7] = np.float32(hi).view(np.uint32)
    w[3], w[7] = left_first, prim_count
    return w


def two_leaves(scale=1.0):
    """root -> leaf [0,0,0]-[1,2,3] with 3 triangles, leaf [2,0,0]-[4,1,1] with 2"""
    s = np.float32(scale)
    return np.stack([node(np.float32([0, 0, 0]) * s, np.float32([4, 2, 3]) * s, 1, 0),
                     node(np.float32([0, 0, 0]) * s, np.float32([1, 2, 3]) * s, 0, 3),
                     node(np.float32([2, 0, 0]) * s, np.float32([4, 1, 1]) * s, 3, 2)])


def three_levels(scale=1.0):
    """root -> {inner [0,0,0]-[2,2,2] -> {leaf [0,0,0]-[1,2,2] x 1, leaf [1,0,0]-[2,2,2] x 5}, flat leaf [3,0,1]-[5,2,1] x 4}"""
    s = np.float32(scale)
    return np.stack([node(np.float32([0, 0, 0]) * s, np.float32([5, 2, 2]) * s, 1, 0),
                     node(np.float32([0, 0, 0]) * s, np.float32([2, 2, 2]) * s, 3, 0),
                     node(np.float32([3, 0, 1]) * s, np.float32([5, 2, 1]) * s, 6, 4),
                     node(np.float32([0, 0, 0]) * s, np.float32([1, 2, 2]) * s, 0, 1),
                     node(np.float32([1, 0, 0]) * s, np.float32([2, 2, 2]) * s, 1, 5)])


def test_half_area():
    assert half_area(np.float32([0, 0, 0]), np.float32([1, 2, 3])) == 1 * 2 + 2 * 3 + 3 * 1
    assert half_area(np.float32([3, 0, 1]), np.float32([5, 2, 1])) == 4.0           # flat in z: the one face


def test_a_root_with_two_leaf_children():
    # H(left) = 2 + 6 + 3 = 11, H(right) = 2 + 1 + 2 = 5, the root box [0,0,0]-[4,2,3]: H = 8 + 6 + 12 = 26
    got = tree_cost(two_leaves())
    assert got == (((26.0) + (11.0 * 3 + 5.0 * 2)) / 26.0, 26.0, 1, 2, 3)
    got = tree_cost(two_leaves(), c_inner=2.0, c_tri=0.5)
    assert got.cost == (2.0 * 26.0 + 0.5 * 43.0) / 26.0


def test_the_root_box_comes_from_the_two_children_not_from_node_0():
    nodes = two_leaves()
    nodes[0] = node([-100, -100, -100], [100, 100, 100], 1, 0)
    assert tree_cost(nodes) == tree_cost(two_leaves())


def test_three_levels_with_a_flat_box():
    # root box [0,0,0]-[5,2,2]: H = 10 + 4 + 10 = 24; inner child H = 12; leaves: flat 4 x 4, 8 x 1, 8 x 5
    got = tree_cost(three_levels())
    assert got == ((24.0 + 12.0 + 16.0 + 8.0 + 40.0) / 24.0, 24.0, 2, 3, 5)
    got = tree_cost(three_levels(), c_inner=3.0, c_tri=0.25)
    assert got.cost == (3.0 * 36.0 + 0.25 * 64.0) / 24.0


def test_a_leaf_root():
    nodes = node([0, 0, 0], [1, 1, 1], 0, 7)[None]
    assert tree_cost(nodes) == (7.0, 0.0, 0, 1, 7)
    assert tree_cost(nodes, c_inner=5.0, c_tri=0.5) == (3.5, 0.0, 0, 1, 7)


def test_the_cost_does_not_change_with_scale():
    for make in (two_leaves, three_levels):
        assert tree_cost(make(2.0)).cost == tree_cost(make()).cost            # a power of two: exactly
        assert tree_cost(make(2.0)).root_half_area == 4.0 * tree_cost(make()).root_half_area
        assert tree_cost(make(0.125)).cost == tree_cost(make()).cost


def test_unreached_nodes_are_not_counted():
    nodes = np.concatenate([two_leaves(), node([0, 0, 0], [9, 9, 9], 0, 50)[None]])
    assert tree_cost(nodes) == tree_cost(two_leaves())


def test_the_tolerance_is_the_derived_one():
    assert tolerance(1279) == (1279 + 16) * 2.0 ** -52
