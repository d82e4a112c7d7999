"""The surface-area cost of a mesh's tree (csrc/host/tree_cost.h), stated in numpy float64 over an exported node array:
(n, 8) uint32 words in the reference's 32-byte layout {aabb_min.xyz, left_first, aabb_max.xyz, prim_count}, node 0 the root, as
Scene.bvh_export and Renderer.export_bvh return them.  The specification of cgpth_tree_cost and cgpt_scene_tree_costs.

    H(box)  = dx dy + dy dz + dz dx, d = float64(max) - float64(min)
    root    = the componentwise min and max of the root's two child boxes
    cost    = (c_inner (H(root) + sum of H(c) over inner children c) + c_tri sum of H(l) n_l over leaf children l) / H(root)

over every child of every splitting node reached from the root.  A root that is a leaf: cost = c_tri n_tris, root_half_area 0."""
from collections import namedtuple

import numpy as np

TreeCost = namedtuple("TreeCost", "cost root_half_area n_inner n_leaves max_leaf_tris")


def half_area(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def reachable_children(nodes):
    """indices of every child of every splitting node reached from the root"""
    left, count = nodes[:, 3], nodes[:, 7]
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        assert count[i] == 0 and 0 < left[i] and left[i] + 1 < len(nodes), i
        for c in (int(left[i]), int(left[i]) + 1):
            out.append(c)
            if count[c] == 0:
                stack.append(c)
        assert len(out) <= len(nodes), "the nodes form no tree"
    return np.array(out, np.int64)


def tree_cost(nodes, c_inner=1.0, c_tri=1.0):
    nodes = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 8)
    lo, hi = nodes[:, 0:3].view(np.float32), nodes[:, 4:7].view(np.float32)
    count = nodes[:, 7].astype(np.int64)
    if count[0] != 0:
        return TreeCost(float(c_tri) * float(count[0]), 0.0, 0, 1, int(count[0]))
    kids = reachable_children(nodes)
    h = half_area(lo[kids], hi[kids])
    inner, leaf = count[kids] == 0, count[kids] != 0
    a, b = int(nodes[0, 3]), int(nodes[0, 3]) + 1
    h_root = float(half_area(np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])))
    with np.errstate(all="ignore"):
        cost = (c_inner * (h_root + float(np.sum(h[inner]))) + c_tri * float(np.sum(h[leaf] * count[kids][leaf]))) / h_root
    return TreeCost(float(cost), h_root, int(inner.sum()) + 1, int(leaf.sum()), int(count[kids][leaf].max()))


def tolerance(n_nodes):
    """Two evaluations of the cost, each with correctly rounded double operations but in any order of summation, differ by at most this
    relative amount.  Every H is a sum of three non-negative products of non-negative exactly representable differences (a double holds
    the difference of two floats of like magnitude exactly; where it rounds, both sides round the same operation the same way), each
    term H n_l one more rounding, so every term of the sums is non-negative and carries the same bits on both sides.  A sum of m
    non-negative terms evaluated in any order has relative error at most (m - 1) u / (1 - (m - 1) u), u = 2^-53 (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2); two orders therefore differ by at most about 2 (m - 1) u = (m - 1) 2^-52 relative.
    m <= n_nodes; the products with the constants, the sum of the two parts and the division add a handful of roundings on each
    side: 16 covers them with room."""
    return (n_nodes + 16) * 2.0 ** -52
