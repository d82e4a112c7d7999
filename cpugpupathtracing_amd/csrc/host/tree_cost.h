// tree_cost.h -- the surface-area cost of a mesh's tree: the metric, stated once for the host mirror (host_capi.cpp: cgpth_tree_cost) and
// the device kernels (csrc/device/tree_cost.hip), which share the per-node term below as animation.h's users share its sampler.
// tests/tree_cost_ref.py states the same in numpy float64; DESIGN.md 5.36.
//
// For a mesh whose root split, all in double from the float bounds:
//   half area   H(box) = dx*dy + dy*dz + dz*dx,  d = (double)max - (double)min       (the builder's "volume", mesh_bvh.cpp: HalfArea, ref: Primitives.cpp:280-284)
//   root box    the componentwise min and max of the root's two child boxes (b < a ? b : a and a < b ? b : a): the device holds no other
//   cost        (c_inner * (H(root) + sum of H(c) over inner children c) + c_tri * sum of H(l) * n_l over leaf children l) / H(root)
// over every child box of every splitting node; n_l is the leaf's triangle count.  It is the expected work of a ray that hits the root
// box, in units of c_inner per node visited and c_tri per triangle tested (Goldsmith & Salmon 1987, MacDonald & Booth 1990), and does not
// change when the mesh is scaled.  A mesh whose root is a leaf has no child box: its cost is c_tri * n_tris and its root_half_area is
// reported as 0.
// The counts: n_inner = the splitting nodes (the root among them), n_leaves = the leaves, max_leaf_tris = the largest n_l.
// How the sums are formed is each implementation's own: the mirror adds the terms in double while it walks the tree and divides once; the
// device divides every term by H(root) first and adds the quotients exactly, as integers, so that its bits do not depend on the order in
// which it meets the records (tree_cost.hip).  Every term is non-negative, so any two such evaluations differ by at most
// (terms + a few) * 2^-52 relative (tests/tree_cost_ref.py: tolerance derives the bound).
// The builders use no constants of their own: their split criterion compares count * H of the two sides with the parent's (mesh_bvh.cpp:
// ShouldSplit, the binned build), which is c_tri = 1 with no term for the traversal.  The defaults below are the conventional unit costs.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIP__
#define CGPT_TREE_COST_FN __host__ __device__ inline
#else
#define CGPT_TREE_COST_FN inline
#endif

namespace cgpt {

constexpr double kTreeCostInnerDefault = 1.0;   // c_inner: one node visited
constexpr double kTreeCostTriDefault = 1.0;     // c_tri: one triangle tested

CGPT_TREE_COST_FN double TreeCostHalfArea(float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const double dx = (double)hix - (double)lox, dy = (double)hiy - (double)loy, dz = (double)hiz - (double)loz;
    return dx * dy + dy * dz + dz * dx;
}

// What one child box adds to the two sums and the counts: a leaf child holds n_l = leaf_tris > 0 triangles, an inner child 0.
struct TreeCostSums {
    double inner = 0.0, leaf = 0.0;             // sum of H(c) over inner children; sum of H(l) * n_l over leaf children
    uint32_t n_inner_children = 0, n_leaves = 0, max_leaf_tris = 0;
};
CGPT_TREE_COST_FN void TreeCostAddChild(TreeCostSums& s, double half_area, uint32_t leaf_tris)
{
    if (leaf_tris == 0u) { s.inner += half_area; s.n_inner_children += 1u; return; }
    s.leaf += half_area * (double)leaf_tris;
    s.n_leaves += 1u;
    if (leaf_tris > s.max_leaf_tris) s.max_leaf_tris = leaf_tris;
}

// the root box's half area from the root's two child boxes
CGPT_TREE_COST_FN double TreeCostRootHalfArea(const float l_lo[3], const float l_hi[3], const float r_lo[3], const float r_hi[3])
{
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) { lo[k] = r_lo[k] < l_lo[k] ? r_lo[k] : l_lo[k]; hi[k] = l_hi[k] < r_hi[k] ? r_hi[k] : l_hi[k]; }
    return TreeCostHalfArea(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
}

CGPT_TREE_COST_FN double TreeCostTotal(double c_inner, double c_tri, double root_half_area, double inner_sum, double leaf_sum)
{
    return (c_inner * (root_half_area + inner_sum) + c_tri * leaf_sum) / root_half_area;
}

inline bool TreeCostConstantOk(double c) { return std::isfinite(c) && c > 0.0; }

}  // namespace cgpt
