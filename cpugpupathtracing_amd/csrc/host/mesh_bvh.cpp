// mesh_bvh.cpp -- host BVH build reproducing the reference tree bit for bit (see mesh_bvh.h).
//
// Same decisions as ref: Source/BVH.cpp:11-59,188-366, organised differently: an explicit depth-first
// work list instead of recursion (children are numbered in the reference's allocation order: left,
// right, then the whole left subtree before the right one) and cached per-triangle bounds (min/max are
// exact and return the left-most tied operand under any grouping, so no bit changes).
#include "mesh_bvh.h"

#include <cmath>
#include <cstring>
#include <algorithm>
#include <utility>

namespace cgpt {

namespace {

inline Vec3 P(const float p[3]) { return { p[0], p[1], p[2] }; }

// Heron's formula, ref: Source/Primitives.cpp:270-278
float TriangleArea(const cgpt_triangle& t)
{
    float a = length(P(t.v1.pos) - P(t.v0.pos));
    float b = length(P(t.v2.pos) - P(t.v0.pos));
    float c = length(P(t.v2.pos) - P(t.v1.pos));
    float s = (a + b + c) / 2.0f;
    return sqrtf(s * (s - a) * (s - b) * (s - c));
}

// the reference's SAH "volume" is the half surface area, ref: Source/Primitives.cpp:280-284 (SURVEY A-6)
inline float HalfArea(const Vec3& lo, const Vec3& hi)
{
    Vec3 e = hi - lo;
    return e.x * e.y + e.y * e.z + e.z * e.x;
}

// BuildOption_SAHBinned folds bounds under the total order on floats in which -0 < +0: the usual monotone map to uint32 (negative
// floats have all bits flipped, the others the sign bit).  min / max of the keys do not depend on the order of the operands, down to
// the sign of a zero, which is what lets the device build fold with integer atomics (csrc/device/bvh_build.hip).
inline uint32_t OrderKey(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
inline float KeyFloat(uint32_t k)
{
    const uint32_t u = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
struct KeyBounds {              // a box as keys; empty = (all ones, zero), never converted back
    uint32_t lo[3] = { ~0u, ~0u, ~0u }, hi[3] = { 0u, 0u, 0u };
    void Add(const Vec3& l, const Vec3& h)
    {
        for (int k = 0; k < 3; ++k) {
            const uint32_t a = OrderKey(l[k]), b = OrderKey(h[k]);
            if (a < lo[k]) lo[k] = a;
            if (b > hi[k]) hi[k] = b;
        }
    }
    void Add(const KeyBounds& o)
    {
        for (int k = 0; k < 3; ++k) {
            if (o.lo[k] < lo[k]) lo[k] = o.lo[k];
            if (o.hi[k] > hi[k]) hi[k] = o.hi[k];
        }
    }
    Vec3 Lo() const { return { KeyFloat(lo[0]), KeyFloat(lo[1]), KeyFloat(lo[2]) }; }
    Vec3 Hi() const { return { KeyFloat(hi[0]), KeyFloat(hi[1]), KeyFloat(hi[2]) }; }
};

constexpr uint32_t kBins = 16;
// the bin of a centroid coordinate c >= lo; a product that is not below 16 (the last bin's upper edge, an overflowed scale) is bin 15
inline uint32_t BinOf(float c, float lo, float scale)
{
    const float f = (c - lo) * scale;
    return f < 16.0f ? (uint32_t)f : kBins - 1u;
}

}  // namespace

bool MeshBVH::InBinnedDomain(const cgpt_triangle* triangles, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) {
        const cgpt_vertex* v[3] = { &triangles[i].v0, &triangles[i].v1, &triangles[i].v2 };
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a)
                if (!(fabsf(v[k]->pos[a]) <= 1e30f)) return false;                // NaN fails every comparison
    }
    return true;
}

bool MeshBVH::SetTriangles(const std::vector<cgpt_vertex>& vertices, const std::vector<uint32_t>& indices)
{
    nodes_.clear(); triangles_.clear(); tri_indices_.clear(); centroids_.clear(); tri_bounds_.clear();
    nodes_used_ = 0; max_depth_ = 0; total_area_ = 0.0f;

    const size_t n = indices.size() / 3;
    if (n == 0) return false;
    for (size_t k = 0; k < n * 3; ++k)
        if (indices[k] >= vertices.size()) return false;

    triangles_.resize(n);
    tri_indices_.resize(n);
    centroids_.resize(n);
    tri_bounds_.resize(n);
    for (size_t i = 0; i < n; ++i) {
        cgpt_triangle& t = triangles_[i];
        t.v0 = vertices[indices[3 * i]];
        t.v1 = vertices[indices[3 * i + 1]];
        t.v2 = vertices[indices[3 * i + 2]];
        total_area_ += TriangleArea(t);                                       // ref: BVH.cpp:22
        tri_indices_[i] = (uint32_t)i;
        CacheTriangle((uint32_t)i);
    }
    if (option_ == BuildOption_SAHBinned && !InBinnedDomain(triangles_.data(), (uint32_t)n)) {
        triangles_.clear(); tri_indices_.clear(); centroids_.clear(); tri_bounds_.clear();
        total_area_ = 0.0f;
        return false;
    }
    nodes_.assign(2 * n - 1, cgpt_bvh_node{});                                // ref: BVH.cpp:37
    return true;
}

void MeshBVH::CacheTriangle(uint32_t i)
{
    const cgpt_triangle& t = triangles_[i];
    Vec3 p0 = P(t.v0.pos), p1 = P(t.v1.pos), p2 = P(t.v2.pos);
    centroids_[i] = (p0 + p1 + p2) * 0.3333f;                                 // ref: Primitives.cpp:255-258 (SURVEY A-10)
    tri_bounds_[i].lo = vmin(vmin(p0, p1), p2);                               // ref: Primitives.cpp:232-243
    tri_bounds_[i].hi = vmax(vmax(p0, p1), p2);
}

bool MeshBVH::Refit(const cgpt_triangle* triangles, uint32_t n)
{
    if (!triangles || triangles_.empty() || n != triangles_.size()) return false;
    float area = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
        triangles_[i] = triangles[i];
        area += TriangleArea(triangles_[i]);                                  // ref: BVH.cpp:22
        CacheTriangle(i);
    }
    total_area_ = area;
    // children have larger indices than their parent (WellFormed): a reverse sweep sees both children of a node before the node
    for (uint32_t i = nodes_used_; i-- > 0;) {
        cgpt_bvh_node& node = nodes_[i];
        if (node.prim_count > 0) { FitNode(i); continue; }
        const cgpt_bvh_node& l = nodes_[node.left_first];
        const cgpt_bvh_node& r = nodes_[node.left_first + 1];
        for (int k = 0; k < 3; ++k) {
            node.aabb_min[k] = min_std(l.aabb_min[k], r.aabb_min[k]);
            node.aabb_max[k] = max_std(l.aabb_max[k], r.aabb_max[k]);
        }
    }
    return true;
}

bool MeshBVH::Build(const std::vector<cgpt_vertex>& vertices, const std::vector<uint32_t>& indices, BuildOption option)
{
    option_ = option;
    if (!SetTriangles(vertices, indices)) return false;
    if (option_ == BuildOption_SAHBinned) BuildTreeBinned(); else BuildTree();
    return true;
}

// adopt only a well-formed tree: a malformed one would send the device traversal out of bounds
bool MeshBVH::WellFormed(const cgpt_bvh_node* nodes, uint32_t n_nodes, const uint32_t* tri_indices, uint32_t n)
{
    if (n_nodes < 1 || n_nodes > 2 * n - 1) return false;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (tri_indices[i] >= n || seen[tri_indices[i]]) return false;
        seen[tri_indices[i]] = 1;
    }
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const cgpt_bvh_node& node = nodes[i];
        if (node.prim_count == 0) { if (!(node.left_first > i && node.left_first + 1 < n_nodes)) return false; }
        else if (!(node.left_first < n && node.prim_count <= n - node.left_first)) return false;
    }
    return true;
}

bool MeshBVH::BuildWith(const std::vector<cgpt_vertex>& vertices, const std::vector<uint32_t>& indices, BuildOption option, const TreeBuilder& build)
{
    option_ = option;
    if (!SetTriangles(vertices, indices)) return false;
    const uint32_t n = (uint32_t)triangles_.size();
    uint32_t n_nodes = 0, depth = 0;
    const bool ok = build(triangles_.data(), n, (int)option, nullptr, nodes_.data(), &n_nodes, tri_indices_.data(), &depth) &&
                    WellFormed(nodes_.data(), n_nodes, tri_indices_.data(), n);
    if (!ok) {
        nodes_.clear(); triangles_.clear(); tri_indices_.clear(); centroids_.clear(); tri_bounds_.clear();
        nodes_used_ = 0; max_depth_ = 0; total_area_ = 0.0f;
        return false;
    }
    nodes_used_ = n_nodes;
    max_depth_ = depth;
    return true;
}

bool MeshBVH::RebuildWith(BuildOption option, const TreeBuilder& build)       // ref: BVH.cpp:47-59
{
    if (triangles_.empty()) return false;
    const uint32_t n = (uint32_t)triangles_.size();
    std::vector<cgpt_bvh_node> nodes(2 * n - 1);
    std::vector<uint32_t> order(n);
    uint32_t n_nodes = 0, depth = 0;
    if (!build(triangles_.data(), n, (int)option, tri_indices_.data(), nodes.data(), &n_nodes, order.data(), &depth) ||
        !WellFormed(nodes.data(), n_nodes, order.data(), n))
        return false;
    option_ = option;
    nodes_.swap(nodes); tri_indices_.swap(order);
    nodes_used_ = n_nodes;
    max_depth_ = depth;                                                       // m_total_area is not recomputed by Rebuild
    return true;
}

bool MeshBVH::Rebuild(BuildOption option)
{
    if (triangles_.empty()) return true;
    if (option == BuildOption_SAHBinned && !InBinnedDomain(triangles_.data(), (uint32_t)triangles_.size())) return false;
    option_ = option;
    nodes_used_ = 0;
    max_depth_ = 0;
    if (option_ == BuildOption_SAHBinned) BuildTreeBinned(); else BuildTree();
    return true;
}

void MeshBVH::FitNode(uint32_t node_index)                                    // ref: BVH.cpp:188-202
{
    cgpt_bvh_node& node = nodes_[node_index];
    Vec3 lo(1e30f), hi(-1e30f);
    for (uint32_t i = node.left_first; i < node.left_first + node.prim_count; ++i) {
        const Bounds& tb = tri_bounds_[tri_indices_[i]];
        lo = vmin(lo, tb.lo);
        hi = vmax(hi, tb.hi);
    }
    node.aabb_min[0] = lo.x; node.aabb_min[1] = lo.y; node.aabb_min[2] = lo.z;
    node.aabb_max[0] = hi.x; node.aabb_max[1] = hi.y; node.aabb_max[2] = hi.z;
}

float MeshBVH::SplitCost(const cgpt_bvh_node& node, uint32_t axis, float pos) const  // ref: BVH.cpp:299-327
{
    Bounds left, right;
    uint32_t n_left = 0, n_right = 0;
    for (uint32_t i = node.left_first; i < node.left_first + node.prim_count; ++i) {
        const uint32_t tri = tri_indices_[i];
        const Bounds& tb = tri_bounds_[tri];
        if (centroids_[tri][axis] < pos) { ++n_left; left.lo = vmin(left.lo, tb.lo); left.hi = vmax(left.hi, tb.hi); }
        else { ++n_right; right.lo = vmin(right.lo, tb.lo); right.hi = vmax(right.hi, tb.hi); }
    }
    // an empty side has extent -2e30 -> +inf area -> 0 * inf = NaN, which every "<" below rejects
    return (float)n_left * HalfArea(left.lo, left.hi) + (float)n_right * HalfArea(right.lo, right.hi);
}

bool MeshBVH::ChooseSplit(uint32_t node_index, uint32_t& axis, float& pos) const
{
    const cgpt_bvh_node& node = nodes_[node_index];
    const Vec3 lo = P(node.aabb_min), hi = P(node.aabb_max);

    if (option_ == BuildOption_NaiveSplit) {                                  // ref: BVH.cpp:208-224
        if (node.prim_count <= 2) return false;
        Vec3 extent = hi - lo;
        axis = 0;
        if (extent.y > extent.x) axis = 1;
        if (extent.z > extent[axis]) axis = 2;
        pos = lo[axis] + extent[axis] * 0.5f;
        return true;
    }

    const float parent_cost = HalfArea(lo, hi) * (float)node.prim_count;
    float best_cost = 1e30f;
    axis = 0; pos = 0.0f;

    if (option_ == BuildOption_SAHSplitIntervals) {                           // ref: BVH.cpp:225-259
        for (uint32_t k = 0; k < 8; ++k) {
            for (uint32_t a = 0; a < 3; ++a) {
                float width = hi[a] - lo[a];
                float candidate = width * ((float)k / 8) + lo[a];
                float cost = SplitCost(node, a, candidate);
                if (cost < best_cost) { best_cost = cost; axis = a; pos = candidate; }
            }
        }
    } else {                                                                  // ref: BVH.cpp:260-296
        for (uint32_t i = node.left_first; i < node.left_first + node.prim_count; ++i) {
            const Vec3& c = centroids_[tri_indices_[i]];
            for (uint32_t a = 0; a < 3; ++a) {
                float cost = SplitCost(node, a, c[a]);
                // the reference records axis/pos but never the cost (SURVEY A-5), so best_cost stays 1e30
                if (cost < best_cost) { axis = a; pos = c[a]; }
            }
        }
    }
    return !(best_cost >= parent_cost);                                       // ref: BVH.cpp:253,290
}

uint32_t MeshBVH::Partition(const cgpt_bvh_node& node, uint32_t axis, float pos)  // ref: BVH.cpp:331-344
{
    int32_t i = (int32_t)node.left_first;
    int32_t j = i + (int32_t)node.prim_count - 1;
    while (i <= j) {
        if (centroids_[tri_indices_[i]][axis] < pos) ++i;
        else std::swap(tri_indices_[i], tri_indices_[j--]);
    }
    return (uint32_t)i;
}

void MeshBVH::BuildTree()
{
    cgpt_bvh_node& root = nodes_[nodes_used_++];                              // ref: BVH.cpp:39-44
    root.left_first = 0;
    root.prim_count = (uint32_t)triangles_.size();
    FitNode(0);

    struct Work { uint32_t node, depth; };
    std::vector<Work> todo;
    todo.push_back({ 0, 0 });
    while (!todo.empty()) {
        const Work w = todo.back();
        todo.pop_back();
        if (w.depth > max_depth_) max_depth_ = w.depth;                       // ref: BVH.cpp:206

        uint32_t axis; float pos;
        if (!ChooseSplit(w.node, axis, pos)) continue;

        cgpt_bvh_node& node = nodes_[w.node];
        const uint32_t mid = Partition(node, axis, pos);
        const uint32_t n_left = mid - node.left_first;
        if (n_left == 0 || n_left == node.prim_count) continue;               // ref: BVH.cpp:346-348

        const uint32_t left = nodes_used_++, right = nodes_used_++;           // ref: BVH.cpp:350-359
        nodes_[left].left_first = node.left_first;
        nodes_[left].prim_count = n_left;
        nodes_[right].left_first = mid;
        nodes_[right].prim_count = node.prim_count - n_left;
        node.left_first = left;
        node.prim_count = 0;
        FitNode(left);
        FitNode(right);
        todo.push_back({ right, w.depth + 1 });                               // left subtree is numbered first
        todo.push_back({ left, w.depth + 1 });
    }
}

// ---- BuildOption_SAHBinned (the reference's README, "Planned: Binned BVH build"; the specification of the device build) ----------
// Per node: the bounds of its triangles' centroids give, per axis with a positive extent, 16 equal bins; each bin keeps a count, the
// union of its triangles' boxes and the bounds of their centroids.  Candidates: axis outer, split s = 1..15 inner, left = bins [0, s);
// an empty side is skipped; the reference's cost expression (ref: BVH.cpp:325) and leaf criterion (:253); the first strictly cheaper
// candidate wins.  The partition is stable and the children's bounds are the unions of the bins on each side, so nothing but the
// partition reads the triangles a second time.  Every min / max is taken on OrderKey, so no result depends on the order of the fold.
void MeshBVH::BuildTreeBinned()
{
    struct Bin {
        uint32_t count = 0; KeyBounds box, cen;
        void Add(const Bin& o) { count += o.count; box.Add(o.box); cen.Add(o.cen); }
    };
    struct Work { uint32_t node, depth; KeyBounds cen; };

    const uint32_t n_all = (uint32_t)triangles_.size();
    std::vector<uint32_t> left_part, right_part;
    std::vector<Work> todo;
    {
        KeyBounds box, cen;
        for (uint32_t i = 0; i < n_all; ++i) {
            const uint32_t tri = tri_indices_[i];
            box.Add(tri_bounds_[tri].lo, tri_bounds_[tri].hi);
            cen.Add(centroids_[tri], centroids_[tri]);
        }
        cgpt_bvh_node& root = nodes_[nodes_used_++];
        root.left_first = 0;
        root.prim_count = n_all;
        const Vec3 lo = box.Lo(), hi = box.Hi();
        for (int k = 0; k < 3; ++k) { root.aabb_min[k] = lo[k]; root.aabb_max[k] = hi[k]; }
        todo.push_back({ 0, 0, cen });
    }
    while (!todo.empty()) {
        const Work w = todo.back();
        todo.pop_back();
        if (w.depth > max_depth_) max_depth_ = w.depth;

        cgpt_bvh_node& node = nodes_[w.node];
        const uint32_t first = node.left_first, n = node.prim_count;
        const Vec3 cmin = w.cen.Lo(), cmax = w.cen.Hi();
        Bin bins[3][kBins];
        float scale[3] = { 0.0f, 0.0f, 0.0f };
        for (uint32_t a = 0; a < 3; ++a)
            if (cmax[a] > cmin[a]) scale[a] = 16.0f / (cmax[a] - cmin[a]);
        for (uint32_t i = first; i < first + n; ++i) {
            const uint32_t tri = tri_indices_[i];
            for (uint32_t a = 0; a < 3; ++a) {
                if (!(cmax[a] > cmin[a])) continue;
                Bin& b = bins[a][BinOf(centroids_[tri][a], cmin[a], scale[a])];
                ++b.count;
                b.box.Add(tri_bounds_[tri].lo, tri_bounds_[tri].hi);
                b.cen.Add(centroids_[tri], centroids_[tri]);
            }
        }

        float best = INFINITY;
        uint32_t best_axis = 0, best_s = 0;
        Bin best_l, best_r;
        for (uint32_t a = 0; a < 3; ++a) {
            if (!(cmax[a] > cmin[a])) continue;
            Bin suffix[kBins + 1];                                                // suffix[b]: bins [b, 16); an empty bin is the identity
            for (uint32_t b = kBins; b-- > 1;) { suffix[b] = suffix[b + 1]; suffix[b].Add(bins[a][b]); }
            Bin l;
            for (uint32_t s = 1; s < kBins; ++s) {
                l.Add(bins[a][s - 1]);
                const Bin& r = suffix[s];
                if (l.count == 0 || r.count == 0) continue;
                const float cost = (float)l.count * HalfArea(l.box.Lo(), l.box.Hi()) + (float)r.count * HalfArea(r.box.Lo(), r.box.Hi());
                if (cost < best) { best = cost; best_axis = a; best_s = s; best_l = l; best_r = r; }
            }
        }
        if (!(best < HalfArea(P(node.aabb_min), P(node.aabb_max)) * (float)n)) continue;     // leaf (ref: BVH.cpp:253); also: no candidate

        left_part.clear(); right_part.clear();                                    // stable: both sides keep their relative order
        for (uint32_t i = first; i < first + n; ++i) {
            const uint32_t tri = tri_indices_[i];
            (BinOf(centroids_[tri][best_axis], cmin[best_axis], scale[best_axis]) < best_s ? left_part : right_part).push_back(tri);
        }
        std::copy(left_part.begin(), left_part.end(), tri_indices_.begin() + first);
        std::copy(right_part.begin(), right_part.end(), tri_indices_.begin() + first + left_part.size());

        const uint32_t left = nodes_used_++, right = nodes_used_++;             // the other options' numbering (ref: BVH.cpp:350-359)
        const Bin* side[2] = { &best_l, &best_r };
        for (uint32_t c = 0; c < 2; ++c) {
            cgpt_bvh_node& child = nodes_[left + c];
            child.left_first = c == 0 ? first : first + best_l.count;
            child.prim_count = side[c]->count;
            const Vec3 lo = side[c]->box.Lo(), hi = side[c]->box.Hi();
            for (int k = 0; k < 3; ++k) { child.aabb_min[k] = lo[k]; child.aabb_max[k] = hi[k]; }
        }
        node.left_first = left;
        node.prim_count = 0;
        todo.push_back({ right, w.depth + 1, best_r.cen });                       // left subtree is numbered first
        todo.push_back({ left, w.depth + 1, best_l.cen });
    }
}

}  // namespace cgpt
